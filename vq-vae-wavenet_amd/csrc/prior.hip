// The latent prior's input stage (prior.py): a causal conv over one-hot codes that never materialises the one-hot tensor.
//
//   net0[b][:][t] = b_pre + sum_{j < pre_k} W_pre[j][c[b][t - pre_k + j]][:]      (terms with t - pre_k + j < 0 omitted)
//
// i.e. conv1d_v2(one_hot(shift_right(c)), W_pre, b_pre) with CAUSAL padding (wavenet_ops.py:59-90): tap pre_k-1 meets the
// previous code.  Codes outside [0, k) contribute nothing (the gathers stay inside W_pre).
//
// Forward: HBM-bound.  A block covers 64 time steps x 64 channels of one batch row: the gathers read 256-byte row segments of
// W_pre (R-contiguous), the tile is transposed through LDS, and the [B][R][T] writes are 256-byte time-contiguous segments.
// Weight gradient: dW[j][q][:] = sum_{(b,s) : c[b][s] = q, s + pre_k - j < T} dnet[b][:][s + pre_k - j], over the positions of
// code q in a fixed (stable-sorted) order, one block per (q, j), one channel per thread: deterministic, no atomics.  It reads
// dnet transposed to [B][T][R] so that every position is one R-contiguous row.
#include "vqw_common.h"

namespace {

constexpr int PT = 64;    // time steps per forward block
constexpr int PC = 64;    // channels per forward block

__global__ __launch_bounds__(256) void prior_input_fwd_kernel(const int32_t* __restrict__ codes, const float* __restrict__ w,
                                                              const float* __restrict__ bias, float* __restrict__ net0,
                                                              int32_t* __restrict__ labels, int T, int k, int R, int pre_k) {
    __shared__ float tile[PC][PT + 1];
    const int t0 = blockIdx.x * PT, c0 = blockIdx.y * PC, b = blockIdx.z, tid = threadIdx.x;
    const int32_t* cb = codes + (size_t)b * T;
    // gather: thread (tt, cq) sums 4 consecutive channels of time t0 + tt (16 threads = one 256-byte row segment per tap)
    const int cq = (tid & 15) * 4;
    const bool vec = (R % 4 == 0) && (c0 + cq + 3 < R);
    for (int tt = tid >> 4; tt < PT; tt += 16) {
        const int t = t0 + tt;
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (t < T) {
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] = (c0 + cq + q < R) ? bias[c0 + cq + q] : 0.0f;
            for (int j = 0; j < pre_k; ++j) {
                const int s = t - pre_k + j;
                if (s < 0) continue;
                const int code = cb[s];
                if (code < 0 || code >= k) continue;
                const float* row = w + ((size_t)j * k + code) * R + c0 + cq;
                if (vec) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(row);
                    acc[0] += v[0]; acc[1] += v[1]; acc[2] += v[2]; acc[3] += v[3];
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (c0 + cq + q < R) acc[q] += row[q];
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) tile[cq + q][tt] = acc[q];
    }
    if (labels && blockIdx.y == 0)
        for (int tt = tid; tt < PT; tt += 256)
            if (t0 + tt < T) labels[(size_t)b * T + t0 + tt] = cb[t0 + tt];
    __syncthreads();
    // store: 16 threads per channel row, 4 consecutive time steps each
    const int tq = (tid & 15) * 4;
    for (int cc = tid >> 4; cc < PC; cc += 16) {
        const int c = c0 + cc;
        if (c >= R) break;
        float* dst = net0 + ((size_t)b * R + c) * T + t0 + tq;
        if (T % 4 == 0) {
            if (t0 + tq < T) {
                f32x4 v;
                v[0] = tile[cc][tq]; v[1] = tile[cc][tq + 1]; v[2] = tile[cc][tq + 2]; v[3] = tile[cc][tq + 3];
                *reinterpret_cast<f32x4*>(dst) = v;
            }
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (t0 + tq + q < T) dst[q] = tile[cc][tq + q];
        }
    }
}

// grid (k, pre_k); 256 threads, channel r = tid, tid + 256, ...  order: positions b*T + s sorted by code (stable);
// starts[q] .. starts[q+1]: the positions of code q
__global__ __launch_bounds__(256) void prior_input_wgrad_kernel(const int32_t* __restrict__ order, const int32_t* __restrict__ starts,
                                                                const float* __restrict__ dnet_t, float* __restrict__ dw, int T, int k,
                                                                int R, int pre_k) {
    const int q = blockIdx.x, j = blockIdx.y;
    const int shift = pre_k - j;            // code at s feeds net0 at t = s + pre_k - j through tap j
    const int i0 = starts[q], i1 = starts[q + 1];
    for (int r = threadIdx.x; r < R; r += 256) {
        float acc = 0.0f;
        int i = i0;
        // eight rows in flight, added in list order
        for (; i + 8 <= i1; i += 8) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int pos = order[i + u], s = pos % T, t = s + shift;
                v[u] = (t < T) ? dnet_t[((size_t)(pos - s) + t) * R + r] : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) acc += v[u];
        }
        for (; i < i1; ++i) {
            const int pos = order[i], s = pos % T, t = s + shift;
            if (t < T) acc += dnet_t[((size_t)(pos - s) + t) * R + r];
        }
        dw[((size_t)j * k + q) * R + r] = acc;
    }
}

}  // namespace

extern "C" int vqw_prior_input_fwd(const int32_t* codes, const float* w_pre, const float* b_pre, float* net0, int32_t* labels,
                                   int B, int T, int k, int R, int pre_k, vqw_stream_t s) {
    VQW_CHECK(codes && w_pre && b_pre && net0, "vqw_prior_input_fwd: null pointer");
    VQW_CHECK(B > 0 && T > 0 && k > 0 && R > 0 && pre_k >= 1, "vqw_prior_input_fwd: bad shape B=%d T=%d k=%d R=%d pre_k=%d", B, T, k, R, pre_k);
    VQW_CHECK(B <= 65535, "vqw_prior_input_fwd: B=%d exceeds the grid", B);
    VQW_CHECK(((uintptr_t)w_pre % 16 == 0) && ((uintptr_t)net0 % 16 == 0), "vqw_prior_input_fwd: w_pre and net0 must be 16-byte aligned");
    dim3 grid(vqw_cdiv(T, PT), vqw_cdiv(R, PC), B);
    hipLaunchKernelGGL(prior_input_fwd_kernel, grid, dim3(256), 0, (hipStream_t)s, codes, w_pre, b_pre, net0, labels, T, k, R, pre_k);
    VQW_LAUNCH_CHECK("vqw_prior_input_fwd");
    return 0;
}

extern "C" int vqw_prior_input_wgrad(const int32_t* order, const int32_t* starts, const float* dnet_t, float* dw_pre, int B, int T,
                                     int k, int R, int pre_k, vqw_stream_t s) {
    VQW_CHECK(order && starts && dnet_t && dw_pre, "vqw_prior_input_wgrad: null pointer");
    VQW_CHECK(B > 0 && T > 0 && k > 0 && R > 0 && pre_k >= 1 && pre_k <= 65535, "vqw_prior_input_wgrad: bad shape");
    VQW_CHECK((long long)B * T < (1ll << 31), "vqw_prior_input_wgrad: B*T must fit 31 bits");
    hipLaunchKernelGGL(prior_input_wgrad_kernel, dim3(k, pre_k), dim3(256), 0, (hipStream_t)s, order, starts, dnet_t, dw_pre, T, k, R,
                       pre_k);
    VQW_LAUNCH_CHECK("vqw_prior_input_wgrad");
    return 0;
}
