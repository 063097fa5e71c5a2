// Held-out scoring for gfx950: per-position / per-row negative log-likelihood, entropy and greedy hits from logits
// (no gradients, no floating-point atomics), and the VQ code histogram.  Both are HBM-bound, straight-line kernels.
#include "vqw_common.h"

namespace {

// ----------------------------------------------------------------------------- softmax score
// Block = NW waves x 64 consecutive time steps of ONE batch row; wave w owns channels [w*Q/NW, (w+1)*Q/NW): every load is a
// 256-byte row segment, sixteen independent loads in flight per lane (the access pattern of softmax_xent_kernel).  One pass
// over the logits: per lane the online triple (m, s, u) with
//     s = sum_q exp(z_q - m),   u = sum_q exp(z_q - m) (z_q - m)      =>  lse = m + log s,  entropy = log s - u / s
// plus the label's logit and the lowest index among the maxima.  Wave 0 merges the NW partial states in ascending wave order,
// writes the per-position outputs and ONE partial (nll, entropy, count, hits) per (row, tile) from a fixed xor-shuffle tree;
// score_rows_kernel then adds a row's tiles in a fixed order in double precision.  A row's sums depend on that row's logits
// only and come out with the same bits on every launch.
template <int NW>
__global__ __launch_bounds__(NW * 64) void softmax_score_kernel(const float* __restrict__ logits, const int32_t* __restrict__ labels,
                                                                const int32_t* __restrict__ t_begin, const int32_t* __restrict__ t_end,
                                                                float* __restrict__ nll, float* __restrict__ entropy,
                                                                float* __restrict__ part, int Q, int T) {
    __shared__ float sm[NW][64], ss[NW][64], su[NW][64], sl[NW][64], sv[NW][64];
    __shared__ int si[NW][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int ntile = (T + 63) / 64;
    const int b = blockIdx.x / ntile;
    const int t0 = (blockIdx.x % ntile) * 64;
    const int t = t0 + lane;
    const bool ok = t < T;
    const int tb = t_begin ? max(t_begin[b], 0) : 0;
    const int te = t_end ? min(t_end[b], T) : T;
    float* prt = part + (size_t)blockIdx.x * 4;
    if (max(tb, t0) >= min(te, t0 + 64)) {      // no scored position in this tile (block-uniform): nothing is read
        if (w == 0) {
            if (ok && nll) nll[(size_t)b * T + t] = 0.0f;
            if (ok && entropy) entropy[(size_t)b * T + t] = 0.0f;
            if (lane < 4) prt[lane] = 0.0f;
        }
        return;
    }
    const bool scored = ok && t >= tb && t < te;
    const int qn = Q / NW, q0 = w * qn;
    const float* lp = logits + ((size_t)b * Q + q0) * T + t;
    const int lab = scored ? labels[(size_t)b * T + t] : -1;
    float m = -INFINITY, s = 0.0f, u = 0.0f, xl = 0.0f, bv = -INFINITY;
    int bi = Q;
    if (scored) {
        int q = 0;
        for (; q + 16 <= qn; q += 16) {
            float v[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) v[k] = lp[(size_t)(q + k) * T];
            float cm = v[0];
#pragma unroll
            for (int k = 1; k < 16; ++k) cm = fmaxf(cm, v[k]);
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if (v[k] > bv) { bv = v[k]; bi = q0 + q + k; }      // strict: the lowest index among equals stays
            const float mn = fmaxf(m, cm);
            float cs = 0.0f, cu = 0.0f;
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const float d = v[k] - mn, e = __expf(d);
                cs += e;
                cu += e > 0.0f ? e * d : 0.0f;
                if (q0 + q + k == lab) xl = v[k];
            }
            const float r = __expf(m - mn), dm = s > 0.0f ? m - mn : 0.0f;
            u = r * (u + dm * s) + cu;
            s = r * s + cs;
            m = mn;
        }
        for (; q < qn; ++q) {
            const float v = lp[(size_t)q * T];
            if (v > bv) { bv = v; bi = q0 + q; }
            if (q0 + q == lab) xl = v;
            const float mn = fmaxf(m, v);
            const float d = v - mn, e = __expf(d);
            const float r = __expf(m - mn), dm = s > 0.0f ? m - mn : 0.0f;
            u = r * (u + dm * s) + (e > 0.0f ? e * d : 0.0f);
            s = r * s + e;
            m = mn;
        }
    }
    sm[w][lane] = m; ss[w][lane] = s; su[w][lane] = u; sl[w][lane] = xl; sv[w][lane] = bv; si[w][lane] = bi;
    __syncthreads();
    if (w != 0) return;
    float M = sm[0][lane];
#pragma unroll
    for (int i = 1; i < NW; ++i) M = fmaxf(M, sm[i][lane]);
    float S = 0.0f, U = 0.0f, XL = 0.0f, BV = -INFINITY;
    int BI = Q;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        const float si_ = ss[i][lane];
        if (si_ > 0.0f) {
            const float dm = sm[i][lane] - M, r = __expf(dm);
            S += si_ * r;
            U += r * (su[i][lane] + dm * si_);
        }
        XL += sl[i][lane];                                           // only one is non-zero
        if (sv[i][lane] > BV) { BV = sv[i][lane]; BI = si[i][lane]; }
    }
    float vn = 0.0f, ve = 0.0f;
    int cnt = 0, hit = 0;
    if (scored) {
        const float ls = logf(S);
        vn = (ls + M) - XL;
        ve = ls - U / S;
        cnt = 1;
        hit = BI == lab ? 1 : 0;
    }
    if (ok && nll) nll[(size_t)b * T + t] = vn;
    if (ok && entropy) entropy[(size_t)b * T + t] = ve;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        vn += __shfl_xor(vn, o);
        ve += __shfl_xor(ve, o);
        cnt += __shfl_xor(cnt, o);
        hit += __shfl_xor(hit, o);
    }
    if (lane == 0) {
        prt[0] = vn;
        prt[1] = ve;
        prt[2] = __int_as_float(cnt);
        prt[3] = __int_as_float(hit);
    }
}

// One wave per row: lane i adds tiles i, i + 64, ... in ascending order, then a fixed xor-shuffle tree, all in double.
__global__ __launch_bounds__(64) void score_rows_kernel(const float* __restrict__ part, double* __restrict__ row_sums,
                                                        int32_t* __restrict__ row_counts, int ntile) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const f32x4* p = reinterpret_cast<const f32x4*>(part) + (size_t)b * ntile;
    double a = 0.0, e = 0.0;
    int c = 0, h = 0;
    for (int i = lane; i < ntile; i += 64) {
        const f32x4 v = p[i];
        a += (double)v[0];
        e += (double)v[1];
        c += __float_as_int(v[2]);
        h += __float_as_int(v[3]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o);
        e += __shfl_xor(e, o);
        c += __shfl_xor(c, o);
        h += __shfl_xor(h, o);
    }
    if (lane == 0) {
        row_sums[2 * b] = a;
        row_sums[2 * b + 1] = e;
        row_counts[2 * b] = c;
        row_counts[2 * b + 1] = h;
    }
}

// ----------------------------------------------------------------------------- code histogram
// counts[c] += #{(b, f) : idx[b][f] == c, f < f_end[b]}.  Integer atomics on a per-block LDS copy of the table (K <= 8192),
// flushed with one global atomic per non-empty bin; larger tables take the global atomics directly.  An index outside [0, K)
// raises the flag word and is counted nowhere.
constexpr int HIST_LDS = 8192;

__global__ __launch_bounds__(256) void code_histogram_kernel(const int64_t* __restrict__ idx, const int32_t* __restrict__ f_end,
                                                             int32_t* __restrict__ counts, int32_t* __restrict__ flag, int B, int Tz,
                                                             int K) {
    __shared__ int h[HIST_LDS];
    const bool lds = K <= HIST_LDS;
    if (lds) {
        for (int i = threadIdx.x; i < K; i += 256) h[i] = 0;
        __syncthreads();
    }
    const size_t n = (size_t)B * Tz;
    for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int b = (int)(i / Tz), f = (int)(i - (size_t)b * Tz);
        if (f_end && f >= f_end[b]) continue;
        const int64_t c = idx[i];
        if (c < 0 || c >= K) {
            atomicOr(flag, 1);
            continue;
        }
        if (lds)
            atomicAdd(&h[(int)c], 1);
        else
            atomicAdd(&counts[c], 1);
    }
    if (lds) {
        __syncthreads();
        for (int i = threadIdx.x; i < K; i += 256)
            if (h[i]) atomicAdd(&counts[i], h[i]);
    }
}

}  // namespace

// ============================================================================ C ABI
extern "C" int vqw_softmax_score(const float* logits, const int32_t* labels, const int32_t* t_begin, const int32_t* t_end,
                                 float* nll, float* entropy, double* row_sums, int32_t* row_counts, float* scratch,
                                 int64_t scratch_floats, int B, int Q, int T, vqw_stream_t s) {
    VQW_CHECK(logits && labels && row_sums && row_counts && scratch, "vqw_softmax_score: null pointer");
    VQW_CHECK(B > 0 && T > 0, "vqw_softmax_score: bad shape B=%d T=%d", B, T);
    VQW_CHECK(Q >= 4 && Q % 4 == 0 && Q <= 1024, "vqw_softmax_score: Q=%d must be a multiple of 4 and at most 1024", Q);
    const int ntile = vqw_cdiv(T, 64);
    VQW_CHECK((int64_t)B * ntile < (int64_t)1 << 31, "vqw_softmax_score: B * ceil(T / 64) must be below 2^31");
    VQW_CHECK(scratch_floats >= (int64_t)4 * B * ntile, "vqw_softmax_score: scratch needs 4 * B * ceil(T / 64) = %lld floats (got %lld)",
              (long long)4 * B * ntile, (long long)scratch_floats);
    VQW_CHECK((reinterpret_cast<uintptr_t>(scratch) & 15u) == 0 && (reinterpret_cast<uintptr_t>(row_sums) & 7u) == 0,
              "vqw_softmax_score: scratch must be 16-byte and row_sums 8-byte aligned");
    // eight waves per tile where every wave still has whole chunks of 16 channels: twice the loads in flight per position
    if (Q % 128 == 0)
        hipLaunchKernelGGL(softmax_score_kernel<8>, dim3(B * ntile), dim3(512), 0, (hipStream_t)s, logits, labels, t_begin, t_end, nll,
                           entropy, scratch, Q, T);
    else
        hipLaunchKernelGGL(softmax_score_kernel<4>, dim3(B * ntile), dim3(256), 0, (hipStream_t)s, logits, labels, t_begin, t_end, nll,
                           entropy, scratch, Q, T);
    VQW_LAUNCH_CHECK("vqw_softmax_score");
    hipLaunchKernelGGL(score_rows_kernel, dim3(B), dim3(64), 0, (hipStream_t)s, scratch, row_sums, row_counts, ntile);
    VQW_LAUNCH_CHECK("vqw_softmax_score (row sums)");
    return 0;
}

extern "C" int vqw_code_histogram(const int64_t* idx, const int32_t* f_end, int32_t* counts, int32_t* flag, int B, int Tz, int K,
                                  vqw_stream_t s) {
    VQW_CHECK(idx && counts && flag, "vqw_code_histogram: null pointer");
    VQW_CHECK(B > 0 && Tz > 0 && K > 0, "vqw_code_histogram: bad shape B=%d Tz=%d K=%d", B, Tz, K);
    const size_t n = (size_t)B * Tz;
    size_t grid = (n + 1023) / 1024;       // ~4 indices per thread: few blocks, few table flushes
    if (grid > 64) grid = 64;
    hipLaunchKernelGGL(code_histogram_kernel, dim3((int)grid), dim3(256), 0, (hipStream_t)s, idx, f_end, counts, flag, B, Tz, K);
    VQW_LAUNCH_CHECK("vqw_code_histogram");
    return 0;
}
