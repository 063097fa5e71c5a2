// The 2019 decoder's conditioning conv over the latents for gfx950 (arXiv 1901.08810; the reference names it in
// Decoder/decoder.py:22-28 and builds it in Decoder/decoder_ops.py:31-32: Conv1D(filters=C, kernel_size=k, padding='same')
// between the VQ and the speaker concat).  With pl = (k - 1) / 2, zero padding per utterance, rows independent:
//   fwd:    out[b][o][t] = bias[o] + sum_{j<k} sum_{d<D} w[j][d][o] z[b][d][t + j - pl]
//   dgrad:  dz[b][d][s]  = sum_{j<k} sum_{o<C} w[j][d][o] dout[b][o][s - j + pl]
//   wgrad:  dw[j][d][o] += sum_{b,t} z[b][d][t + j - pl] dout[b][o][t];   db[o] += sum_{b,t} dout[b][o][t]
// Contractions of k D (192), k C (384) and B Tz (832) terms on tensors of a few hundred KB: 20 / 20 / 41 MFLOP at the
// benchmark's latent shape, less than one wave's worth of MFMA work per CU, so the kernels are plain fp32 fmaf chains whose
// order the header states -- one thread per output element (fwd: four output channels, which share every z load), time on
// the lanes so that activations load and store coalesced and a wave's weight reads are one address.  Only the weight
// gradient contracts over (batch, time): its blocks stage 64-frame chunks of z and dout in LDS, every thread owns one
// (d, o) pair for all k taps, and the chunks are split over up to 16 blocks per tile whose partial sums go through scratch
// and are added in split order by a second kernel (no atomics; dw and db are added to once per element).
#include "vqw_common.h"

namespace {

constexpr int CC_MAXK = 7;                       // taps
constexpr int CC_LANES = 64, CC_ROWS = 4;        // fwd / dgrad block: 64 frames x 4 rows (fwd: rows of four output channels)
constexpr int CC_DT = 16, CC_OT = 16, CC_TT = 64;  // wgrad block: 16 d x 16 o, chunks of 64 frames
constexpr int CC_ZW = CC_TT + CC_MAXK;           // LDS row of z: 64 + k - 1 <= 70 frames used; 71: odd, rows land on different banks
constexpr int CC_QW = CC_TT + 1;
constexpr int CC_SPLITS = 16;                    // partial sums of dw / db per element, at most

__global__ __launch_bounds__(CC_LANES * CC_ROWS) void cond_conv_fwd_kernel(
    const float* __restrict__ z, long z_bs, const float* __restrict__ w, const float* __restrict__ bias, float* __restrict__ out,
    long out_bs, int B, int D, int C, int Tz, int k) {
    const int t = blockIdx.x * CC_LANES + threadIdx.x, o0 = (blockIdx.y * CC_ROWS + threadIdx.y) * 4;
    if (t >= Tz || o0 >= C) return;
    const int pl = (k - 1) >> 1;
    for (int b = blockIdx.z; b < B; b += gridDim.z) {
        const float* zb = z + (size_t)b * z_bs;
        float a0 = bias[o0], a1 = bias[o0 + 1], a2 = bias[o0 + 2], a3 = bias[o0 + 3];
        for (int j = 0; j < k; ++j) {
            const int tt = t + j - pl;
            if (tt < 0 || tt >= Tz) continue;      // (padding: the frame reads 0, its terms are left out)
            const float* wj = w + (size_t)j * D * C + o0;
            for (int d = 0; d < D; ++d) {
                const float zv = zb[(size_t)d * Tz + tt];
                const float* wr = wj + (size_t)d * C;
                a0 = fmaf(wr[0], zv, a0);
                a1 = fmaf(wr[1], zv, a1);
                a2 = fmaf(wr[2], zv, a2);
                a3 = fmaf(wr[3], zv, a3);
            }
        }
        float* ob = out + (size_t)b * out_bs + (size_t)o0 * Tz + t;
        ob[0] = a0;
        ob[(size_t)Tz] = a1;
        ob[(size_t)2 * Tz] = a2;
        ob[(size_t)3 * Tz] = a3;
    }
}

__global__ __launch_bounds__(CC_LANES * CC_ROWS) void cond_conv_dgrad_kernel(
    const float* __restrict__ w, const float* __restrict__ dout, long dout_bs, float* __restrict__ dz, long dz_bs, int B, int D,
    int C, int Tz, int k) {
    const int s = blockIdx.x * CC_LANES + threadIdx.x, d = blockIdx.y * CC_ROWS + threadIdx.y;
    if (s >= Tz || d >= D) return;
    const int pl = (k - 1) >> 1;
    for (int b = blockIdx.z; b < B; b += gridDim.z) {
        const float* gb = dout + (size_t)b * dout_bs;
        float acc = 0.0f;
        for (int j = 0; j < k; ++j) {
            const int tt = s - j + pl;
            if (tt < 0 || tt >= Tz) continue;
            const float* wr = w + ((size_t)j * D + d) * C;
            const float* g = gb + tt;
#pragma unroll 4
            for (int o = 0; o < C; ++o) acc = fmaf(wr[o], g[(size_t)o * Tz], acc);
        }
        dz[(size_t)b * dz_bs + (size_t)d * Tz + s] = acc;
    }
}

// part[split][(j D + d) C + o] and part[split][k D C + o]: the sums over the split's chunks.  grid (C / 16, ceil(D / 16), splits).
__global__ __launch_bounds__(CC_DT * CC_OT) void cond_conv_wgrad_kernel(
    const float* __restrict__ z, long z_bs, const float* __restrict__ dout, long dout_bs, float* __restrict__ part, int B, int D,
    int C, int Tz, int k, int nsplit) {
    __shared__ float zs[CC_DT][CC_ZW];
    __shared__ float qs[CC_OT][CC_QW];
    const int tid = threadIdx.x, ol = tid & (CC_OT - 1), dl = tid / CC_OT;
    const int o0 = blockIdx.x * CC_OT, d0 = blockIdx.y * CC_DT, split = blockIdx.z;
    const int pl = (k - 1) >> 1, W = CC_TT + k - 1;
    const int ntc = (Tz + CC_TT - 1) / CC_TT;
    const long nchunk = (long)B * ntc;
    const long c_lo = split * nchunk / nsplit, c_hi = (split + 1) * nchunk / nsplit;
    float acc[CC_MAXK], accb = 0.0f;
#pragma unroll
    for (int j = 0; j < CC_MAXK; ++j) acc[j] = 0.0f;
    for (long ci = c_lo; ci < c_hi; ++ci) {
        const int b = (int)(ci / ntc), t0 = (int)(ci % ntc) * CC_TT;
        const float* zb = z + (size_t)b * z_bs;
        const float* gb = dout + (size_t)b * dout_bs;
        __syncthreads();                           // (the previous chunk has been read)
        for (int e = tid; e < CC_DT * W; e += CC_DT * CC_OT) {
            const int r = e / W, c = e - r * W, d = d0 + r, tt = t0 - pl + c;
            zs[r][c] = (d < D && tt >= 0 && tt < Tz) ? zb[(size_t)d * Tz + tt] : 0.0f;
        }
        for (int e = tid; e < CC_OT * CC_TT; e += CC_DT * CC_OT) {
            const int r = e / CC_TT, c = e - r * CC_TT, tt = t0 + c;
            qs[r][c] = tt < Tz ? gb[(size_t)(o0 + r) * Tz + tt] : 0.0f;
        }
        __syncthreads();
        for (int tl = 0; tl < CC_TT; ++tl) {
            const float q = qs[ol][tl];
#pragma unroll
            for (int j = 0; j < CC_MAXK; ++j)
                if (j < k) acc[j] = fmaf(zs[dl][tl + j], q, acc[j]);
            accb = __fadd_rn(accb, q);
        }
    }
    float* pb = part + (size_t)split * ((size_t)k * D * C + C);
    const int d = d0 + dl;
    if (d < D) {
#pragma unroll
        for (int j = 0; j < CC_MAXK; ++j)
            if (j < k) pb[((size_t)j * D + d) * C + o0 + ol] = acc[j];
    }
    if (blockIdx.y == 0 && dl == 0) pb[(size_t)k * D * C + o0 + ol] = accb;
}

// dw[i] += sum_s part[s][i], db[o] += sum_s part[s][k D C + o], s ascending from part[0]
__global__ void cond_conv_wgrad_reduce_kernel(const float* __restrict__ part, float* __restrict__ dw, float* __restrict__ db,
                                              int nsplit, size_t ndw, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float s = part[i];
    for (int sp = 1; sp < nsplit; ++sp) s = __fadd_rn(s, part[(size_t)sp * n + i]);
    float* o = i < ndw ? dw + i : db + (i - ndw);
    *o = __fadd_rn(*o, s);
}

int cc_splits(int B, int Tz) {
    const long nchunk = (long)B * ((Tz + CC_TT - 1) / CC_TT);
    return nchunk < CC_SPLITS ? (int)nchunk : CC_SPLITS;
}

int cc_check_shape(const char* name, int B, int D, int C, int Tz, int k) {
    VQW_CHECK(B > 0 && D > 0 && Tz > 0, "%s: B=%d, D=%d, Tz=%d must be positive", name, B, D, Tz);
    VQW_CHECK(C > 0 && C % 16 == 0, "%s: C=%d must be a positive multiple of 16", name, C);
    VQW_CHECK(k >= 1 && k <= CC_MAXK && (k & 1), "%s: k=%d must be odd and in 1..%d", name, k, CC_MAXK);
    VQW_CHECK(Tz <= (1 << 24) && D <= (1 << 16) && C <= (1 << 16), "%s: Tz=%d <= 2^24, D=%d <= 2^16, C=%d <= 2^16", name, Tz, D, C);
    return 0;
}

struct cc_range {
    const char* what;
    uintptr_t lo, hi;
};
cc_range cc_span(const char* what, const void* p, int64_t floats) {
    const uintptr_t lo = reinterpret_cast<uintptr_t>(p);
    return {what, lo, lo + (uintptr_t)floats * 4};
}
int64_t cc_extent(int B, int64_t bs, int rows, int Tz) { return (int64_t)(B - 1) * bs + (int64_t)rows * Tz; }

// every output (the first n_out ranges) apart from every other range
int cc_check_alias(const char* name, const cc_range* r, int n, int n_out) {
    for (int i = 0; i < n_out; ++i)
        for (int j = 0; j < n; ++j)
            VQW_CHECK(j == i || (j < i && j < n_out) || r[i].hi <= r[j].lo || r[j].hi <= r[i].lo, "%s: %s must not overlap %s", name,
                      r[i].what, r[j].what);
    return 0;
}

dim3 cc_grid(int rows, int B, int Tz) { return dim3(vqw_cdiv(Tz, CC_LANES), vqw_cdiv(rows, CC_ROWS), B < 65535 ? B : 65535); }

}  // namespace

extern "C" {

int vqw_cond_conv_fwd(const float* z, int64_t z_bstride, const float* w, const float* bias, float* out, int64_t out_bstride, int B,
                      int D, int C, int Tz, int k, vqw_stream_t s) {
    const char* name = "vqw_cond_conv_fwd";
    VQW_CHECK(z && w && bias && out, "%s: null pointer", name);
    if (cc_check_shape(name, B, D, C, Tz, k)) return 1;
    VQW_CHECK(z_bstride >= (int64_t)D * Tz && out_bstride >= (int64_t)C * Tz, "%s: batch strides %lld, %lld must be >= D*Tz = %lld, C*Tz = %lld",
              name, (long long)z_bstride, (long long)out_bstride, (long long)D * Tz, (long long)C * Tz);
    const cc_range r[4] = {cc_span("out", out, cc_extent(B, out_bstride, C, Tz)), cc_span("z", z, cc_extent(B, z_bstride, D, Tz)),
                           cc_span("w", w, (int64_t)k * D * C), cc_span("bias", bias, C)};
    if (cc_check_alias(name, r, 4, 1)) return 1;
    hipLaunchKernelGGL(cond_conv_fwd_kernel, cc_grid(C / 4, B, Tz), dim3(CC_LANES, CC_ROWS), 0, (hipStream_t)s, z, (long)z_bstride, w, bias,
                       out, (long)out_bstride, B, D, C, Tz, k);
    VQW_LAUNCH_CHECK(name);
    return 0;
}

int vqw_cond_conv_dgrad(const float* w, const float* dout, int64_t dout_bstride, float* dz, int64_t dz_bstride, int B, int D, int C,
                        int Tz, int k, vqw_stream_t s) {
    const char* name = "vqw_cond_conv_dgrad";
    VQW_CHECK(w && dout && dz, "%s: null pointer", name);
    if (cc_check_shape(name, B, D, C, Tz, k)) return 1;
    VQW_CHECK(dz_bstride >= (int64_t)D * Tz && dout_bstride >= (int64_t)C * Tz, "%s: batch strides %lld, %lld must be >= D*Tz = %lld, C*Tz = %lld",
              name, (long long)dz_bstride, (long long)dout_bstride, (long long)D * Tz, (long long)C * Tz);
    const cc_range r[3] = {cc_span("dz", dz, cc_extent(B, dz_bstride, D, Tz)), cc_span("dout", dout, cc_extent(B, dout_bstride, C, Tz)),
                           cc_span("w", w, (int64_t)k * D * C)};
    if (cc_check_alias(name, r, 3, 1)) return 1;
    hipLaunchKernelGGL(cond_conv_dgrad_kernel, cc_grid(D, B, Tz), dim3(CC_LANES, CC_ROWS), 0, (hipStream_t)s, w, dout, (long)dout_bstride, dz,
                       (long)dz_bstride, B, D, C, Tz, k);
    VQW_LAUNCH_CHECK(name);
    return 0;
}

int vqw_cond_conv_wgrad(const float* z, int64_t z_bstride, const float* dout, int64_t dout_bstride, float* dw, float* db, float* scratch,
                        int64_t scratch_floats, int B, int D, int C, int Tz, int k, vqw_stream_t s) {
    const char* name = "vqw_cond_conv_wgrad";
    VQW_CHECK(z && dout && dw && db && scratch, "%s: null pointer", name);
    if (cc_check_shape(name, B, D, C, Tz, k)) return 1;
    VQW_CHECK(z_bstride >= (int64_t)D * Tz && dout_bstride >= (int64_t)C * Tz, "%s: batch strides %lld, %lld must be >= D*Tz = %lld, C*Tz = %lld",
              name, (long long)z_bstride, (long long)dout_bstride, (long long)D * Tz, (long long)C * Tz);
    const int nsplit = cc_splits(B, Tz);
    const size_t ndw = (size_t)k * D * C, n = ndw + C;
    VQW_CHECK(scratch_floats >= (int64_t)(nsplit * n), "%s: scratch needs %d * (k*D*C + C) = %zu floats, has %lld", name, nsplit, nsplit * n,
              (long long)scratch_floats);
    VQW_CHECK(vqw_cdiv(D, CC_DT) <= 65535, "%s: D=%d too large", name, D);
    const cc_range r[5] = {cc_span("dw", dw, (int64_t)ndw), cc_span("db", db, C), cc_span("scratch", scratch, (int64_t)(nsplit * n)),
                           cc_span("z", z, cc_extent(B, z_bstride, D, Tz)), cc_span("dout", dout, cc_extent(B, dout_bstride, C, Tz))};
    if (cc_check_alias(name, r, 5, 3)) return 1;
    hipLaunchKernelGGL(cond_conv_wgrad_kernel, dim3(C / CC_OT, vqw_cdiv(D, CC_DT), nsplit), dim3(CC_DT * CC_OT), 0, (hipStream_t)s, z,
                       (long)z_bstride, dout, (long)dout_bstride, scratch, B, D, C, Tz, k, nsplit);
    hipLaunchKernelGGL(cond_conv_wgrad_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)s, (const float*)scratch, dw,
                       db, nsplit, ndw, n);
    VQW_LAUNCH_CHECK(name);
    return 0;
}

int vqw_cond_conv_wgrad_scratch_floats(int B, int D, int C, int Tz, int k, int64_t* out) {
    const char* name = "vqw_cond_conv_wgrad_scratch_floats";
    VQW_CHECK(out, "%s: null pointer", name);
    if (cc_check_shape(name, B, D, C, Tz, k)) return 1;
    *out = (int64_t)cc_splits(B, Tz) * ((int64_t)k * D * C + C);
    return 0;
}

}  // extern "C"
