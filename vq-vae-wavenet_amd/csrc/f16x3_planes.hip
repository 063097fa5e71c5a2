// The fp16x3 engine (f16x3.h): the kernels that write operand planes from fp32 tensors, and the range-guard scales.
//
// Operand planes ("chunk-major"): P[plane 0..1][channel chunk of 8][row][8 fp16]; a row is an output channel
// (weights) or a (batch, time) position (activations).  The 16-byte entries of 32 consecutive rows are contiguous:
// one 64-lane x 16-byte load fetches a 32-row x 16-k MFMA operand fragment in the lane order of the MFMA, and the
// dilation shift of a tap is a row offset (rows before the start of a batch row read as zero through the buffer
// range check: the causal left padding of conv1d_v2, wavenet_ops.py:81).
#include "f16x3.h"

namespace {

// x [B][C][T] fp32 -> planes [2][C/8][B*T][8] fp16 of scale * scale_dev[0] * x
// s2d (the input of a stride-2 conv; T even): planes [2][2 C/8][B*T/2][8], sample t = 2 t' + r of channel c in chunk block r
// (chunks r C/8 ..), row b T/2 + t' -- the strided conv then reads whole consecutive rows per tap (LoopGeom, TAB)
template <bool BF>
__global__ void split_act_kernel(const float* __restrict__ x, uint4* __restrict__ planes, int B, int C, int T, float scale, int kc0, int KC,
                                 const float* __restrict__ scale_dev, unsigned* amax, int* flag, int s2d) {
    const size_t NB = (size_t)B * T;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < NB * (C / 8);
    const float sc = scale * dev_scale(scale_dev);
    float m = 0.0f;
    bool bad = false;
    if (live) {
        const size_t row = i % NB;
        const int kc = (int)(i / NB);
        const int b = (int)(row / T), t = (int)(row % T);
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float xv = x[((size_t)b * C + kc * 8 + e) * T + t];
            v[e] = xv * sc;
            bad |= !(fabsf(xv) <= 3.0e38f);
            m = fmaxf(m, fabsf(xv));
        }
        uint4 p0, p1;
        split8<BF>(v, p0, p1);
        if (s2d) {
            const size_t NH = NB / 2, r2 = (size_t)b * (T / 2) + t / 2;
            const int kcs = (t & 1) * (C / 8) + kc;
            planes[(size_t)kcs * NH + r2] = p0;
            if (!BF) planes[((size_t)(C / 4) + kcs) * NH + r2] = p1;
        } else {
            planes[(size_t)(kc0 + kc) * NB + row] = p0;
            if (!BF) planes[((size_t)KC + kc0 + kc) * NB + row] = p1;
        }
    }
    if (!amax && !flag) return;
    // one atomic per block (see guard_report: same-address atomics of tens of thousands of waves serialise)
    __shared__ float smax[4];
    __shared__ int sbad[4];
    const float wm = wave_max(m);
    const bool wbad = __any(bad || !(m * sc <= F16_MAX));
    if ((threadIdx.x & 63) == 0) { smax[threadIdx.x >> 6] = wm; sbad[threadIdx.x >> 6] = wbad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned bits = __float_as_uint(fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3])));
        if (amax && bits > __hip_atomic_load(amax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(amax, bits);
        if (flag && (sbad[0] | sbad[1] | sbad[2] | sbad[3])) atomicOr(flag, 1);
    }
}

// max |x| over `count` strided matrices [rows][cols] (row stride ld, matrix stride mstride) -> amax[blockIdx.y]
__global__ void amax_kernel(const float* __restrict__ x, long rows, int cols, long ld, long mstride, unsigned* amax, int* flag) {
    const float* xb = x + (size_t)blockIdx.y * mstride;
    const size_t n = (size_t)rows * cols;
    float m = 0.0f;
    bool bad = false;
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (size_t)gridDim.x * blockDim.x;
    if (ld == cols && (n & 3) == 0 && (reinterpret_cast<uintptr_t>(xb) & 15u) == 0) {      // contiguous: 16 bytes per lane, four requests in flight
        const f32x4* x4 = reinterpret_cast<const f32x4*>(xb);
        const size_t n4 = n >> 2;
        auto fold = [&](const f32x4 v) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float a = fabsf(v[e]);
                bad |= !(a <= 3.0e38f);
                m = fmaxf(m, a);
            }
        };
        size_t i = tid;
        for (; i + 7 * nthr < n4; i += 8 * nthr) {
            f32x4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = __builtin_nontemporal_load(x4 + i + u * nthr);
#pragma unroll
            for (int u = 0; u < 8; ++u) fold(v[u]);
        }
        for (; i < n4; i += nthr) fold(__builtin_nontemporal_load(x4 + i));
    } else {
        for (size_t i = tid; i < n; i += nthr) {
            const float v = xb[(i / cols) * ld + (i % cols)];
            bad |= !(fabsf(v) <= 3.0e38f);
            m = fmaxf(m, fabsf(v));
        }
    }
    // one atomic per BLOCK (thousands of waves hitting one address serialise in L2: 8 k wave-level atomics cost ~70 us)
    __shared__ float smax[4];
    __shared__ int sbad[4];
    const float wm = wave_max(m);
    const bool wbad = __any(bad);
    if ((threadIdx.x & 63) == 0) { smax[threadIdx.x >> 6] = wm; sbad[threadIdx.x >> 6] = wbad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned bits = __float_as_uint(fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3])));
        unsigned* dst = amax + blockIdx.y;
        if (bits > __hip_atomic_load(dst, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(dst, bits);
        if (flag && (sbad[0] | sbad[1] | sbad[2] | sbad[3])) atomicOr(flag, 1);
    }
}

// scale[i] = 2^(target_exp - 1 - floor(log2(amax[i]))): amax * scale in [2^(target_exp-1), 2^target_exp); a slot that saw
// nothing (amax == 0) keeps its scale; reset: amax[i] = 0 afterwards (the next step collects afresh)
__global__ void update_scales_kernel(unsigned* amax, float* scale, int n, int target_exp, int reset, int* flag, const int* skip) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || (skip && *skip)) return;      // (skip: a voided step of the deferred guard leaves scales and max-abs slots alone)
    const unsigned b = amax[i];
    if (b >= 0x7f800000u) {                  // inf / NaN was seen
        if (flag) atomicOr(flag, 1);
    } else if (b != 0) {
        int e = (int)(b >> 23) - 127;        // floor(log2(amax)); denormals: -127
        int se = target_exp - 1 - e;
        se = se > 100 ? 100 : (se < -100 ? -100 : se);
        scale[i] = __uint_as_float((unsigned)(se + 127) << 23);
    } else if (scale[i] == 0.0f) {
        scale[i] = 1.0f;
    }
    if (reset) amax[i] = 0;
}

// w [ks][R][ldw] (kernel[k, Cin, Cout], filter columns 0..R-1, gate columns R..2R-1) -> planes [2][ks*R/8][2R][8],
// rows in block order: row m' = 256 mt + i is filter channel 128 mt + i (i < 128) or gate channel 128 mt + i - 128
template <bool BF>
__global__ void pack_gate_w_kernel(const float* __restrict__ w, uint4* __restrict__ planes, int ks, int R, int ldw, float scale,
                                   const float* __restrict__ scale_dev, int hb) {     // hb: rows of a block (256 or 128)
    scale *= dev_scale(scale_dev);
    const int M = 2 * R, KC = ks * R / 8;
    w += (size_t)blockIdx.y * ks * R * ldw;          // one layer per grid row
    planes += (size_t)blockIdx.y * 2 * KC * M;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= KC * M) return;
    const int mp = i % M, kc = i / M;
    const int mt = mp / hb, ii = mp % hb, hh = hb / 2;          // a block holds hh filter rows, then the hh matching gate rows
    const int col = ii < hh ? hh * mt + ii : R + hh * mt + (ii - hh);
    const int j = kc / (R / 8), c0 = (kc % (R / 8)) * 8;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = w[((size_t)j * R + c0 + e) * ldw + col] * scale;
    uint4 p0, p1;
    split8<BF>(v, p0, p1);
    planes[(size_t)kc * M + mp] = p0;
    if (!BF) planes[((size_t)KC + kc) * M + mp] = p1;
}

// w [K][ldw] fp32 (columns = output rows m) -> planes [2][K/8][M][8], natural row order
template <bool BF>
__global__ void pack_w_kernel(const float* __restrict__ w, uint4* __restrict__ planes, int K, int M, int ldw, float scale,
                              const float* __restrict__ scale_dev) {
    scale *= dev_scale(scale_dev);
    const int KC = K / 8;
    w += (size_t)blockIdx.y * K * ldw;
    planes += (size_t)blockIdx.y * 2 * KC * M;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= KC * M) return;
    const int m = i % M, kc = i / M;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = w[(size_t)(kc * 8 + e) * ldw + m] * scale;
    uint4 p0, p1;
    split8<BF>(v, p0, p1);
    planes[(size_t)kc * M + m] = p0;
    if (!BF) planes[((size_t)KC + kc) * M + m] = p1;
}

// The same planes from the TRANSPOSED storage: logical row k = jb * Kin + ko, column m is src[jb * blk_stride + m * ld_src + ko]
// (blocks of Kin rows: the taps of a conv kernel [tap][m][Kin], transposed tap by tap) -- the kernels of the input-gradient GEMMs
// straight from the parameters, without a transposed fp32 copy in between.  A thread reads its 8 rows as 32 contiguous bytes.
template <bool BF>
__global__ void pack_w_t_kernel(const float* __restrict__ w, uint4* __restrict__ planes, int K, int M, int Kin, int ld_src, long blk_stride,
                                float scale, const float* __restrict__ scale_dev) {
    scale *= dev_scale(scale_dev);
    const int KC = K / 8;
    w += (size_t)blockIdx.y * (K / Kin) * blk_stride;
    planes += (size_t)blockIdx.y * 2 * KC * M;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= KC * M) return;
    const int m = i % M, kc = i / M, k0 = kc * 8, jb = k0 / Kin, ko = k0 - jb * Kin;
    const float* src = w + (size_t)jb * blk_stride + (size_t)m * ld_src + ko;
    const f32x4 a = *reinterpret_cast<const f32x4*>(src), b = *reinterpret_cast<const f32x4*>(src + 4);
    float v[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) { v[e] = a[e] * scale; v[4 + e] = b[e] * scale; }
    uint4 p0, p1;
    split8<BF>(v, p0, p1);
    planes[(size_t)kc * M + m] = p0;
    if (!BF) planes[((size_t)KC + kc) * M + m] = p1;
}

// ... through LDS, for blocks of k that are multiples of 64: a tile of 64 columns m x 64 rows k is READ with k fastest (eight
// threads = 256 contiguous bytes of a source row) and WRITTEN with m fastest (64 threads = 1 KiB of a plane), the 16-byte plane
// entries change hands in LDS.  The direct kernel reads 32-byte pieces 1-3 KB apart: 17.3 us per launch on the step's seven packs
// against 10.9 us (tools/pmc_step.sh).
template <bool BF>
__global__ __launch_bounds__(256) void pack_w_t_tile_kernel(const float* __restrict__ w, uint4* __restrict__ planes, int K, int M, int Kin, int ld_src,
                                                            long blk_stride, float scale, const float* __restrict__ scale_dev) {
    __shared__ uint4 lp[2][8][65];
    scale *= dev_scale(scale_dev);
    const int KC = K / 8, mt = (M + 63) / 64;
    const int m0 = (blockIdx.x % mt) * 64, kc0 = (blockIdx.x / mt) * 8, k0 = kc0 * 8, jb = k0 / Kin, ko0 = k0 - jb * Kin;
    w += (size_t)blockIdx.y * (K / Kin) * blk_stride + (size_t)jb * blk_stride + ko0;
    planes += (size_t)blockIdx.y * 2 * KC * M;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int e = threadIdx.x + 256 * r, mm = e >> 3, kq = e & 7;
        float v[8];
        if (m0 + mm < M) {
            const float* src = w + (size_t)(m0 + mm) * ld_src + kq * 8;
            const f32x4 a = *reinterpret_cast<const f32x4*>(src), b = *reinterpret_cast<const f32x4*>(src + 4);
#pragma unroll
            for (int i = 0; i < 4; ++i) { v[i] = a[i] * scale; v[4 + i] = b[i] * scale; }
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = 0.0f;
        }
        uint4 p0, p1;
        split8<BF>(v, p0, p1);
        lp[0][kq][mm] = p0;
        if (!BF) lp[1][kq][mm] = p1;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int e = threadIdx.x + 256 * r, kq = e >> 6, mm = e & 63;
        if (m0 + mm >= M) continue;
        planes[(size_t)(kc0 + kq) * M + m0 + mm] = lp[0][kq][mm];
        if (!BF) planes[((size_t)KC + kc0 + kq) * M + m0 + mm] = lp[1][kq][mm];
    }
}

}  // namespace

extern "C" {

int vqw_f16x3_amax(const float* x, int64_t rows, int cols, int64_t ld, int64_t mstride, int count, uint32_t* amax, int32_t* flag, vqw_stream_t s_) {
    VQW_CHECK(x && amax, "vqw_f16x3_amax: null pointer");
    VQW_CHECK(rows > 0 && cols > 0 && ld >= cols && count >= 1 && count <= 65535, "vqw_f16x3_amax: bad shape (rows=%lld cols=%d ld=%lld count=%d)", (long long)rows, cols, (long long)ld, count);
    const size_t n = (size_t)rows * cols;
    unsigned g = (unsigned)((n + 256 * 32 - 1) / (256 * 32));
    if (g > 512) g = 512;
    hipLaunchKernelGGL(amax_kernel, dim3(g, count), dim3(256), 0, (hipStream_t)s_, x, (long)rows, cols, (long)ld, (long)mstride, amax, flag);
    VQW_LAUNCH_CHECK("vqw_f16x3_amax");
    return 0;
}

int vqw_f16x3_update_scales_guarded(uint32_t* amax, float* scale, int n, int target_exp, int reset, int32_t* flag, const int32_t* skip,
                                    vqw_stream_t s_) {
    VQW_CHECK(amax && scale && n > 0, "vqw_f16x3_update_scales: null pointer");
    VQW_CHECK(target_exp >= 1 && target_exp <= 15, "vqw_f16x3_update_scales: target_exp must be in 1..15 (fp16 holds |x| < 2^16)");
    hipLaunchKernelGGL(update_scales_kernel, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)s_, amax, scale, n, target_exp, reset, flag, skip);
    VQW_LAUNCH_CHECK("vqw_f16x3_update_scales");
    return 0;
}

int vqw_f16x3_update_scales(uint32_t* amax, float* scale, int n, int target_exp, int reset, int32_t* flag, vqw_stream_t s_) {
    return vqw_f16x3_update_scales_guarded(amax, scale, n, target_exp, reset, flag, nullptr, s_);
}

int vqw_f16x3_split_activations(const float* x, void* planes, int B, int C, int T, float scale, int kc0, int KC,
                                const float* scale_dev, uint32_t* amax, int32_t* flag, int mode, vqw_stream_t s_) {
    hipStream_t st = (hipStream_t)s_;
    VQW_CHECK(x && planes, "vqw_f16x3_split_activations: null pointer");
    VQW_CHECK(B > 0 && T > 0 && C > 0 && C % 8 == 0, "vqw_f16x3_split_activations: C must be a positive multiple of 8 (got %d)", C);
    if (KC <= 0) { KC = C / 8; kc0 = 0; }
    VQW_CHECK(kc0 >= 0 && kc0 + C / 8 <= KC, "vqw_f16x3_split_activations: bad chunk range (kc0=%d KC=%d)", kc0, KC);
    const size_t n = (size_t)B * T * (C / 8);
    VQW_CHECK(mode >= 0 && mode <= 7, "vqw_f16x3_split_activations: mode is a bit set of VQW_X3_BF16 | VQW_X3_HALF_BLOCKS | VQW_X3_S2D");
    const int s2d = (mode & VQW_X3_S2D) ? 1 : 0;
    VQW_CHECK(!s2d || (T % 2 == 0 && kc0 == 0 && KC == C / 8), "vqw_f16x3_split_activations: space-to-depth planes need an even T and the whole plane (T=%d kc0=%d)", T, kc0);
    if (mode & 1) hipLaunchKernelGGL(split_act_kernel<true>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, (uint4*)planes, B, C, T, scale, kc0, KC,
                                 scale_dev, amax, flag, s2d);
    else hipLaunchKernelGGL(split_act_kernel<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, (uint4*)planes, B, C, T, scale, kc0, KC,
                            scale_dev, amax, flag, s2d);
    VQW_LAUNCH_CHECK("vqw_f16x3_split_activations");
    return 0;
}

int vqw_f16x3_pack_gate_weights(const float* w, void* planes, int ks, int R, int ldw, float scale, int count, const float* scale_dev, int mode, vqw_stream_t s_) {
    hipStream_t st = (hipStream_t)s_;
    VQW_CHECK(w && planes, "vqw_f16x3_pack_gate_weights: null pointer");
    VQW_CHECK(ks >= 1 && R > 0 && R % 128 == 0 && ldw >= 2 * R && count >= 1 && count <= 65535, "vqw_f16x3_pack_gate_weights: needs R %% 128 == 0, ldw >= 2R, 1 <= count <= 65535 (R=%d ldw=%d count=%d)", R, ldw, count);
    const int n = (ks * R / 8) * 2 * R;
    const int hb = (mode & VQW_X3_HALF_BLOCKS) ? 128 : 256;      // must match the block height of the gate conv that reads the planes
    if (mode & 1) hipLaunchKernelGGL(pack_gate_w_kernel<true>, dim3((n + 255) / 256, count), dim3(256), 0, st, w, (uint4*)planes, ks, R, ldw, scale, scale_dev, hb);
    else hipLaunchKernelGGL(pack_gate_w_kernel<false>, dim3((n + 255) / 256, count), dim3(256), 0, st, w, (uint4*)planes, ks, R, ldw, scale, scale_dev, hb);
    VQW_LAUNCH_CHECK("vqw_f16x3_pack_gate_weights");
    return 0;
}

int vqw_f16x3_pack_weights(const float* w, void* planes, int K, int M, int ldw, float scale, int count, const float* scale_dev, int mode, vqw_stream_t s_) {
    hipStream_t st = (hipStream_t)s_;
    VQW_CHECK(w && planes, "vqw_f16x3_pack_weights: null pointer");
    VQW_CHECK(K > 0 && K % 8 == 0 && M > 0 && ldw >= M && count >= 1 && count <= 65535, "vqw_f16x3_pack_weights: needs K %% 8 == 0, ldw >= M, 1 <= count <= 65535 (K=%d M=%d ldw=%d count=%d)", K, M, ldw, count);
    const int n = (K / 8) * M;
    if (mode & 1) hipLaunchKernelGGL(pack_w_kernel<true>, dim3((n + 255) / 256, count), dim3(256), 0, st, w, (uint4*)planes, K, M, ldw, scale, scale_dev);
    else hipLaunchKernelGGL(pack_w_kernel<false>, dim3((n + 255) / 256, count), dim3(256), 0, st, w, (uint4*)planes, K, M, ldw, scale, scale_dev);
    VQW_LAUNCH_CHECK("vqw_f16x3_pack_weights");
    return 0;
}

int vqw_f16x3_pack_weights_t(const float* w, void* planes, int K, int M, int k_inner, int ld_src, int64_t blk_stride, float scale, int count,
                             const float* scale_dev, int mode, vqw_stream_t s_) {
    hipStream_t st = (hipStream_t)s_;
    VQW_CHECK(w && planes, "vqw_f16x3_pack_weights_t: null pointer");
    VQW_CHECK(K > 0 && M > 0 && k_inner > 0 && k_inner % 8 == 0 && K % k_inner == 0 && ld_src >= k_inner && ld_src % 4 == 0 && blk_stride % 4 == 0 &&
              blk_stride >= 0 && count >= 1 && count <= 65535 && (reinterpret_cast<uintptr_t>(w) & 15) == 0,
              "vqw_f16x3_pack_weights_t: needs k_inner %% 8 == 0, K %% k_inner == 0, ld_src >= k_inner, 16-byte aligned rows (K=%d M=%d k_inner=%d ld_src=%d)",
              K, M, k_inner, ld_src);
    const int n = (K / 8) * M;
    if (k_inner % 64 == 0) {        // whole 64-row tiles inside every block of k: the LDS-transposing kernel
        const dim3 grid(((M + 63) / 64) * (K / 64), count);
        if (mode & 1) hipLaunchKernelGGL(pack_w_t_tile_kernel<true>, grid, dim3(256), 0, st, w, (uint4*)planes, K, M, k_inner, ld_src, (long)blk_stride, scale, scale_dev);
        else hipLaunchKernelGGL(pack_w_t_tile_kernel<false>, grid, dim3(256), 0, st, w, (uint4*)planes, K, M, k_inner, ld_src, (long)blk_stride, scale, scale_dev);
    } else if (mode & 1) hipLaunchKernelGGL(pack_w_t_kernel<true>, dim3((n + 255) / 256, count), dim3(256), 0, st, w, (uint4*)planes, K, M, k_inner, ld_src, (long)blk_stride, scale, scale_dev);
    else hipLaunchKernelGGL(pack_w_t_kernel<false>, dim3((n + 255) / 256, count), dim3(256), 0, st, w, (uint4*)planes, K, M, k_inner, ld_src, (long)blk_stride, scale, scale_dev);
    VQW_LAUNCH_CHECK("vqw_f16x3_pack_weights_t");
    return 0;
}

}  // extern "C"
