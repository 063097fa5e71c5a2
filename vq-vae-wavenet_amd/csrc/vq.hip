// VQ nearest-codebook kernels for gfx950 -- reference model.py:57-74 (forward),
// model.py:73,100,103 (gradients), model.py:22-27 + decoder_ops.py:39-43 (speaker tiling).
//
// Bit-exactness contract: the distance is the DIRECT form
// sum_d (z-e)^2 accumulated for d = 0..D-1 in order, with the subtract, the multiply and the
// add each rounded to fp32 (no FMA contraction: explicit __f*_rn intrinsics), and the argmin
// returns the lowest index among equal minima -- identical to oracle/vqw_oracle.c.
#include "vqw_common.h"

namespace {

// One wave per latent row (b, t).  Lane l scans codes l, l+64, ... in increasing order
// (strict '<' keeps the lowest index inside a lane); the 64 per-lane candidates are then
// merged with wavefront xor-shuffles using (distance, index) lexicographic order.
__global__ __launch_bounds__(256) void vq_nearest_fwd_kernel(
    const float* __restrict__ z_e, const float* __restrict__ emb, int64_t* __restrict__ idx,
    float* __restrict__ e_k, float* __restrict__ zq, long zq_bstride, float* __restrict__ mind,
    int rows, int D, int Tz, int K) {
    extern __shared__ float zs_all[];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int row = blockIdx.x * 4 + wid;
    float* zs = zs_all + wid * D;
    const bool live = row < rows;
    const int b = live ? row / Tz : 0, t = live ? row % Tz : 0;
    const float* zrow = z_e + (size_t)b * D * Tz + t;
    if (live)
        for (int d = lane; d < D; d += 64) zs[d] = zrow[(size_t)d * Tz];
    __syncthreads();
    if (!live) return;

    float best = INFINITY;
    int bi = 0x7fffffff;
    for (int k = lane; k < K; k += 64) {
        const float* e = emb + (size_t)k * D;
        float acc = 0.0f;
        for (int d = 0; d < D; d += 4) {
            const f32x4 ev = *reinterpret_cast<const f32x4*>(e + d);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float diff = __fsub_rn(zs[d + u], ev[u]);
                acc = __fadd_rn(acc, __fmul_rn(diff, diff));
            }
        }
        if (acc < best) { best = acc; bi = k; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o);
        const int oi = __shfl_xor(bi, o);
        if (ob < best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    if (bi == 0x7fffffff) bi = 0;  // all-NaN row: tf.argmin would return 0
    if (lane == 0) {
        idx[row] = bi;
        if (mind) mind[row] = best;
    }
    const float* e = emb + (size_t)bi * D;
    for (int d = lane; d < D; d += 64) {
        const float ek = e[d], z = zs[d];
        if (e_k) e_k[(size_t)b * D * Tz + (size_t)d * Tz + t] = ek;
        if (zq) zq[(size_t)b * zq_bstride + (size_t)d * Tz + t] = __fadd_rn(z, __fsub_rn(ek, z));  // model.py:73
    }
}

__global__ void vq_nearest_bwd_kernel(const float* __restrict__ z_e, const float* __restrict__ e_k,
                                      const int64_t* __restrict__ idx, const float* __restrict__ dzq,
                                      long dzq_bstride, float* __restrict__ dz_e,
                                      float* __restrict__ demb, float cscale, float escale, int B,
                                      int D, int Tz) {
    const size_t n = (size_t)B * D * Tz;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int t = (int)(i % Tz);
        const int d = (int)((i / Tz) % D);
        const int b = (int)(i / ((size_t)Tz * D));
        const float z = z_e[i], e = e_k[i];
        const float g = dzq ? dzq[(size_t)b * dzq_bstride + (size_t)d * Tz + t] : 0.0f;
        if (dz_e) dz_e[i] = g + cscale * (z - e);
        if (demb) unsafeAtomicAdd(demb + (size_t)idx[(size_t)b * Tz + t] * D + d, escale * (e - z));
    }
}

// Codebook gradient through an LDS copy of the whole table: early in training most latents share a few codes
// (measured: 53 k global atomics on ~64 addresses = 308 us), LDS atomics absorb that contention; every block
// owns a slice of the (b, t) rows and flushes only the entries it touched.  dz_e as above.
__global__ __launch_bounds__(256) void vq_nearest_bwd_lds_kernel(const float* __restrict__ z_e, const float* __restrict__ e_k,
                                                                 const int64_t* __restrict__ idx, const float* __restrict__ dzq,
                                                                 long dzq_bstride, float* __restrict__ dz_e, float* __restrict__ demb,
                                                                 float cscale, float escale, int B, int D, int Tz, int K) {
    extern __shared__ float tabl[];   // [K][D]
    const int KD = K * D;
    for (int i = threadIdx.x; i < KD; i += blockDim.x) tabl[i] = 0.0f;
    __syncthreads();
    const size_t n = (size_t)B * D * Tz;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int t = (int)(i % Tz);
        const int d = (int)((i / Tz) % D);
        const int b = (int)(i / ((size_t)Tz * D));
        const float z = z_e[i], e = e_k[i];
        const float g = dzq ? dzq[(size_t)b * dzq_bstride + (size_t)d * Tz + t] : 0.0f;
        if (dz_e) dz_e[i] = g + cscale * (z - e);
        unsafeAtomicAdd(&tabl[(size_t)idx[(size_t)b * Tz + t] * D + d], escale * (e - z));
    }
    __syncthreads();
    for (int i = threadIdx.x; i < KD; i += blockDim.x) {
        const float v = tabl[i];
        if (v != 0.0f) unsafeAtomicAdd(demb + i, v);
    }
}

__global__ void speaker_tile_fwd_kernel(const float* __restrict__ table, const int64_t* __restrict__ spk,
                                        float* __restrict__ cond, long cond_bstride, int row0, int B,
                                        int Cs, int Tz, int n_speakers) {
    const size_t n = (size_t)B * Cs * Tz;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int t = (int)(i % Tz);
        const int j = (int)((i / Tz) % Cs);
        const int b = (int)(i / ((size_t)Tz * Cs));
        // model.py:22: one_hot -> argmax; an id outside the table is an all-zero one-hot row, whose argmax is 0
        const int64_t id = spk[b];
        const size_t row = (id >= 0 && id < n_speakers) ? (size_t)id : 0;
        cond[(size_t)b * cond_bstride + (size_t)(row0 + j) * Tz + t] = table[row * Cs + j];
    }
}

__global__ void speaker_tile_bwd_kernel(const float* __restrict__ dcond, long dcond_bstride, int row0,
                                        const int64_t* __restrict__ spk, float* __restrict__ dtable,
                                        int B, int Cs, int Tz, int n_speakers) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * Cs) return;
    const int b = i / Cs, j = i % Cs;
    const float* r = dcond + (size_t)b * dcond_bstride + (size_t)(row0 + j) * Tz;
    float s = 0.0f;
    for (int t = 0; t < Tz; ++t) s += r[t];
    const int64_t id = spk[b];
    const size_t row = (id >= 0 && id < n_speakers) ? (size_t)id : 0;     // same row the forward pass read
    unsafeAtomicAdd(dtable + row * Cs + j, s);
}

// ---- codebook by moving averages --------------------------------------------------------------------
// Cluster statistics of one pass: one wave per code k.  The wave's 64 lanes load 64 consecutive idx (frames f = b*Tz + t in
// ascending order), a ballot finds the frames of code k, the set bits are walked from the lowest up and the lanes stride
// over d: sum[k][d] is a chain of fp32 adds in ascending f from +0.0f -- a fixed order, nothing atomic, every element of
// cnt / sum / cand written by exactly one lane (zeros for an unused code).  More than 64 channels: the frames are scanned
// once per 64 channels (the running sums stay in one register per lane).  cand[k] = the frame pick[k], clamped to [0, Nf).
constexpr int CB_WAVES = 4;

__global__ __launch_bounds__(64 * CB_WAVES) void vq_cluster_stats_kernel(
    const float* __restrict__ z_e, const int64_t* __restrict__ idx, const int32_t* __restrict__ pick, int32_t* __restrict__ cnt,
    float* __restrict__ sum, float* __restrict__ cand, int Nf, int D, int Tz, int K) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * CB_WAVES + (threadIdx.x >> 6);
    if (k >= K) return;                                   // (whole waves leave; the kernel has no barrier)
    const size_t bstride = (size_t)D * Tz;
    for (int d0 = 0; d0 < D; d0 += 64) {
        const int d = d0 + lane;
        const bool on = d < D;
        const float* zd = z_e + (size_t)(on ? d : 0) * Tz;
        float acc = 0.0f;
        int n = 0;
        for (int f0 = 0; f0 < Nf; f0 += 64) {
            const int f = f0 + lane;
            unsigned long long hit = __ballot(f < Nf && idx[f < Nf ? f : 0] == (int64_t)k);
            n += __popcll(hit);
            while (hit) {
                const int fk = f0 + __builtin_ctzll(hit);
                hit &= hit - 1;
                const int b = fk / Tz, t = fk - b * Tz;
                if (on) acc = acc + zd[(size_t)b * bstride + t];
            }
        }
        if (on) sum[(size_t)k * D + d] = acc;
        if (d0 == 0 && lane == 0) cnt[k] = n;
    }
    if (cand) {
        int p = pick[k];
        p = p < 0 ? 0 : (p >= Nf ? Nf - 1 : p);
        const int b = p / Tz, t = p - b * Tz;
        for (int d = lane; d < D; d += 64) cand[(size_t)k * D + d] = z_e[(size_t)b * bstride + (size_t)d * Tz + t];
    }
}

// The codebook's update, one wave per code (the per-code scalars once per wave, the lanes over d).  Every operation is
// rounded to fp32 on its own.  info[0..1] = codes restarted / codes with cnt > 0 of THIS call: the blocks add their counts
// into info[4..5] (integer atomics) and the last block to finish (ticket info[6]) moves them to info[0..1] and leaves
// info[4..6] at zero for the next call.  *skip != 0: the kernel returns before it reads or writes anything else.
__global__ __launch_bounds__(64 * CB_WAVES) void vq_codebook_ema_kernel(
    float* __restrict__ emb, float* __restrict__ n_, float* __restrict__ m_, const int32_t* __restrict__ cnt,
    const float* __restrict__ sum, const float* __restrict__ cand, float g, float h, float tau, int32_t* __restrict__ info,
    const int32_t* __restrict__ skip, int K, int D) {
    // plain operators under contract(off): each is one IEEE fp32 operation (what __fmul_rn / __fadd_rn / __fdiv_rn name); the
    // intrinsics are inlined WITH the translation unit's contraction and g*m + h*sum came out as v_mul + v_fmac
#pragma clang fp contract(off)
    if (skip && *skip != 0) return;
    __shared__ int tally[2];
    if (threadIdx.x < 2) tally[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * CB_WAVES + (threadIdx.x >> 6);
    if (k < K) {
        const int c = cnt[k];
        const float gn = g * n_[k], hc = h * (float)c;
        const float n1 = gn + hc;
        const bool dead = tau > 0.0f && n1 < tau;
        const size_t row = (size_t)k * D;
        for (int d = lane; d < D; d += 64) {
            const float gm = g * m_[row + d], hs = h * sum[row + d];
            const float m1 = gm + hs;
            if (dead) {
                const float z = cand[row + d];
                m_[row + d] = z;
                emb[row + d] = z;
            } else {
                m_[row + d] = m1;
                if (c > 0) emb[row + d] = m1 / n1;
            }
        }
        if (lane == 0) {          // (every lane has read n_[k] above: one wave, program order)
            n_[k] = dead ? 1.0f : n1;
            if (dead) atomicAdd(&tally[0], 1);
            if (c > 0) atomicAdd(&tally[1], 1);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (tally[0]) atomicAdd(info + 4, tally[0]);
        if (tally[1]) atomicAdd(info + 5, tally[1]);
        __threadfence();
        if (atomicAdd(info + 6, 1) == (int)gridDim.x - 1) {
            __threadfence();
            info[0] = atomicExch(info + 4, 0);
            info[1] = atomicExch(info + 5, 0);
            atomicExch(info + 6, 0);
        }
    }
}

// [a, a + na) and [b, b + nb) bytes share a byte
bool cb_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return a && b && x < y + nb && y < x + na;
}

}  // namespace

extern "C" int vqw_vq_nearest_fwd(const float* z_e, const float* emb, int64_t* idx, float* e_k, float* zq,
                                  int64_t zq_bstride, float* mind, int B, int D, int Tz, int K,
                                  vqw_stream_t s) {
    VQW_CHECK(z_e && emb && idx, "vqw_vq_nearest_fwd: null pointer");
    VQW_CHECK(B > 0 && Tz > 0 && K > 0 && D > 0 && D % 4 == 0, "vqw_vq_nearest_fwd: D=%d must be a positive multiple of 4", D);
    VQW_CHECK((reinterpret_cast<uintptr_t>(emb) & 15u) == 0, "vqw_vq_nearest_fwd: emb must be 16-byte aligned");
    const int rows = B * Tz;
    hipLaunchKernelGGL(vq_nearest_fwd_kernel, dim3(vqw_cdiv(rows, 4)), dim3(256), 4 * D * sizeof(float),
                       (hipStream_t)s, z_e, emb, idx, e_k, zq, (long)zq_bstride, mind, rows, D, Tz, K);
    VQW_LAUNCH_CHECK("vqw_vq_nearest_fwd");
    return 0;
}

extern "C" int vqw_vq_nearest_bwd(const float* z_e, const float* e_k, const int64_t* idx, const float* dzq,
                                  int64_t dzq_bstride, float* dz_e, float* demb, float cscale,
                                  float escale, int B, int D, int Tz, int K, vqw_stream_t s) {
    VQW_CHECK(z_e && e_k && idx && (dz_e || demb), "vqw_vq_nearest_bwd: null pointer");
    const size_t n = (size_t)B * D * Tz;
    const size_t lds = (size_t)K * D * sizeof(float);
    if (demb && K > 0 && lds <= 144 * 1024) {
        // per call: the attribute belongs to the current device's copy of the kernel (no process-wide "done" flag)
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(vq_nearest_bwd_lds_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                144 * 1024) != hipSuccess)
            return vqw_set_error("vqw_vq_nearest_bwd: hipFuncSetAttribute failed");
        int g = (int)((n + 256 * 16 - 1) / (256 * 16));   // ~16 elements per thread: few table flushes
        if (g < 1) g = 1;
        if (g > 64) g = 64;
        hipLaunchKernelGGL(vq_nearest_bwd_lds_kernel, dim3(g), dim3(256), lds, (hipStream_t)s, z_e, e_k, idx, dzq,
                           (long)dzq_bstride, dz_e, demb, cscale, escale, B, D, Tz, K);
        VQW_LAUNCH_CHECK("vqw_vq_nearest_bwd");
        return 0;
    }
    int g = (int)((n + 255) / 256);
    if (g > 2048) g = 2048;
    hipLaunchKernelGGL(vq_nearest_bwd_kernel, dim3(g), dim3(256), 0, (hipStream_t)s, z_e, e_k, idx, dzq,
                       (long)dzq_bstride, dz_e, demb, cscale, escale, B, D, Tz);
    VQW_LAUNCH_CHECK("vqw_vq_nearest_bwd");
    return 0;
}

extern "C" int vqw_vq_cluster_stats(const float* z_e, const int64_t* idx, const int32_t* pick, int32_t* cnt, float* sum,
                                    float* cand, int B, int D, int Tz, int K, vqw_stream_t s) {
    VQW_CHECK(z_e && idx && cnt && sum, "vqw_vq_cluster_stats: null pointer");
    VQW_CHECK((pick == nullptr) == (cand == nullptr), "vqw_vq_cluster_stats: null pointer (pick and cand go together)");
    VQW_CHECK(B > 0 && D > 0 && Tz > 0 && K > 0, "vqw_vq_cluster_stats: B=%d, D=%d, Tz=%d, K=%d must be positive", B, D, Tz, K);
    VQW_CHECK((int64_t)B * Tz <= (1 << 30) && (int64_t)K * D <= (1 << 30), "vqw_vq_cluster_stats: B*Tz and K*D must be <= 2^30");
    const size_t nz = (size_t)B * D * Tz * 4, ni = (size_t)B * Tz * 8, nk = (size_t)K * 4, nkd = (size_t)K * D * 4;
    const void* in[3] = {z_e, idx, pick};
    const size_t in_n[3] = {nz, ni, nk};
    const void* out[3] = {cnt, sum, cand};
    const size_t out_n[3] = {nk, nkd, nkd};
    for (int o = 0; o < 3; ++o) {
        for (int i = 0; i < 3; ++i)
            VQW_CHECK(!cb_overlap(out[o], out_n[o], in[i], in_n[i]), "vqw_vq_cluster_stats: an output must not alias an input");
        for (int p = o + 1; p < 3; ++p)
            VQW_CHECK(!cb_overlap(out[o], out_n[o], out[p], out_n[p]), "vqw_vq_cluster_stats: the outputs must not alias each other");
    }
    hipLaunchKernelGGL(vq_cluster_stats_kernel, dim3(vqw_cdiv(K, CB_WAVES)), dim3(64 * CB_WAVES), 0, (hipStream_t)s, z_e, idx,
                       pick, cnt, sum, cand, B * Tz, D, Tz, K);
    VQW_LAUNCH_CHECK("vqw_vq_cluster_stats");
    return 0;
}

extern "C" int vqw_vq_codebook_ema_step(float* emb, float* n, float* m, const int32_t* cnt, const float* sum, const float* cand,
                                        float g, float h, float tau, int32_t* info, const int32_t* skip, int K, int D,
                                        vqw_stream_t s) {
    VQW_CHECK(emb && n && m && cnt && sum && info, "vqw_vq_codebook_ema_step: null pointer");
    VQW_CHECK(K > 0 && D > 0 && (int64_t)K * D <= (1 << 30), "vqw_vq_codebook_ema_step: K=%d, D=%d must be positive, K*D <= 2^30", K, D);
    VQW_CHECK(g > 0.0f && g < 1.0f && h > 0.0f && h < 1.0f, "vqw_vq_codebook_ema_step: g=%g and h=%g must lie in (0, 1)", g, h);
    VQW_CHECK(tau >= 0.0f && tau < 1.0f, "vqw_vq_codebook_ema_step: tau=%g must lie in [0, 1)", tau);
    VQW_CHECK(cand || tau == 0.0f, "vqw_vq_codebook_ema_step: null pointer (tau > 0 needs cand)");
    const size_t nk = (size_t)K * 4, nkd = (size_t)K * D * 4;
    const void* out[4] = {emb, n, m, info};
    const size_t out_n[4] = {nkd, nk, nkd, 8 * 4};
    const void* in[4] = {cnt, sum, cand, skip};
    const size_t in_n[4] = {nk, nkd, nkd, 4};
    for (int o = 0; o < 4; ++o) {
        for (int i = 0; i < 4; ++i)
            VQW_CHECK(!cb_overlap(out[o], out_n[o], in[i], in_n[i]), "vqw_vq_codebook_ema_step: an output must not alias an input");
        for (int p = o + 1; p < 4; ++p)
            VQW_CHECK(!cb_overlap(out[o], out_n[o], out[p], out_n[p]), "vqw_vq_codebook_ema_step: the outputs must not alias each other");
    }
    hipLaunchKernelGGL(vq_codebook_ema_kernel, dim3(vqw_cdiv(K, CB_WAVES)), dim3(64 * CB_WAVES), 0, (hipStream_t)s, emb, n, m,
                       cnt, sum, cand, g, h, tau, info, skip, K, D);
    VQW_LAUNCH_CHECK("vqw_vq_codebook_ema_step");
    return 0;
}

extern "C" int vqw_speaker_tile_fwd(const float* table, const int64_t* spk, float* cond, int64_t cond_bstride,
                                    int row0, int B, int Cs, int Tz, int n_speakers, vqw_stream_t s) {
    VQW_CHECK(table && spk && cond && B > 0 && Cs > 0 && Tz > 0 && n_speakers > 0, "vqw_speaker_tile_fwd: bad arguments");
    const size_t n = (size_t)B * Cs * Tz;
    int g = (int)((n + 255) / 256);
    if (g > 2048) g = 2048;
    hipLaunchKernelGGL(speaker_tile_fwd_kernel, dim3(g), dim3(256), 0, (hipStream_t)s, table, spk, cond,
                       (long)cond_bstride, row0, B, Cs, Tz, n_speakers);
    VQW_LAUNCH_CHECK("vqw_speaker_tile_fwd");
    return 0;
}

extern "C" int vqw_speaker_tile_bwd(const float* dcond, int64_t dcond_bstride, int row0, const int64_t* spk,
                                    float* dtable, int B, int Cs, int Tz, int n_speakers, vqw_stream_t s) {
    VQW_CHECK(dcond && spk && dtable && B > 0 && Cs > 0 && Tz > 0 && n_speakers > 0, "vqw_speaker_tile_bwd: bad arguments");
    hipLaunchKernelGGL(speaker_tile_bwd_kernel, dim3(vqw_cdiv(B * Cs, 256)), dim3(256), 0, (hipStream_t)s,
                       dcond, (long)dcond_bstride, row0, spk, dtable, B, Cs, Tz, n_speakers);
    VQW_LAUNCH_CHECK("vqw_speaker_tile_bwd");
    return 0;
}
