// Teacher-forced sampling for gfx950: one class per position of a logits tensor [B][Q][T], by argmax or by the generators'
// temperature / top-k / top-p sampling (ar_sampling.h), for all B * T positions in one pass.  Straight-line, HBM-bound kernels:
// no atomics, no communication between blocks, every sum in one fixed order, a row's output a function of that row's inputs.
//
// Sample mode calls ar_sample_truncated for EVERY sampled position, default rows (temperature 1, top_k off, top_p 1) included:
// with both truncations off that function is a plain softmax and its lane-major cdf.  A truncated row therefore runs exactly
// the device code the two generators run.  NO bit-equality with the generators' DEFAULT path is promised: that path keeps the
// serial cdf of utils.py (another summation order), so a draw whose uniform lies within rounding of a cdf value may differ.
#include <algorithm>

#include "ar_sampling.h"
#include "mu_law.h"

namespace {

// ----------------------------------------------------------------------------- greedy without probs
// The argmax path of softmax_score_kernel (score.hip): block = NW waves x 64 consecutive time steps of one batch row, wave w
// owns channels [w*Q/NW, (w+1)*Q/NW), every load a 256-byte row segment, sixteen in flight per lane; strict '>' in ascending
// channel order keeps the lowest index among equal maxima, and wave 0 merges the NW candidates in ascending wave order.
template <int NW>
__global__ __launch_bounds__(NW * 64) void greedy_kernel(const float* __restrict__ logits, const int32_t* __restrict__ t_begin,
                                                         const int32_t* __restrict__ t_end, int32_t* __restrict__ idx,
                                                         float* __restrict__ audio, int Q, int T, const VqwMu mu) {
    __shared__ float sv[NW][64];
    __shared__ int si[NW][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int ntile = (T + 63) / 64;
    const int b = blockIdx.x / ntile;
    const int t0 = (blockIdx.x % ntile) * 64;
    const int t = t0 + lane;
    const bool ok = t < T;
    const int tb = t_begin ? max(t_begin[b], 0) : 0;
    const int te = t_end ? min(t_end[b], T) : T;
    if (max(tb, t0) >= min(te, t0 + 64)) {      // no position of this tile is in the range (block-uniform): nothing is read
        if (w == 0 && ok) {
            idx[(size_t)b * T + t] = -1;
            if (audio) audio[(size_t)b * T + t] = 0.0f;
        }
        return;
    }
    const bool in = ok && t >= tb && t < te;
    const int qn = Q / NW, q0 = w * qn;
    const float* lp = logits + ((size_t)b * Q + q0) * T + t;
    float bv = -INFINITY;
    int bi = Q;
    if (in) {
        int q = 0;
        for (; q + 16 <= qn; q += 16) {
            float v[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) v[k] = lp[(size_t)(q + k) * T];
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if (v[k] > bv) { bv = v[k]; bi = q0 + q + k; }
        }
        for (; q < qn; ++q) {
            const float v = lp[(size_t)q * T];
            if (v > bv) { bv = v; bi = q0 + q; }
        }
    }
    sv[w][lane] = bv;
    si[w][lane] = bi;
    __syncthreads();
    if (w != 0 || !ok) return;
    float BV = -INFINITY;
    int BI = Q;
#pragma unroll
    for (int i = 0; i < NW; ++i)
        if (sv[i][lane] > BV) { BV = sv[i][lane]; BI = si[i][lane]; }
    BI = min(BI, Q - 1);                        // nothing compared greater (-inf or NaN everywhere): still a class
    idx[(size_t)b * T + t] = in ? BI : -1;
    if (audio) audio[(size_t)b * T + t] = in ? vqw_mu_decode_m((float)BI, mu) : 0.0f;
}

// ----------------------------------------------------------------------------- sample (and greedy with probs)
// Block = 8 waves x NT consecutive time steps of one batch row (NT a power of two, chosen on the host from Q).  The block
// loads its Q x NT tile with row segments contiguous along t (eight independent loads in flight per lane) and writes it
// TRANSPOSED into LDS, tile[tl][q] with a row stride of Q + 1 floats: a position's Q logits are contiguous, as
// ar_sample_truncated wants its `row`, and the odd stride spreads the transposing writes (lanes along t) over all banks.
// Wave w then takes positions w, w + 8, ... one after another; the row it leaves in LDS (q, or softmax(z) in greedy mode)
// goes to probs[b][t][:] as one contiguous write.  idx / audio are staged in LDS and stored contiguously along t.
constexpr int SMP_THREADS = 512;
constexpr int SMP_ROWS = 32;                    // batch rows of one launch: their settings travel as kernel arguments
struct SmpRows {
    ArSampleRow r[SMP_ROWS];
};

// greedy on one LDS row by one wave: the lowest index among the maxima; the row becomes softmax(z)
__device__ __forceinline__ int smp_greedy_row(float* row, int Q) {
    const int lane = threadIdx.x & 63;
    const int nj = (Q + 63) >> 6, base = lane * nj;
    const int nv = max(0, min(nj, Q - base));
    float* const p = row + base;
    float m = -INFINITY;
    int mi = Q;
    for (int j = 0; j < nv; ++j)
        if (p[j] > m) { m = p[j]; mi = base + j; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float om = __shfl_xor(m, o);
        const int oi = __shfl_xor(mi, o);
        if (om > m || (om == m && oi < mi)) { m = om; mi = oi; }
    }
    float sum = 0.0f;
    for (int j = 0; j < nv; ++j) {
        const float e = __expf(p[j] - m);
        p[j] = e;
        sum += e;
    }
    const float inv = 1.0f / ars_wave_sum(sum);
    for (int j = 0; j < nv; ++j) p[j] *= inv;
    return mi;
}

__global__ __launch_bounds__(SMP_THREADS) void sample_tile_kernel(const float* __restrict__ logits, const float* __restrict__ uniforms,
                                                          const SmpRows rows, const int32_t* __restrict__ t_begin,
                                                          const int32_t* __restrict__ t_end, int mode, int32_t* __restrict__ idx,
                                                          float* __restrict__ audio, float* __restrict__ probs, int Q, int T,
                                                          int nt_shift, const VqwMu mu) {
    extern __shared__ float tile[];             // [NT][Q + 1]
    __shared__ int sidx[64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int NT = 1 << nt_shift, ld = Q + 1;
    const int ntile = (T + NT - 1) >> nt_shift;
    const int b = blockIdx.x / ntile;
    const int t0 = (blockIdx.x % ntile) << nt_shift;
    const int tb = t_begin ? max(t_begin[b], 0) : 0;
    const int te = t_end ? min(t_end[b], T) : T;
    const int lo = max(tb, t0), hi = min(te, t0 + NT);           // this tile's positions in the range: [lo, hi)
    if (lo < hi) {
        const float* lp = logits + (size_t)b * Q * T + t0;
        const int total = Q << nt_shift, mask = NT - 1;
        for (int i0 = tid; i0 < total; i0 += SMP_THREADS * 8) {
            float v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int i = i0 + SMP_THREADS * k, tl = i & mask;
                v[k] = (i < total && t0 + tl < T) ? lp[(size_t)(i >> nt_shift) * T + tl] : 0.0f;
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int i = i0 + SMP_THREADS * k;
                if (i < total) tile[(i & mask) * ld + (i >> nt_shift)] = v[k];
            }
        }
    }
    __syncthreads();
    const ArSampleRow s = rows.r[b % SMP_ROWS];
    for (int tl = w; tl < NT; tl += SMP_THREADS / 64) {
        const int t = t0 + tl;
        if (t >= T) break;
        float* const row = tile + tl * ld;
        float* const pr = probs ? probs + ((size_t)b * T + t) * Q : nullptr;
        if (t < lo || t >= hi) {                // outside the range (wave-uniform)
            if (lane == 0) sidx[tl] = -1;
            if (pr)
                for (int q = lane; q < Q; q += 64) pr[q] = 0.0f;
            continue;
        }
        int c;
        if (mode == 0)
            c = smp_greedy_row(row, Q);
        else
            c = ar_sample_truncated(row, Q, s, uniforms[(size_t)b * T + t], nullptr);
        c = min(max(c, 0), Q - 1);              // non-finite logits: still a class
        if (lane == 0) sidx[tl] = c;
        if (pr) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // lanes read each other's LDS writes (same wave)
            for (int q = lane; q < Q; q += 64) pr[q] = row[q];
        }
    }
    __syncthreads();
    if (tid < NT && t0 + tid < T) {
        const int c = sidx[tid];
        idx[(size_t)b * T + t0 + tid] = c;
        if (audio) audio[(size_t)b * T + t0 + tid] = c >= 0 ? vqw_mu_decode_m((float)c, mu) : 0.0f;
    }
}

// the largest power of two NT <= 64 whose tile NT x (Q + 1) floats fits 64 KB of LDS
inline int sample_nt_shift(int Q) {
    int sh = 6;
    while (sh > 0 && ((int64_t)(Q + 1) << sh) > 16384) --sh;
    return sh;
}

// both entry points; fn names the caller in the messages, mu is the level audio is decoded at
int softmax_sample(const char* fn, const float* logits, const float* uniforms, const vqw_ar_sampling* rows, const int32_t* t_begin,
                   const int32_t* t_end, int mode, int32_t* idx, float* audio, float* probs, int B, int Q, int T, const VqwMu& mu,
                   vqw_stream_t s) {
    VQW_CHECK(logits && idx, "%s: null pointer", fn);
    VQW_CHECK(B >= 1 && T >= 1, "%s: bad shape B=%d T=%d", fn, B, T);
    VQW_CHECK(Q >= 1 && Q % 4 == 0 && Q <= 1024, "%s: Q=%d must be a multiple of 4 and at most 1024", fn, Q);
    VQW_CHECK(mode == 0 || mode == 1, "%s: mode %d must be 0 (greedy) or 1 (sample)", fn, mode);
    VQW_CHECK(mode == 0 || uniforms, "%s: mode 1 (sample) needs uniforms", fn);
    VQW_CHECK(!audio || Q == mu.levels, "%s: audio is the mu-law decode of %d classes (Q=%d)", fn, mu.levels, Q);
    SmpRows group;
    int any = 0;
    for (int b0 = 0; b0 < B; b0 += SMP_ROWS)    // every row's settings are checked before the first launch
        if (ar_sampling_rows(rows ? rows + b0 : nullptr, std::min(SMP_ROWS, B - b0), Q, mode, group.r, &any)) return 1;
    if (mode == 0 && !probs) {
        const int ntile = vqw_cdiv(T, 64);
        VQW_CHECK((int64_t)B * ntile < (int64_t)1 << 31, "%s: B * ceil(T / 64) must be below 2^31", fn);
        if (Q % 128 == 0)
            hipLaunchKernelGGL(greedy_kernel<8>, dim3(B * ntile), dim3(512), 0, (hipStream_t)s, logits, t_begin, t_end, idx, audio, Q, T, mu);
        else
            hipLaunchKernelGGL(greedy_kernel<4>, dim3(B * ntile), dim3(256), 0, (hipStream_t)s, logits, t_begin, t_end, idx, audio, Q, T, mu);
        VQW_LAUNCH_CHECK("vqw_softmax_sample (greedy)");
        return 0;
    }
    const int sh = sample_nt_shift(Q);
    const int ntile = (T + (1 << sh) - 1) >> sh;
    VQW_CHECK((int64_t)SMP_ROWS * ntile < (int64_t)1 << 31, "%s: T too large", fn);
    const size_t lds = ((size_t)(Q + 1) << sh) * sizeof(float);
    for (int b0 = 0; b0 < B; b0 += SMP_ROWS) {
        const int nb = std::min(SMP_ROWS, B - b0);
        for (int i = 0; i < SMP_ROWS; ++i) group.r[i] = ArSampleRow{1.0f, 0, 1.0f, 0};
        if (ar_sampling_rows(rows ? rows + b0 : nullptr, nb, Q, mode, group.r, &any)) return 1;
        const size_t o = (size_t)b0 * T;
        hipLaunchKernelGGL(sample_tile_kernel, dim3(nb * ntile), dim3(SMP_THREADS), lds, (hipStream_t)s, logits + o * Q,
                           uniforms ? uniforms + o : nullptr, group, t_begin ? t_begin + b0 : nullptr, t_end ? t_end + b0 : nullptr, mode,
                           idx + o, audio ? audio + o : nullptr, probs ? probs + o * Q : nullptr, Q, T, sh, mu);
        VQW_LAUNCH_CHECK("vqw_softmax_sample");
    }
    return 0;
}

}  // namespace

// ============================================================================ C ABI
extern "C" int vqw_softmax_sample(const float* logits, const float* uniforms, const vqw_ar_sampling* rows, const int32_t* t_begin,
                                  const int32_t* t_end, int mode, int32_t* idx, float* audio, float* probs, int B, int Q, int T,
                                  vqw_stream_t s) {
    VqwMu mu;
    vqw_mu_level(256, &mu);
    return softmax_sample("vqw_softmax_sample", logits, uniforms, rows, t_begin, t_end, mode, idx, audio, probs, B, Q, T, mu, s);
}

// audio decoded at 256, 512 or 1024 levels (with audio given, Q must be that level)
extern "C" int vqw_softmax_sample_levels(const float* logits, const float* uniforms, const vqw_ar_sampling* rows,
                                         const int32_t* t_begin, const int32_t* t_end, int mode, int32_t* idx, float* audio,
                                         float* probs, int B, int Q, int T, int levels, vqw_stream_t s) {
    VqwMu mu;
    VQW_CHECK(vqw_mu_level(levels, &mu), "vqw_softmax_sample_levels: levels=%d must be 256, 512 or 1024", levels);
    return softmax_sample("vqw_softmax_sample_levels", logits, uniforms, rows, t_begin, t_end, mode, idx, audio, probs, B, Q, T, mu, s);
}
