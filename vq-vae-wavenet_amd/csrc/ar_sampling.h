// The generators' sampling of one batch row.
//
// ar_sample_truncated: temperature, top-k and nucleus (top-p) sampling by ONE wave, shared by the persistent generator
// (ar_persist.hip decode_rows), the launch-per-phase path (ar_decode.hip ar_sample_kernel), the wide generator (ar_wide.hip
// arw_sample_kernel) and the all-positions pass (sample.hip).  Rows at their defaults (temperature 1, top_k off, top_p 1)
// never come there: they keep the plain softmax + serial cdf of utils.py:13-46 bit for bit, which for a 256-thread block is
// ar_sample_default (ar_sample_kernel, arw_sample_kernel; the persistent kernel has its own in decode_rows).
//
// Semantics (include/vqwave.h, vqw_ar_sampling):  p = softmax(z / T) (max subtracted first);  top-k keeps the first K classes
// in the order (p descending, index ascending);  top-p keeps, in the same order, the shortest prefix of the kept set whose
// mass is >= P times the kept mass;  q = p on the kept set, renormalised;  the draw is the first kept index whose ascending
// cdf of q reaches u, or the largest kept index when u lies above the last cdf value.
//
// Layout: lane l holds classes l*nj .. l*nj + nj - 1 (nj = ceil(Q/64)), so index order is lane-major and a lane's prefix is
// serial.  Every decision is wave-uniform and every sum has one fixed order (per lane in j order, then a DPP reduction
// whose total lane 63 broadcasts): the persistent kernel runs this redundantly in every workgroup and gets the same bits.
//   - top-k: bisection over the fp32 bit patterns of p (non-negative, so they order as uint32): count(p >= cand) by an exact
//     integer DPP reduction; ties at the K-th value filled in index order from ballot prefix counts;
//   - top-p: bisection over the same bit patterns on the mass M(x) = sum of kept p >= x (monotone in x: one summation order
//     with the dropped terms as zeros); ties at the cut filled in index order while the prefix mass is below the target;
//   - cdf: serial per lane + one shuffle scan of the lane totals.
#pragma once
#include "vqw_common.h"

// per-row settings as the kernels read them (host: ar_sampling_rows)
struct ArSampleRow {
    float temperature;
    int top_k;        // 0 = off (K >= Q is stored as 0)
    float top_p;      // 1 = off
    int on;           // 0: the row takes the default path
};

constexpr int AR_SAMPLE_MAXJ = 16;   // classes per lane: Q <= 1024

// sum over the 64 lanes of a wave with DPP only; the total of lane 63, broadcast
__device__ __forceinline__ float ars_wave_sum(float v) {
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, false));    // quad_perm [1,0,3,2]
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, false));    // quad_perm [2,3,0,1]
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xF, 0xF, false));   // row_half_mirror
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xF, 0xF, false));   // row_mirror
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x142, 0xA, 0xF, false));   // row_bcast15
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x143, 0xC, 0xF, false));   // row_bcast31
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

__device__ __forceinline__ int ars_wave_isum(int v) {   // the same for integers (exact): the total is in lane 63
    v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, false);
    return v;
}
// sum of v over the lanes below mine (v small and non-negative: counts per lane, < 32): bit planes by ballots
__device__ __forceinline__ int ars_wave_excl_isum(int v, unsigned long long lt_mask) {
    int r = 0;
#pragma unroll
    for (int b = 0; b < 6; ++b) r += __popcll(__ballot((v >> b) & 1) & lt_mask) << b;
    return r;
}

// The sampled class of one row (the same value in every lane).  row: the row's Q logits in LDS, overwritten with p, then with
// the sampled distribution q (lane l only touches its own classes l*nj.., so no barrier is needed; p stays in LDS rather
// than registers to keep the register budget of the kernels that inline this); u: the row's uniform of this step;
// q_out (may be null): a global copy of q.  Called by all 64 lanes of one wave, with Q <= 64 * AR_SAMPLE_MAXJ.
__device__ __forceinline__ int ar_sample_truncated(float* row, int Q, const ArSampleRow& s, float u, float* q_out) {
    const int lane = threadIdx.x & 63;
    const int nj = (Q + 63) >> 6, base = lane * nj;
    const int nv = max(0, min(nj, Q - base));   // my classes: row[base .. base + nv)
    float* const p = row + base;
    const unsigned valid = (nv >= 32) ? ~0u : (1u << nv) - 1u;
    float m = -INFINITY;
    for (int j = 0; j < nv; ++j) m = fmaxf(m, p[j]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    // 1. p = softmax(z / T)
    const float rt = 1.0f / s.temperature;
    float sum = 0.0f;
    for (int j = 0; j < nv; ++j) {
        const float e = __expf((p[j] - m) * rt);
        p[j] = e;
        sum += e;
    }
    const float inv = 1.0f / ars_wave_sum(sum);
    for (int j = 0; j < nv; ++j) p[j] *= inv;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    unsigned keep = valid;
    // 2. top-k
    if (s.top_k > 0) {
        unsigned ans = 0;                      // the K-th largest bit pattern (p <= 1: bits 30, 31 are zero)
        for (int bit = 29; bit >= 0; --bit) {
            const unsigned cand = ans | (1u << bit);
            int cnt = 0;
            for (int j = 0; j < nv; ++j) cnt += __float_as_uint(p[j]) >= cand;
            cnt = __builtin_amdgcn_readlane(ars_wave_isum(cnt), 63);
            if (cnt >= s.top_k) ans = cand;
        }
        int gt = 0, eq = 0;                    // my classes above the K-th value / tied with it
        for (int j = 0; j < nv; ++j) {
            const unsigned bits = __float_as_uint(p[j]);
            gt += bits > ans;
            eq += bits == ans;
        }
        const int need = s.top_k - __builtin_amdgcn_readlane(ars_wave_isum(gt), 63);   // >= 1 ties to keep
        int rank = ars_wave_excl_isum(eq, lt_mask);   // ties in the lanes before mine
        unsigned k2 = 0;
        for (int j = 0; j < nv; ++j) {
            const unsigned bits = __float_as_uint(p[j]);
            if (bits > ans) k2 |= 1u << j;
            else if (bits == ans) {
                if (rank < need) k2 |= 1u << j;
                ++rank;
            }
        }
        keep = k2;
    }
    // 3. top-p over the kept set
    if (s.top_p < 1.0f) {
        auto mass = [&](unsigned cand, bool strict) {
            float v = 0.0f;
            for (int j = 0; j < nv; ++j) {
                const unsigned bits = __float_as_uint(p[j]);
                const bool in = ((keep >> j) & 1u) && (strict ? bits > cand : bits >= cand);
                v += in ? p[j] : 0.0f;
            }
            return ars_wave_sum(v);
        };
        const float target = fmaxf(s.top_p * mass(0u, false), 1.17549435e-38f);   // >= 1 class whatever P
        unsigned ans = 0;                      // the largest x with M(x) >= target: the value at the cut
        for (int bit = 29; bit >= 0; --bit) {
            const unsigned cand = ans | (1u << bit);
            if (mass(cand, false) >= target) ans = cand;
        }
        const float above = mass(ans, true);   // < target
        const float cut = __uint_as_float(ans);
        int eq = 0;
        for (int j = 0; j < nv; ++j) eq += ((keep >> j) & 1u) && __float_as_uint(p[j]) == ans;
        int rank = ars_wave_excl_isum(eq, lt_mask);
        unsigned k2 = 0;
        for (int j = 0; j < nv; ++j) {
            if (!((keep >> j) & 1u)) continue;
            const unsigned bits = __float_as_uint(p[j]);
            if (bits > ans) k2 |= 1u << j;
            else if (bits == ans) {
                if (above + (float)rank * cut < target) k2 |= 1u << j;   // the prefix before this tie is still short
                ++rank;
            }
        }
        keep = k2;
    }
    // 4. q = p on the kept set, renormalised; ascending cdf; draw
    float ks = 0.0f;
    for (int j = 0; j < nv; ++j) ks += ((keep >> j) & 1u) ? p[j] : 0.0f;
    const float kinv = 1.0f / ars_wave_sum(ks);
    float run = 0.0f;
    for (int j = 0; j < nv; ++j) {
        const float q = ((keep >> j) & 1u) ? p[j] * kinv : 0.0f;
        p[j] = q;
        run += q;
        if (q_out) q_out[base + j] = q;
    }
    float pre = run;                           // inclusive scan of the lane totals
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const float o = __shfl_up(pre, d);
        if (lane >= d) pre += o;
    }
    const float prev_lanes = __shfl_up(pre, 1);
    float c = (lane == 0) ? 0.0f : prev_lanes;  // the mass of the lanes before mine
    int first_hit = -1;
    for (int j = 0; j < nv; ++j) {
        c += p[j];
        if (first_hit < 0 && ((keep >> j) & 1u) && c >= u) first_hit = j;
    }
    const int last_kept = keep ? 31 - __clz((int)keep) : 0;
    const unsigned long long hl = __ballot(first_hit >= 0);
    if (hl) {                                  // the first kept index whose cdf reaches u
        const int l0 = __ffsll((unsigned long long)hl) - 1;
        return l0 * nj + __shfl(first_hit, l0);
    }
    const unsigned long long kl = __ballot(keep != 0);   // u above the last cdf value: the largest kept index
    const int l1 = 63 - __clzll((long long)kl);
    return l1 * nj + __shfl(last_kept, l1);
}

// A row at its defaults, by a block of 256 threads (all of them call): softmax with the maximum subtracted (wavenet.py:171),
// then utils.decode (utils.py:30-46): mode 0 the lowest index among the maxima (np.argmax), mode 1 a sequential fp32 cumsum
// and searchsorted left, which gives Q when *u lies above the last cdf value.  The index is returned in thread 0 only.
// logits: the row's Q <= 1024 logits in global memory, `stride` floats apart; sp [Q], redv [4], redi [4]: LDS scratch of the
// block, sp is left holding p; u: the row's uniform of this step, read by thread 0 in mode 1 only; p0, p1 (either may be
// null): global copies of p.  May be called row after row on the same scratch: the barrier at the top ends the last call's
// reads of it (thread 0's of sp among them); until the last barrier a thread touches only the sp[q] it wrote itself.
__device__ __forceinline__ int ar_sample_default(const float* logits, size_t stride, float* sp, float* redv, int* redi, int Q,
                                                 int mode, const float* u, float* p0, float* p1) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    __syncthreads();
    float m = -INFINITY;
    int mi = 0x7fffffff;
    for (int q = tid; q < Q; q += 256) {
        const float v = logits[q * stride];
        sp[q] = v;
        if (v > m) { m = v; mi = q; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float om = __shfl_xor(m, o);
        const int oi = __shfl_xor(mi, o);
        if (om > m || (om == m && oi < mi)) { m = om; mi = oi; }
    }
    if (lane == 0) { redv[wv] = m; redi[wv] = mi; }
    __syncthreads();
    m = redv[0]; mi = redi[0];
#pragma unroll
    for (int w = 1; w < 4; ++w)
        if (redv[w] > m || (redv[w] == m && redi[w] < mi)) { m = redv[w]; mi = redi[w]; }
    float s = 0.0f;
    for (int q = tid; q < Q; q += 256) {
        const float e = __expf(sp[q] - m);
        sp[q] = e;
        s += e;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    __syncthreads();                           // every wave has read the maxima
    if (lane == 0) redv[wv] = s;
    __syncthreads();
    s = (redv[0] + redv[1]) + (redv[2] + redv[3]);
    const float inv = 1.0f / s;
    for (int q = tid; q < Q; q += 256) {
        const float p = sp[q] * inv;
        sp[q] = p;
        if (p0) p0[q] = p;
        if (p1) p1[q] = p;
    }
    __syncthreads();
    if (tid != 0 || mode == 0) return mi;
    const float uu = *u;
    float cs = 0.0f;
    int idx = 0;
    for (int q = 0; q < Q; ++q) {
        cs += sp[q];
        if (cs < uu) idx = q + 1;
    }
    return idx;
}

// host: validate the per-row settings of one handle (NULL = all defaults) and turn them into ArSampleRow; `any` is set when
// at least one row leaves the default path.  Errors go through vqw_set_error (non-zero return).
inline int ar_sampling_rows(const vqw_ar_sampling* s, int B, int Q, int mode, ArSampleRow* out, int* any) {
    for (int b = 0; b < B; ++b) {
        ArSampleRow r = {1.0f, 0, 1.0f, 0};
        if (s) {
            const vqw_ar_sampling& v = s[b];
            if (!(v.temperature > 0.0f) || !(v.temperature <= 3.4028235e38f))
                return vqw_set_error("vqw_ar_sampling: row %d: temperature %g must be finite and > 0", b, (double)v.temperature);
            if (v.top_k < 0) return vqw_set_error("vqw_ar_sampling: row %d: top_k %d must be >= 0", b, (int)v.top_k);
            if (!(v.top_p > 0.0f && v.top_p <= 1.0f))
                return vqw_set_error("vqw_ar_sampling: row %d: top_p %g must be in (0, 1]", b, (double)v.top_p);
            r.temperature = v.temperature;
            r.top_k = (v.top_k >= Q) ? 0 : v.top_k;
            r.top_p = v.top_p;
            r.on = (r.temperature != 1.0f || r.top_k > 0 || r.top_p < 1.0f) ? 1 : 0;
        }
        if (r.on && mode != 1)
            return vqw_set_error("vqw_ar_sampling: row %d: temperature / top_k / top_p apply to mode 1 (sample) only", b);
        if (r.on && Q > 64 * AR_SAMPLE_MAXJ)
            return vqw_set_error("vqw_ar_sampling: truncated sampling supports Q <= %d (got %d)", 64 * AR_SAMPLE_MAXJ, Q);
        if (r.on) *any = 1;
        out[b] = r;
    }
    return 0;
}
