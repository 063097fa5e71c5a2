// mu-law companding in device code (mu_law_ops.py:6-8 and 26-31), ONE definition: the op surface (pointwise.hip), both
// generators (ar_decode.hip, ar_persist.hip) and the teacher-forced sampler (sample.hip) give the same bits for the same input.
//
// Levels: 256 (the reference's only one), 512 and 1024.  vqw_mu_encode / vqw_mu_decode are the 256-level forms with their
// constants folded; the _l forms take mu = Q - 1 and the fp32 log1p(mu) of the level (VqwMu, filled on the host by
// vqw_mu_level from a three-entry table).  A kernel that compands carries a VqwMu and calls the _m forms: at 256 levels
// they branch (wave-uniform) into the folded functions, so the 256 path keeps its bits whatever the compiler makes of a
// runtime powf base.
#pragma once
#include <hip/hip_runtime.h>

struct VqwMu {
    int levels;       // 256, 512 or 1024
    float mu;         // levels - 1
    float log1p_mu;   // np.log1p(np.float32(mu)) in fp32
};

// false: not one of the three levels (m is left at 256)
__host__ inline bool vqw_mu_level(int levels, VqwMu* m) {
    static const VqwMu tab[3] = {{256, 255.0f, 5.5451774444795623f}, {512, 511.0f, 6.23832464f}, {1024, 1023.0f, 6.93147182f}};
    *m = tab[0];
    for (const VqwMu& t : tab)
        if (t.levels == levels) { *m = t; return true; }
    return false;
}

__device__ __forceinline__ float vqw_mu_encode(float x) {
    x = fminf(fmaxf(x, -1.0f), 1.0f);
    const float s = (x > 0.0f) ? 1.0f : ((x < 0.0f) ? -1.0f : 0.0f);
    return s * log1pf(255.0f * fabsf(x)) / 5.5451774444795623f;
}

__device__ __forceinline__ float vqw_mu_decode(float idx) {
    const float y = 2.0f * idx / 255.0f - 1.0f;
    const float s = (y > 0.0f) ? 1.0f : ((y < 0.0f) ? -1.0f : 0.0f);
    return s * (powf(256.0f, fabsf(y)) - 1.0f) / 255.0f;
}

__device__ __forceinline__ float vqw_mu_encode_l(float x, float mu, float log1p_mu) {
    x = fminf(fmaxf(x, -1.0f), 1.0f);
    const float s = (x > 0.0f) ? 1.0f : ((x < 0.0f) ? -1.0f : 0.0f);
    return s * log1pf(mu * fabsf(x)) / log1p_mu;
}

__device__ __forceinline__ float vqw_mu_decode_l(float idx, float mu) {
    const float y = 2.0f * idx / mu - 1.0f;
    const float s = (y > 0.0f) ? 1.0f : ((y < 0.0f) ? -1.0f : 0.0f);
    return s * (powf(mu + 1.0f, fabsf(y)) - 1.0f) / mu;
}

__device__ __forceinline__ float vqw_mu_encode_m(float x, const VqwMu& m) {
    return m.levels == 256 ? vqw_mu_encode(x) : vqw_mu_encode_l(x, m.mu, m.log1p_mu);
}

__device__ __forceinline__ float vqw_mu_decode_m(float idx, const VqwMu& m) {
    return m.levels == 256 ? vqw_mu_decode(idx) : vqw_mu_decode_l(idx, m.mu);
}
