// mu-law companding in device code (mu_law_ops.py:6-8 and 26-31), ONE definition: the op surface (pointwise.hip), both
// generators (ar_decode.hip, ar_persist.hip) and the teacher-forced sampler (sample.hip) give the same bits for the same input.
#pragma once
#include <hip/hip_runtime.h>

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
