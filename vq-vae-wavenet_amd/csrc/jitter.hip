// Time-jitter regularisation of the latents for gfx950 (arXiv 1901.08810): in training every latent
// frame the decoder reads is replaced, with probability p, by its left or right neighbour of the SAME utterance.
//   move = -1 if u < lo, +1 if u >= hi, else 0 (fp32 compares; lo = fp32(p / 2), hi = fp32(1 - p / 2) come from the host)
//   src  = t + move, reflected at both ends of the row (-1 -> 1, Tz -> Tz - 2; Tz == 1: 0)
// Forward: a gather along time, no arithmetic.  Backward: the transposed gather in GATHER form -- frame s collects the at
// most three frames t in {s-1, s, s+1} that read it, in ascending t, in fp32 from +0.0f -- so every element is written
// once, nothing is atomic and the result is bitwise reproducible.
// Layout: time is the contiguous axis, so the 64 lanes of a wave take 64 consecutive frames (coalesced up to the +-1 shift
// of the gather) and the four waves of a block take different channels; a lane computes / loads its frame's source index
// once and reuses it over its channels.
#include "vqw_common.h"

namespace {

constexpr int JT_LANES = 64, JT_ROWS = 4;       // block = 64 frames x 4 channel rows
constexpr int JT_DPER = 4;                      // channels per thread the grid is sized for (the loop takes any number)

__device__ __forceinline__ int jitter_src(float u, float lo, float hi, int t, int Tz) {
    int s = t + (u < lo ? -1 : (u >= hi ? 1 : 0));
    if (s < 0) s += 2;
    if (s >= Tz) s -= 2;
    return Tz == 1 ? 0 : s;
}

__global__ __launch_bounds__(JT_LANES * JT_ROWS) void time_jitter_fwd_kernel(
    const float* __restrict__ zq, long zq_bstride, const float* __restrict__ u, float lo, float hi, float* __restrict__ out,
    long out_bstride, int32_t* __restrict__ src, int B, int D, int Tz) {
    const int t = blockIdx.x * JT_LANES + threadIdx.x;
    if (t >= Tz) return;
    for (int b = blockIdx.z; b < B; b += gridDim.z) {
        const int s = jitter_src(u[(size_t)b * Tz + t], lo, hi, t, Tz);
        if (blockIdx.y == 0 && threadIdx.y == 0) src[(size_t)b * Tz + t] = s;
        const float* zb = zq + (size_t)b * zq_bstride;
        float* ob = out + (size_t)b * out_bstride;
        for (int d = blockIdx.y * JT_ROWS + threadIdx.y; d < D; d += gridDim.y * JT_ROWS)
            ob[(size_t)d * Tz + t] = zb[(size_t)d * Tz + s];
    }
}

__global__ __launch_bounds__(JT_LANES * JT_ROWS) void time_jitter_bwd_kernel(
    const float* __restrict__ dout, long dout_bstride, const int32_t* __restrict__ src, float* __restrict__ dzq,
    long dzq_bstride, int B, int D, int Tz) {
    const int s = blockIdx.x * JT_LANES + threadIdx.x;
    if (s >= Tz) return;
    for (int b = blockIdx.z; b < B; b += gridDim.z) {
        const int32_t* sb = src + (size_t)b * Tz;
        const bool left = s > 0 && sb[s - 1] == s, mid = sb[s] == s, right = s + 1 < Tz && sb[s + 1] == s;
        const float* gb = dout + (size_t)b * dout_bstride;
        float* zb = dzq + (size_t)b * dzq_bstride;
        for (int d = blockIdx.y * JT_ROWS + threadIdx.y; d < D; d += gridDim.y * JT_ROWS) {
            const float* g = gb + (size_t)d * Tz + s;
            float acc = 0.0f;
            if (left) acc = __fadd_rn(acc, g[-1]);
            if (mid) acc = __fadd_rn(acc, g[0]);
            if (right) acc = __fadd_rn(acc, g[1]);
            zb[(size_t)d * Tz + s] = acc;
        }
    }
}

int jitter_check(const char* name, const void* a, const void* b, const void* c, const void* d, int64_t bs0, int64_t bs1, int B,
                 int D, int Tz) {
    VQW_CHECK(a && b && c && d, "%s: null pointer", name);
    VQW_CHECK(B > 0 && D > 0 && Tz > 0, "%s: B=%d, D=%d, Tz=%d must be positive", name, B, D, Tz);
    VQW_CHECK(Tz <= (1 << 30), "%s: Tz=%d must be <= 2^30", name, Tz);
    VQW_CHECK(bs0 >= (int64_t)D * Tz && bs1 >= (int64_t)D * Tz, "%s: batch strides %lld, %lld must be >= D*Tz = %lld", name,
              (long long)bs0, (long long)bs1, (long long)D * Tz);
    return 0;
}

dim3 jitter_grid(int B, int D, int Tz) {
    const int gy = vqw_cdiv(D, JT_ROWS * JT_DPER);
    return dim3(vqw_cdiv(Tz, JT_LANES), gy < 65535 ? gy : 65535, B < 65535 ? B : 65535);
}

}  // namespace

extern "C" int vqw_time_jitter_fwd(const float* zq, int64_t zq_bstride, const float* u, float lo, float hi, float* out,
                                   int64_t out_bstride, int32_t* src, int B, int D, int Tz, vqw_stream_t s) {
    if (jitter_check("vqw_time_jitter_fwd", zq, u, out, src, zq_bstride, out_bstride, B, D, Tz)) return 1;
    VQW_CHECK(out != zq, "vqw_time_jitter_fwd: out must not alias zq (a frame would read its neighbour's new value)");
    hipLaunchKernelGGL(time_jitter_fwd_kernel, jitter_grid(B, D, Tz), dim3(JT_LANES, JT_ROWS), 0, (hipStream_t)s, zq,
                       (long)zq_bstride, u, lo, hi, out, (long)out_bstride, src, B, D, Tz);
    VQW_LAUNCH_CHECK("vqw_time_jitter_fwd");
    return 0;
}

extern "C" int vqw_time_jitter_bwd(const float* dout, int64_t dout_bstride, const int32_t* src, float* dzq,
                                   int64_t dzq_bstride, int B, int D, int Tz, vqw_stream_t s) {
    if (jitter_check("vqw_time_jitter_bwd", dout, src, dzq, dzq, dout_bstride, dzq_bstride, B, D, Tz)) return 1;
    VQW_CHECK(dzq != dout, "vqw_time_jitter_bwd: dzq must not alias dout");
    hipLaunchKernelGGL(time_jitter_bwd_kernel, jitter_grid(B, D, Tz), dim3(JT_LANES, JT_ROWS), 0, (hipStream_t)s, dout,
                       (long)dout_bstride, src, dzq, (long)dzq_bstride, B, D, Tz);
    VQW_LAUNCH_CHECK("vqw_time_jitter_bwd");
    return 0;
}
