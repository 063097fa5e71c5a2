// Segmented sum of squares over a flat fp32 buffer for gfx950: the global gradient norm, the clipping scale and one norm per
// segment, left on the device.  Two launches, no floating-point atomics: the result is bitwise reproducible and a
// segment's norm depends on that segment's values alone.
#include "vqw_common.h"

namespace {

constexpr int GN_MAX_SEG = 2048;     // segment ranges and sums of the final stage live in LDS (32 KiB)

__device__ __forceinline__ double gn_sq(float x, float gs) {
    // g = x * gs in fp32, as the optimiser forms it; the SQUARE is fp64 (an fp32 square is 0 below 1e-19 and inf above 1.8e19)
    const double d = (double)(x * gs);
    return d * d;
}

// Stage 1: one workgroup per chunk.  Thread t adds, in this order: its head element, its 16-byte groups of the aligned
// interior (t, t + 256, ...), its tail element; then a fixed shuffle tree per wave and the four wave sums in order.
__global__ __launch_bounds__(256) void gradnorm_partial_kernel(const float* __restrict__ buf, const vqw_norm_chunk* __restrict__ chunks,
                                                               double* __restrict__ partial, float gs) {
    __shared__ double red[4];
    const vqw_norm_chunk ck = chunks[blockIdx.x];
    const float* p = buf + ck.start;
    const int len = ck.length, tid = threadIdx.x;
    int head = (int)((4u - (unsigned)((reinterpret_cast<uintptr_t>(p) >> 2) & 3u)) & 3u);     // floats up to the next 16-byte boundary
    if (head > len) head = len;
    const int n4 = (len - head) >> 2, tail0 = head + 4 * n4;
    double acc = 0.0;
    if (tid < head) acc = gn_sq(p[tid], gs);
    const f32x4* p4 = reinterpret_cast<const f32x4*>(p + head);
#pragma unroll 4
    for (int q = tid; q < n4; q += 256) {
        const f32x4 v = p4[q];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc += gn_sq(v[e], gs);
    }
    if (tail0 + tid < len) acc += gn_sq(p[tail0 + tid], gs);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) partial[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// Stage 2: one workgroup.  The chunks of a segment are consecutive in the table; a wave sums one segment's partials (lane j
// takes chunks j, j + 64, ... of the segment in ascending order, then the shuffle tree), thread 0 adds the segments in
// ascending order.  A table that breaks the contract gives wrong sums, never an access outside partial[0, n_chunks) / out.
__global__ __launch_bounds__(1024) void gradnorm_final_kernel(const vqw_norm_chunk* __restrict__ chunks, const double* __restrict__ partial,
                                                              int n_chunks, int n_seg, float clip, float* __restrict__ out) {
    __shared__ int first[GN_MAX_SEG], last[GN_MAX_SEG];
    __shared__ double segsum[GN_MAX_SEG];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int s = tid; s < n_seg; s += 1024) first[s] = last[s] = 0;
    __syncthreads();
#pragma unroll 4
    for (int c = tid; c < n_chunks; c += 1024) {
        const int sp = chunks[c > 0 ? c - 1 : 0].seg, sc = chunks[c].seg, sn = chunks[c + 1 < n_chunks ? c + 1 : c].seg;
        if (sc >= 0 && sc < n_seg) {
            if (c == 0 || sp != sc) first[sc] = c;
            if (c == n_chunks - 1 || sn != sc) last[sc] = c + 1;
        }
    }
    __syncthreads();
    for (int s = wave; s < n_seg; s += 16) {
        const int hi = last[s];
        double acc = 0.0;
        for (int c = first[s] + lane; c < hi; c += 64) acc += partial[c];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
        if (lane == 0) {
            segsum[s] = acc;
            out[2 + s] = (float)sqrt(acc);
        }
    }
    __syncthreads();
    if (tid == 0) {
        double total = 0.0;
#pragma unroll 8
        for (int s = 0; s < n_seg; ++s) total += segsum[s];
        const float norm = (float)sqrt(total);
        out[0] = norm;
        out[1] = norm <= clip ? 1.0f : clip / norm;      // a NaN norm fails the comparison and gives a NaN scale
    }
}

}  // namespace

extern "C" int vqw_grad_norm_segmented(const float* buf, const vqw_norm_chunk* chunks, int n_chunks, int n_seg, double* partial,
                                       float grad_scale, float clip, float* out, vqw_stream_t s) {
    VQW_CHECK(buf && chunks && partial && out, "vqw_grad_norm_segmented: null pointer");
    VQW_CHECK(n_chunks >= 1, "vqw_grad_norm_segmented: n_chunks=%d must be >= 1", n_chunks);
    VQW_CHECK(n_seg >= 1 && n_seg <= GN_MAX_SEG, "vqw_grad_norm_segmented: n_seg=%d must be in [1, %d]", n_seg, GN_MAX_SEG);
    VQW_CHECK(clip > 0.0f, "vqw_grad_norm_segmented: clip must be > 0 (+inf = measure only; NaN is refused)");
    hipLaunchKernelGGL(gradnorm_partial_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)s, buf, chunks, partial, grad_scale);
    VQW_LAUNCH_CHECK("vqw_grad_norm_segmented");
    hipLaunchKernelGGL(gradnorm_final_kernel, dim3(1), dim3(1024), 0, (hipStream_t)s, chunks, (const double*)partial, n_chunks, n_seg, clip, out);
    VQW_LAUNCH_CHECK("vqw_grad_norm_segmented");
    return 0;
}
