// HBM-bound kernels of the hot path for gfx950: mu-law companding, Cin==1 convs, row
// reductions, transposes, softmax cross-entropy and the fused Adam+EMA step.
// Reference call sites are cited per kernel; numerics follow SURVEY.md Appendix A.
#include "mu_law.h"
#include "mu_law_table.h"
#include "mu_law_table_512.h"
#include "mu_law_table_1024.h"
#include "vqw_common.h"

namespace {

__device__ __constant__ unsigned int VQW_MU_LAW_THR_BITS_DEV[255] = VQW_MU_LAW_THR_BITS_LIST;
__device__ __constant__ unsigned int VQW_MU_LAW_THR_BITS_DEV_512[511] = VQW_MU_LAW_THR_BITS_LIST_512;
__device__ __constant__ unsigned int VQW_MU_LAW_THR_BITS_DEV_1024[1023] = VQW_MU_LAW_THR_BITS_LIST_1024;

// ----------------------------------------------------------------------------- mu-law (the float forms: mu_law.h)
// label(x) = #{thr <= clip(x)}: compares only => bit-exact vs the fp32 formula
// (mu_law_ops.py:11); table from tools/gen_mu_law_table.py.
__device__ __forceinline__ int mu_encode_i(float x, const float* thr) {
    x = fminf(fmaxf(x, -1.0f), 1.0f);
    int lo = 0, hi = 255;
#pragma unroll
    for (int it = 0; it < 8; ++it) {
        const int mid = (lo + hi) >> 1;
        const bool ge = (lo < hi) && (thr[mid] <= x);
        const bool lt = (lo < hi) && !(thr[mid] <= x);
        lo = ge ? mid + 1 : lo;
        hi = lt ? mid : hi;
    }
    return lo;
}

__device__ __forceinline__ void load_thr(float* thr) {
    for (int i = threadIdx.x; i < 255; i += blockDim.x) thr[i] = __uint_as_float(VQW_MU_LAW_THR_BITS_DEV[i]);
    __syncthreads();
}

__global__ void mu_encode_f32_kernel(const float* __restrict__ x, float* __restrict__ y, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        y[i] = vqw_mu_encode(x[i]);
}

__global__ void mu_encode_i32_kernel(const float* __restrict__ x, int32_t* __restrict__ y, size_t n) {
    __shared__ float thr[256];
    load_thr(thr);
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        y[i] = mu_encode_i(x[i], thr);
}

__global__ void mu_decode_f32_kernel(const float* __restrict__ idx, float* __restrict__ x, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        x[i] = vqw_mu_decode(idx[i]);
}

// wavenet.py:33-37: labels from x, decoder input from shift_right(x) (wavenet_ops.py:9-14)
__global__ void wavenet_inputs_kernel(const float* __restrict__ x, float* __restrict__ inputs,
                                      int32_t* __restrict__ labels, int B, int T) {
    __shared__ float thr[256];
    load_thr(thr);
    const size_t n = (size_t)B * T;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int t = (int)(i % T);
        const float v = x[i];
        if (labels) labels[i] = mu_encode_i(v, thr);
        if (inputs) inputs[i] = (t == 0) ? 0.0f : vqw_mu_encode(x[i - 1]);
    }
}

// ----------------------------------------------------------------------------- mu-law at 512 / 1024 levels
// The same kernels with the level as a template argument (LV - 1 thresholds in LDS, log2(LV) halvings) and its constants as
// arguments (mu_law.h).  The 256-level kernels above stay as they are: the _levels entry points launch THEM at 256.
template <int LV>
__device__ __forceinline__ int mu_encode_i_lv(float x, const float* thr) {
    static_assert(LV == 512 || LV == 1024, "levels");
    x = fminf(fmaxf(x, -1.0f), 1.0f);
    int lo = 0, hi = LV - 1;
#pragma unroll
    for (int it = 0; it < (LV == 512 ? 9 : 10); ++it) {
        const int mid = (lo + hi) >> 1;
        const bool ge = (lo < hi) && (thr[mid] <= x);
        const bool lt = (lo < hi) && !(thr[mid] <= x);
        lo = ge ? mid + 1 : lo;
        hi = lt ? mid : hi;
    }
    return lo;
}

template <int LV>
__device__ __forceinline__ void load_thr_lv(float* thr) {
    const unsigned int* bits = LV == 512 ? VQW_MU_LAW_THR_BITS_DEV_512 : VQW_MU_LAW_THR_BITS_DEV_1024;
    for (int i = threadIdx.x; i < LV - 1; i += blockDim.x) thr[i] = __uint_as_float(bits[i]);
    __syncthreads();
}

__global__ void mu_encode_f32_lv_kernel(const float* __restrict__ x, float* __restrict__ y, size_t n, float mu, float log1p_mu) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        y[i] = vqw_mu_encode_l(x[i], mu, log1p_mu);
}

template <int LV>
__global__ void mu_encode_i32_lv_kernel(const float* __restrict__ x, int32_t* __restrict__ y, size_t n) {
    __shared__ float thr[LV];
    load_thr_lv<LV>(thr);
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        y[i] = mu_encode_i_lv<LV>(x[i], thr);
}

__global__ void mu_decode_f32_lv_kernel(const float* __restrict__ idx, float* __restrict__ x, size_t n, float mu) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        x[i] = vqw_mu_decode_l(idx[i], mu);
}

template <int LV>
__global__ void wavenet_inputs_lv_kernel(const float* __restrict__ x, float* __restrict__ inputs, int32_t* __restrict__ labels,
                                         int B, int T, float mu, float log1p_mu) {
    __shared__ float thr[LV];
    load_thr_lv<LV>(thr);
    const size_t n = (size_t)B * T;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int t = (int)(i % T);
        const float v = x[i];
        if (labels) labels[i] = mu_encode_i_lv<LV>(v, thr);
        if (inputs) inputs[i] = (t == 0) ? 0.0f : vqw_mu_encode_l(x[i - 1], mu, log1p_mu);
    }
}

// ----------------------------------------------------------------------------- Cin == 1 convs
// wavenet.py:42-44 (preprocess, causal k=32) and encoder.py:15 layer 1 (k=5, stride 2, SAME).
// Block = 256 threads x 4 consecutive output times for FT output channels; the input window of
// the block (stride*1024 + k samples) is staged once in LDS, every thread keeps ITS window (3*stride + k samples) in
// registers (STRIDE is a template argument for that; 0 = any stride, window read from LDS tap by tap) and the taps of the
// block's channels sit in LDS too, so the kernel is bound by its output stream (HBM), not by LDS reads.
template <int KMAX, int FT, int STRIDE>
__global__ __launch_bounds__(256) void conv_cin1_fwd_kernel(
    const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
    const float* __restrict__ scale, const float* __restrict__ shift, float* __restrict__ out,
    float* __restrict__ save_r, int T_in, int T_out, int F, int k, int stride, int offset, int relu) {
    extern __shared__ float cs[];
    const int f0 = blockIdx.y * FT, b = blockIdx.z;
    const int tb = 4 * blockIdx.x * 256;                  // first output time of the block
    const int win = stride * 1024 + KMAX;                 // staged input samples
    float* xs = cs;                                       // [win]
    float* ws = cs + win;                                 // [KMAX][FT]
    const float* xr = x + (size_t)b * T_in;
    const int i0 = stride * tb + offset;                  // input index of xs[0]
    for (int i = threadIdx.x; i < win; i += 256) {
        const int ti = i0 + i;
        xs[i] = (ti >= 0 && ti < T_in) ? xr[ti] : 0.0f;
    }
    for (int i = threadIdx.x; i < KMAX * FT; i += 256) {
        const int j = i / FT, ff = i % FT;
        ws[i] = (j < k && f0 + ff < F) ? w[(size_t)j * F + f0 + ff] : 0.0f;
    }
    __syncthreads();
    const int t0 = tb + 4 * threadIdx.x;
    if (t0 >= T_out) return;
    const int xo = stride * 4 * threadIdx.x;
    constexpr int WIN = STRIDE > 0 ? 3 * STRIDE + KMAX : 1;
    float xw[WIN];
    if (STRIDE > 0) {
#pragma unroll
        for (int i = 0; i < WIN; ++i) xw[i] = xs[xo + i];
    }
    for (int ff = 0; ff < FT; ++ff) {
        const int f = f0 + ff;
        if (f >= F) break;
        float acc[4];
        const float bv = bias ? bias[f] : 0.0f;
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = bv;
#pragma unroll
        for (int j = 0; j < KMAX; ++j) {
            const float wv = ws[j * FT + ff];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = fmaf(wv, STRIDE > 0 ? xw[STRIDE * e + j] : xs[xo + stride * e + j], acc[e]);
        }
        const size_t ro = ((size_t)b * F + f) * T_out;
        float r[4], y[4];
        const float sc = scale ? scale[f] : 1.0f, sh = scale ? shift[f] : 0.0f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            r[e] = relu ? fmaxf(acc[e], 0.0f) : acc[e];
            y[e] = scale ? sc * r[e] + sh : r[e];
        }
        if (t0 + 3 < T_out && (T_out & 3) == 0) {
            *reinterpret_cast<f32x4*>(out + ro + t0) = f32x4{y[0], y[1], y[2], y[3]};
            if (save_r) *reinterpret_cast<f32x4*>(save_r + ro + t0) = f32x4{r[0], r[1], r[2], r[3]};
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (t0 + e < T_out) {
                    out[ro + t0 + e] = y[e];
                    if (save_r) save_r[ro + t0 + e] = r[e];
                }
        }
    }
}

// dw[j][f] += sum_{b,t} x[b][stride*t+j+offset] * dout[b][f][t].  One block per (channel f, batch row b): it walks the
// row in chunks of 1024 output times (same staging of the input window), every thread adds its 4 times x KMAX taps
// into KMAX register sums, and the block reduces ONCE at the end (wavefront shuffles, LDS, one atomic per tap) -- a
// reduction per chunk cost more than the products.
template <int KMAX, int STRIDE>
__global__ __launch_bounds__(256) void conv_cin1_wgrad_kernel(
    const float* __restrict__ x, const float* __restrict__ dout, float* __restrict__ dw, int T_in,
    int T_out, int F, int k, int stride, int offset) {
    extern __shared__ float cs[];
    __shared__ float red[4][KMAX];
    const int f = blockIdx.x, b = blockIdx.y;
    const int win = stride * 1024 + KMAX;
    float* xs = cs;
    const float* xr = x + (size_t)b * T_in;
    const float* dr = dout + ((size_t)b * F + f) * T_out;
    const int xo = stride * 4 * threadIdx.x;
    constexpr int WIN = STRIDE > 0 ? 3 * STRIDE + KMAX : 1;
    float acc[KMAX];
#pragma unroll
    for (int j = 0; j < KMAX; ++j) acc[j] = 0.0f;
    for (int tb = 0; tb < T_out; tb += 1024) {
        const int i0 = stride * tb + offset;
        __syncthreads();                                  // the previous chunk's window has been read
        for (int i = threadIdx.x; i < win; i += 256) {
            const int ti = i0 + i;
            xs[i] = (ti >= 0 && ti < T_in) ? xr[ti] : 0.0f;
        }
        __syncthreads();
        const int t0 = tb + 4 * threadIdx.x;
        float dv[4];
        if (t0 + 3 < T_out && (T_out & 3) == 0) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(dr + t0);
            dv[0] = v[0]; dv[1] = v[1]; dv[2] = v[2]; dv[3] = v[3];
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) dv[e] = (t0 + e < T_out) ? dr[t0 + e] : 0.0f;
        }
        float xw[WIN];
        if (STRIDE > 0) {
#pragma unroll
            for (int i = 0; i < WIN; ++i) xw[i] = xs[xo + i];
        }
#pragma unroll
        for (int j = 0; j < KMAX; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[j] = fmaf(STRIDE > 0 ? xw[STRIDE * e + j] : xs[xo + stride * e + j], dv[e], acc[j]);
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < KMAX; ++j) {
        float v = acc[j];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if (lane == 0) red[wid][j] = v;
    }
    __syncthreads();
    if (threadIdx.x < k) {
        const int j = threadIdx.x;
        unsafeAtomicAdd(dw + (size_t)j * F + f, red[0][j] + red[1][j] + red[2][j] + red[3][j]);
    }
}

// ----------------------------------------------------------------------------- row sums
// One wave per (b, c) row.  LPS = lanes per segment (seg/4); 0 = no segment output.
__global__ void rowsum_kernel(const float* __restrict__ x, const float* __restrict__ y,
                              float* __restrict__ seg_out, float* __restrict__ total, float alpha,
                              int rows, int C, int T, int lps) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* xr = x + (size_t)row * T;
    const float* yr = y ? y + (size_t)row * T : nullptr;
    const int nq = T >> 2;  // float4 per row
    const int nseg = lps ? nq / lps : 0;
    float tot = 0.0f;
    for (int q0 = 0; q0 < nq; q0 += 64) {
        const int q = q0 + lane;
        float s = 0.0f;
        if (q < nq) {
            f32x4 v = *reinterpret_cast<const f32x4*>(xr + 4 * q);
            if (yr) {
                const f32x4 u = *reinterpret_cast<const f32x4*>(yr + 4 * q);
                v = v * u;
            }
            s = (v[0] + v[1]) + (v[2] + v[3]);
        }
        tot += s;
        if (lps) {
            float g = s;
            for (int o = lps >> 1; o > 0; o >>= 1) g += __shfl_xor(g, o);
            if ((lane % lps) == 0 && q < nq) seg_out[(size_t)row * nseg + q / lps] = g;
        }
    }
    if (total) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) tot += __shfl_xor(tot, o);
        if (lane == 0) unsafeAtomicAdd(total + (row % C), alpha * tot);
    }
}

// general (any T, any segment length) variant: one wave per row, segments one after another
__global__ void rowsum_general_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                      float* __restrict__ seg_out, float* __restrict__ total, float alpha,
                                      int rows, int C, int T, int seg) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* xr = x + (size_t)row * T;
    const float* yr = y ? y + (size_t)row * T : nullptr;
    const int sl = seg > 0 ? seg : T;
    const int nseg = T / sl;
    float tot = 0.0f;
    for (int sgi = 0; sgi < nseg; ++sgi) {
        float s = 0.0f;
        for (int i = lane; i < sl; i += 64) {
            const int t = sgi * sl + i;
            s += yr ? xr[t] * yr[t] : xr[t];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (seg_out && lane == 0) seg_out[(size_t)row * nseg + sgi] = s;
        tot += s;
    }
    if (total && lane == 0) unsafeAtomicAdd(total + (row % C), alpha * tot);
}

// ----------------------------------------------------------------------------- MFCC (Encoder_2019)
__global__ __launch_bounds__(256) void mfcc_kernel(const float* __restrict__ x, const float* __restrict__ mel,
                                                   float* __restrict__ out, int T, int frames, int n_mel,
                                                   int n_keep, int C_out) {
    constexpr int FL = 400, STEP = 160, NB = 201;
    __shared__ float xw[FL], cs[FL], sn[FL], mag[NB + 3], lm[128];
    const int b = blockIdx.y, fr = blockIdx.x, tid = threadIdx.x;
    const float* xr = x + (size_t)b * T;
    for (int n = tid; n < FL; n += 256) {
        const int t = fr * STEP + n;
        const float w = 0.5f - 0.5f * cospif(2.0f * n / FL);            // periodic hann (tf hann_window)
        xw[n] = (t < T) ? xr[t] * w : 0.0f;                              // pad_end=True: zeros
        cs[n] = cospif(2.0f * n / FL);
        sn[n] = sinpif(2.0f * n / FL);
    }
    __syncthreads();
    if (tid < NB) {
        float re = 0.0f, im = 0.0f;
        int m = 0;                                                       // (k*n) mod FL
        for (int n = 0; n < FL; ++n) {
            re = fmaf(xw[n], cs[m], re);
            im = fmaf(xw[n], sn[m], im);
            m += tid;
            if (m >= FL) m -= FL;
        }
        mag[tid] = sqrtf(re * re + im * im);
    }
    __syncthreads();
    if (tid < n_mel) {
        float acc = 0.0f;
        for (int k = 0; k < NB; ++k) acc = fmaf(mag[k], mel[(size_t)k * n_mel + tid], acc);
        lm[tid] = logf(acc + 1e-6f);
    }
    __syncthreads();
    if (tid < C_out) {
        float v = 0.0f;
        if (tid < n_keep) {
            float acc = 0.0f;
            for (int j = 0; j < n_mel; ++j) acc = fmaf(lm[j], cospif((float)tid * (2 * j + 1) / (2.0f * n_mel)), acc);
            v = 2.0f * acc * rsqrtf(2.0f * n_mel);                       // tf dct type 2, then * rsqrt(2N)
        }
        out[((size_t)b * C_out + tid) * frames + fr] = v;
    }
}

// ----------------------------------------------------------------------------- relu/BN backward
__global__ void bn_relu_bwd_kernel(const float* __restrict__ dx, const float* __restrict__ r,
                                   const float* __restrict__ scale, float* __restrict__ dz, int C, int T,
                                   size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)((i / T) % C);
        const float v = dx[i] * scale[c];
        dz[i] = (!r || r[i] > 0.0f) ? v : 0.0f;
    }
}

// The same with the three sums the backward pass of an encoder layer needs, in ONE pass over dx (and y / r):
//   dscale[c] += sum_{b,t} dx * y   (y = the relu output, or the BN input of the last layer)
//   dbeta[c]  += sum_{b,t} dx
//   dz = dx * scale[c] * (r > 0);   dbias[c] += sum_{b,t} dz   (the conv's bias gradient, optional)
// One wave per (b, c) row, 16 bytes per lane; three atomics per row.
__global__ void bn_relu_bwd_sums_kernel(const float* __restrict__ dx, const float* __restrict__ y, const float* __restrict__ r,
                                        const float* __restrict__ scale, float* __restrict__ dz, float* __restrict__ dscale,
                                        float* __restrict__ dbeta, float* __restrict__ dbias, int rows, int C, int T) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int c = row % C;
    const float sc = scale[c];
    const size_t o = (size_t)row * T;
    float s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
    if ((T & 3) == 0) {
        for (int q = lane; q < (T >> 2); q += 64) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(dx + o + 4 * q);
            f32x4 yv = {1.f, 1.f, 1.f, 1.f}, rv = {1.f, 1.f, 1.f, 1.f}, z;
            if (y) yv = *reinterpret_cast<const f32x4*>(y + o + 4 * q);
            if (r) rv = (r == y) ? yv : *reinterpret_cast<const f32x4*>(r + o + 4 * q);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                s1 += v[e] * yv[e];
                s2 += v[e];
                z[e] = rv[e] > 0.0f ? v[e] * sc : 0.0f;
                s3 += z[e];
            }
            *reinterpret_cast<f32x4*>(dz + o + 4 * q) = z;
        }
    } else {
        for (int t = lane; t < T; t += 64) {
            const float v = dx[o + t], yv = y ? y[o + t] : 1.0f, rv = r ? r[o + t] : 1.0f;
            const float z = rv > 0.0f ? v * sc : 0.0f;
            s1 += v * yv; s2 += v; s3 += z;
            dz[o + t] = z;
        }
    }
#pragma unroll
    for (int k = 32; k > 0; k >>= 1) { s1 += __shfl_xor(s1, k); s2 += __shfl_xor(s2, k); s3 += __shfl_xor(s3, k); }
    if (lane == 0) {
        if (dscale) unsafeAtomicAdd(dscale + c, s1);
        if (dbeta) unsafeAtomicAdd(dbeta + c, s2);
        if (dbias) unsafeAtomicAdd(dbias + c, s3);
    }
}

// ----------------------------------------------------------------------------- relu/BN forward
// Second pass of a split-K encoder layer (encoder.py:15-20): x holds conv + bias; r = relu(x) is saved for the
// backward pass, x := scale[c] * r + shift[c] (BatchNorm in inference mode).
__global__ void relu_bn_fwd_kernel(float* __restrict__ x, float* __restrict__ r, const float* __restrict__ scale,
                                   const float* __restrict__ shift, int C, int T, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)((i / T) % C);
        const float v = fmaxf(x[i], 0.0f);
        if (r) r[i] = v;
        x[i] = scale ? scale[c] * v + shift[c] : v;
    }
}

// ----------------------------------------------------------------------------- transpose
__global__ void transpose_kernel(const float* __restrict__ src, float* __restrict__ dst, int rows,
                                 int cols) {
    __shared__ float tile[32][33];
    const size_t boff = (size_t)blockIdx.z * rows * cols;
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
    for (int i = ty; i < 32; i += 8) {
        const int r = r0 + i, c = c0 + tx;
        tile[i][tx] = (r < rows && c < cols) ? src[boff + (size_t)r * cols + c] : 0.0f;
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        const int c = c0 + i, r = r0 + tx;
        if (r < rows && c < cols) dst[boff + (size_t)c * rows + r] = tile[tx][i];
    }
}

// ----------------------------------------------------------------------------- softmax CE
// model.py:91-94.  Block = 4 waves x 64 consecutive time steps; wave w owns channels
// [w*Q/4, (w+1)*Q/4): every load is a 256-byte row segment.
// RANGED (vqw_softmax_xent_ranged): position (b, t) is scored iff clamp(t_begin[b], 0, T) <= t < clamp(t_end[b], 0, T) (NULL: 0 / T).
// A scored position goes through the very statements of the unranged instance (ok is the only thing that differs), so its bits
// are the same; an unscored one loads neither its logits nor its label, adds nothing to the loss and has +0.0f written to
// dlogits / probs (the backward pass reads every column of dlogits); a tile with no scored position stores its zeros and returns
// before the first load.  The unranged instance ignores t_begin / t_end and keeps its arithmetic.
template <bool RANGED>
__global__ __launch_bounds__(256) void softmax_xent_kernel(const float* __restrict__ logits,
                                                           const int32_t* __restrict__ labels,
                                                           const int32_t* __restrict__ t_begin,
                                                           const int32_t* __restrict__ t_end,
                                                           float* __restrict__ dlogits,
                                                           float* __restrict__ probs,
                                                           float* __restrict__ loss_sum,
                                                           float grad_scale, int Q, int T) {
    __shared__ float sm[4][64], ss[4][64], sl[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int ntile = (T + 63) / 64;
    const int b = blockIdx.x / ntile;
    const int t = (blockIdx.x % ntile) * 64 + lane;
    const int qn = Q / 4, q0 = w * qn;
    bool ok = t < T;
    if (RANGED) {
        const int tb = t_begin ? min(max(t_begin[b], 0), T) : 0;
        const int te = t_end ? min(max(t_end[b], 0), T) : T;
        const int tile0 = t - lane;
        const bool inb = ok;
        ok = t >= tb && t < te;                              // (te <= T: a scored position is inside the row)
        if (max(tb, tile0) >= min(te, tile0 + 64)) {         // block-uniform: nothing of this tile is scored
            if (inb && (dlogits || probs)) {
                const size_t base = ((size_t)b * Q + q0) * T + t;
                for (int q = 0; q < qn; ++q) {
                    if (probs) probs[base + (size_t)q * T] = 0.0f;
                    if (dlogits) dlogits[base + (size_t)q * T] = 0.0f;
                }
            }
            return;
        }
        if (inb && !ok && (dlogits || probs)) {              // an unscored lane of a partial tile: one write, no read
            const size_t base = ((size_t)b * Q + q0) * T + t;
            for (int q = 0; q < qn; ++q) {
                if (probs) probs[base + (size_t)q * T] = 0.0f;
                if (dlogits) dlogits[base + (size_t)q * T] = 0.0f;
            }
        }
    }
    const float* lp = logits + ((size_t)b * Q + q0) * T + t;
    const int lab = ok ? labels[(size_t)b * T + t] : 0;
    float m = -INFINITY, s = 0.0f, xl = 0.0f;
    if (ok) {
        // chunks of 16 channels: sixteen independent loads in flight, one running-max update per chunk (element by element the
        // online softmax is a dependent chain of exps behind one load each: 59 us for 109 MB = 23 % of the HBM peak in round 2)
        int q = 0;
        for (; q + 16 <= qn; q += 16) {
            float v[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) v[u] = lp[(size_t)(q + u) * T];
            float cm = v[0];
#pragma unroll
            for (int u = 1; u < 16; ++u) cm = fmaxf(cm, v[u]);
            const float mn = fmaxf(m, cm);
            float cs = 0.0f;
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                cs += __expf(v[u] - mn);
                if (q0 + q + u == lab) xl = v[u];
            }
            s = s * __expf(m - mn) + cs;
            m = mn;
        }
        for (; q < qn; ++q) {
            const float v = lp[(size_t)q * T];
            if (q0 + q == lab) xl = v;
            const float mn = fmaxf(m, v);
            s = s * __expf(m - mn) + __expf(v - mn);
            m = mn;
        }
    }
    sm[w][lane] = m; ss[w][lane] = s; sl[w][lane] = xl;
    __syncthreads();
    float M = fmaxf(fmaxf(sm[0][lane], sm[1][lane]), fmaxf(sm[2][lane], sm[3][lane]));
    float S = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) S += ss[i][lane] * __expf(sm[i][lane] - M);
    const float XL = (sl[0][lane] + sl[1][lane]) + (sl[2][lane] + sl[3][lane]);  // only one is non-zero
    if (w == 0) {
        float loss = ok ? (logf(S) + M - XL) : 0.0f;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) loss += __shfl_xor(loss, o);
        if (lane == 0 && loss_sum) unsafeAtomicAdd(loss_sum, loss);
    }
    if (ok && (dlogits || probs)) {
        const float inv = 1.0f / S;
        const size_t base = ((size_t)b * Q + q0) * T + t;
        int q = 0;
        for (; q + 16 <= qn; q += 16) {
            float v[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) v[u] = lp[(size_t)(q + u) * T];
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const float p = __expf(v[u] - M) * inv;
                if (probs) probs[base + (size_t)(q + u) * T] = p;
                if (dlogits) dlogits[base + (size_t)(q + u) * T] = (p - ((q0 + q + u == lab) ? 1.0f : 0.0f)) * grad_scale;
            }
        }
        for (; q < qn; ++q) {
            const float p = __expf(lp[(size_t)q * T] - M) * inv;
            if (probs) probs[base + (size_t)q * T] = p;
            if (dlogits) dlogits[base + (size_t)q * T] = (p - ((q0 + q == lab) ? 1.0f : 0.0f)) * grad_scale;
        }
    }
}

// ----------------------------------------------------------------------------- Adam + EMA
// model.py:116-128 with TF-1.x epsilon placement.
// SCALED: the gradient is (g * gs) * *scale, the clipping scale that vqw_grad_norm_segmented left on the device (read when the
// kernel runs); the unscaled instance is the arithmetic of a step without clipping, untouched.
template <bool SCALED>
__global__ void adam_ema_kernel(float* __restrict__ p, const float* __restrict__ g,
                                float* __restrict__ m, float* __restrict__ v,
                                float* __restrict__ ema, size_t n4, size_t n, float lr_t, float b1,
                                float b2, float eps, float decay, float gs, const int* __restrict__ skip,
                                const float* __restrict__ scale) {
    if (skip && *skip) return;          // a voided step (vqw_adam_ema_step_guarded): nothing changes
    const float sc = SCALED ? *scale : 1.0f;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4; i += stride) {
        f32x4 P = reinterpret_cast<f32x4*>(p)[i];
        f32x4 G = reinterpret_cast<const f32x4*>(g)[i] * gs;
        if (SCALED) G = G * sc;
        f32x4 Mv = reinterpret_cast<f32x4*>(m)[i];
        f32x4 Vv = reinterpret_cast<f32x4*>(v)[i];
        f32x4 E = reinterpret_cast<f32x4*>(ema)[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            Mv[e] = b1 * Mv[e] + (1.0f - b1) * G[e];
            Vv[e] = b2 * Vv[e] + (1.0f - b2) * G[e] * G[e];
            P[e] = P[e] - lr_t * Mv[e] / (sqrtf(Vv[e]) + eps);
            E[e] = E[e] - (1.0f - decay) * (E[e] - P[e]);
        }
        reinterpret_cast<f32x4*>(p)[i] = P;
        reinterpret_cast<f32x4*>(m)[i] = Mv;
        reinterpret_cast<f32x4*>(v)[i] = Vv;
        reinterpret_cast<f32x4*>(ema)[i] = E;
    }
    // tail (n not a multiple of 4)
    for (size_t i = 4 * n4 + blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += stride) {
        float G = g[i] * gs;
        if (SCALED) G = G * sc;
        const float M = b1 * m[i] + (1.0f - b1) * G;
        const float V = b2 * v[i] + (1.0f - b2) * G * G;
        const float P = p[i] - lr_t * M / (sqrtf(V) + eps);
        m[i] = M; v[i] = V; p[i] = P;
        ema[i] = ema[i] - (1.0f - decay) * (ema[i] - P);
    }
}

// ----------------------------------------------------------------------------- gradient accumulation
// out = grad (ADD false) or acc + grad (ADD true), one fp32 add per element, behind the optimiser's skip guard.  out may be acc
// or grad: every element is read at the index it is written at, before the write -- hence no __restrict__ on the three.
template <bool ADD>
__global__ void grad_accumulate_kernel(float* out, const float* acc, const float* grad, size_t n4, size_t n,
                                       const int* __restrict__ skip) {
    if (skip && *skip) return;          // a voided micro-step: the accumulator (or the flat gradient) keeps what it held
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4; i += stride) {
        f32x4 G = reinterpret_cast<const f32x4*>(grad)[i];
        if (ADD) G = reinterpret_cast<const f32x4*>(acc)[i] + G;
        reinterpret_cast<f32x4*>(out)[i] = G;
    }
    // tail (n not a multiple of 4), or everything where a pointer is not 16-byte aligned (n4 = 0)
    for (size_t i = 4 * n4 + blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += stride) {
        const float G = grad[i];
        out[i] = ADD ? acc[i] + G : G;
    }
}

inline int grid_for(size_t n, int block) {
    size_t g = (n + block - 1) / block;
    if (g > 2048) g = 2048;
    if (g < 1) g = 1;
    return (int)g;
}

}  // namespace

// ============================================================================ C ABI
extern "C" int vqw_mu_law_encode_f32(const float* x, float* y, size_t n, vqw_stream_t s) {
    if (n == 0) return 0;
    VQW_CHECK(x && y, "vqw_mu_law_encode_f32: null pointer");
    hipLaunchKernelGGL(mu_encode_f32_kernel, dim3(grid_for(n, 256)), dim3(256), 0, (hipStream_t)s, x, y, n);
    VQW_LAUNCH_CHECK("vqw_mu_law_encode_f32");
    return 0;
}

extern "C" int vqw_mu_law_encode_i32(const float* x, int32_t* y, size_t n, vqw_stream_t s) {
    if (n == 0) return 0;
    VQW_CHECK(x && y, "vqw_mu_law_encode_i32: null pointer");
    hipLaunchKernelGGL(mu_encode_i32_kernel, dim3(grid_for(n, 256)), dim3(256), 0, (hipStream_t)s, x, y, n);
    VQW_LAUNCH_CHECK("vqw_mu_law_encode_i32");
    return 0;
}

extern "C" int vqw_mu_law_decode_f32(const float* idx, float* x, size_t n, vqw_stream_t s) {
    if (n == 0) return 0;
    VQW_CHECK(idx && x, "vqw_mu_law_decode_f32: null pointer");
    hipLaunchKernelGGL(mu_decode_f32_kernel, dim3(grid_for(n, 256)), dim3(256), 0, (hipStream_t)s, idx, x, n);
    VQW_LAUNCH_CHECK("vqw_mu_law_decode_f32");
    return 0;
}

extern "C" int vqw_wavenet_inputs(const float* x, float* inputs, int32_t* labels, int B, int T, vqw_stream_t s) {
    VQW_CHECK(x && (inputs || labels), "vqw_wavenet_inputs: null pointer");
    VQW_CHECK(B > 0 && T > 0, "vqw_wavenet_inputs: bad shape");
    hipLaunchKernelGGL(wavenet_inputs_kernel, dim3(grid_for((size_t)B * T, 256)), dim3(256), 0, (hipStream_t)s, x, inputs, labels, B, T);
    VQW_LAUNCH_CHECK("vqw_wavenet_inputs");
    return 0;
}

// The same four at 256, 512 or 1024 levels.  256 runs the kernels above (the same bits as the entries without a level).
extern "C" int vqw_mu_law_encode_f32_levels(const float* x, float* y, size_t n, int levels, vqw_stream_t s) {
    VqwMu m;
    VQW_CHECK(vqw_mu_level(levels, &m), "vqw_mu_law_encode_f32_levels: levels=%d must be 256, 512 or 1024", levels);
    if (levels == 256) return vqw_mu_law_encode_f32(x, y, n, s);
    if (n == 0) return 0;
    VQW_CHECK(x && y, "vqw_mu_law_encode_f32_levels: null pointer");
    hipLaunchKernelGGL(mu_encode_f32_lv_kernel, dim3(grid_for(n, 256)), dim3(256), 0, (hipStream_t)s, x, y, n, m.mu, m.log1p_mu);
    VQW_LAUNCH_CHECK("vqw_mu_law_encode_f32_levels");
    return 0;
}

extern "C" int vqw_mu_law_encode_i32_levels(const float* x, int32_t* y, size_t n, int levels, vqw_stream_t s) {
    VqwMu m;
    VQW_CHECK(vqw_mu_level(levels, &m), "vqw_mu_law_encode_i32_levels: levels=%d must be 256, 512 or 1024", levels);
    if (levels == 256) return vqw_mu_law_encode_i32(x, y, n, s);
    if (n == 0) return 0;
    VQW_CHECK(x && y, "vqw_mu_law_encode_i32_levels: null pointer");
    if (levels == 512)
        hipLaunchKernelGGL(mu_encode_i32_lv_kernel<512>, dim3(grid_for(n, 256)), dim3(256), 0, (hipStream_t)s, x, y, n);
    else
        hipLaunchKernelGGL(mu_encode_i32_lv_kernel<1024>, dim3(grid_for(n, 256)), dim3(256), 0, (hipStream_t)s, x, y, n);
    VQW_LAUNCH_CHECK("vqw_mu_law_encode_i32_levels");
    return 0;
}

extern "C" int vqw_mu_law_decode_f32_levels(const float* idx, float* x, size_t n, int levels, vqw_stream_t s) {
    VqwMu m;
    VQW_CHECK(vqw_mu_level(levels, &m), "vqw_mu_law_decode_f32_levels: levels=%d must be 256, 512 or 1024", levels);
    if (levels == 256) return vqw_mu_law_decode_f32(idx, x, n, s);
    if (n == 0) return 0;
    VQW_CHECK(idx && x, "vqw_mu_law_decode_f32_levels: null pointer");
    hipLaunchKernelGGL(mu_decode_f32_lv_kernel, dim3(grid_for(n, 256)), dim3(256), 0, (hipStream_t)s, idx, x, n, m.mu);
    VQW_LAUNCH_CHECK("vqw_mu_law_decode_f32_levels");
    return 0;
}

extern "C" int vqw_wavenet_inputs_levels(const float* x, float* inputs, int32_t* labels, int B, int T, int levels, vqw_stream_t s) {
    VqwMu m;
    VQW_CHECK(vqw_mu_level(levels, &m), "vqw_wavenet_inputs_levels: levels=%d must be 256, 512 or 1024", levels);
    if (levels == 256) return vqw_wavenet_inputs(x, inputs, labels, B, T, s);
    VQW_CHECK(x && (inputs || labels), "vqw_wavenet_inputs_levels: null pointer");
    VQW_CHECK(B > 0 && T > 0, "vqw_wavenet_inputs_levels: bad shape");
    const dim3 grid(grid_for((size_t)B * T, 256));
    if (levels == 512)
        hipLaunchKernelGGL(wavenet_inputs_lv_kernel<512>, grid, dim3(256), 0, (hipStream_t)s, x, inputs, labels, B, T, m.mu, m.log1p_mu);
    else
        hipLaunchKernelGGL(wavenet_inputs_lv_kernel<1024>, grid, dim3(256), 0, (hipStream_t)s, x, inputs, labels, B, T, m.mu, m.log1p_mu);
    VQW_LAUNCH_CHECK("vqw_wavenet_inputs_levels");
    return 0;
}

extern "C" int vqw_conv_cin1_fwd(const float* x, const float* w, const float* bias, const float* scale,
                                 const float* shift, float* out, float* save_r, int B, int T_in,
                                 int T_out, int F, int k, int stride, int offset, int relu, vqw_stream_t s) {
    VQW_CHECK(x && w && out, "vqw_conv_cin1_fwd: null pointer");
    VQW_CHECK(B > 0 && T_in > 0 && T_out > 0 && F > 0 && k >= 1 && k <= 32 && stride >= 1, "vqw_conv_cin1_fwd: bad shape (k<=32)");
    VQW_CHECK(!scale || shift, "vqw_conv_cin1_fwd: scale needs shift");
    VQW_CHECK(stride <= 4, "vqw_conv_cin1_fwd: stride must be <= 4");
    // rows of T_out % 4 == 0 are stored 16 bytes at a time
    VQW_CHECK((T_out & 3) != 0 || ((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(save_r)) & 15u) == 0,
              "vqw_conv_cin1_fwd: out and save_r must be 16-byte aligned when T_out %% 4 == 0");
    constexpr int FT = 16;
    dim3 grid(vqw_cdiv(vqw_cdiv(T_out, 4), 256), vqw_cdiv(F, FT), B);
    typedef void (*kfn_t)(const float*, const float*, const float*, const float*, const float*, float*, float*, int, int, int, int, int, int, int);
    const int kmax = k <= 8 ? 8 : 32;
    // the model's two shapes keep their window in registers (compile-time stride); anything else goes tap by tap
    kfn_t kfn = kmax == 8 ? (stride == 2 ? conv_cin1_fwd_kernel<8, FT, 2> : (stride == 1 ? conv_cin1_fwd_kernel<8, FT, 1> : conv_cin1_fwd_kernel<8, FT, 0>))
                          : (stride == 1 ? conv_cin1_fwd_kernel<32, FT, 1> : conv_cin1_fwd_kernel<32, FT, 0>);
    hipLaunchKernelGGL(kfn, grid, dim3(256), (stride * 1024 + kmax + kmax * FT) * sizeof(float), (hipStream_t)s, x, w, bias, scale, shift, out, save_r, T_in, T_out, F, k, stride, offset, relu);
    VQW_LAUNCH_CHECK("vqw_conv_cin1_fwd");
    return 0;
}

extern "C" int vqw_conv_cin1_wgrad(const float* x, const float* dout, float* dw, int B, int T_in, int T_out,
                                   int F, int k, int stride, int offset, vqw_stream_t s) {
    VQW_CHECK(x && dout && dw, "vqw_conv_cin1_wgrad: null pointer");
    VQW_CHECK(B > 0 && T_in > 0 && T_out > 0 && F > 0 && k >= 1 && k <= 32 && stride >= 1, "vqw_conv_cin1_wgrad: bad shape (k<=32)");
    VQW_CHECK(stride <= 4, "vqw_conv_cin1_wgrad: stride must be <= 4");
    VQW_CHECK(B <= 65535, "vqw_conv_cin1_wgrad: B must be <= 65535");
    // rows of T_out % 4 == 0 are loaded 16 bytes at a time
    VQW_CHECK((T_out & 3) != 0 || (reinterpret_cast<uintptr_t>(dout) & 15u) == 0,
              "vqw_conv_cin1_wgrad: dout must be 16-byte aligned when T_out %% 4 == 0");
    dim3 grid(F, B);
    typedef void (*kfn_t)(const float*, const float*, float*, int, int, int, int, int, int);
    const int kmax = k <= 8 ? 8 : 32;
    kfn_t kfn = kmax == 8 ? (stride == 2 ? conv_cin1_wgrad_kernel<8, 2> : (stride == 1 ? conv_cin1_wgrad_kernel<8, 1> : conv_cin1_wgrad_kernel<8, 0>))
                          : (stride == 1 ? conv_cin1_wgrad_kernel<32, 1> : conv_cin1_wgrad_kernel<32, 0>);
    hipLaunchKernelGGL(kfn, grid, dim3(256), (stride * 1024 + kmax) * sizeof(float), (hipStream_t)s, x, dout, dw, T_in, T_out, F, k, stride, offset);
    VQW_LAUNCH_CHECK("vqw_conv_cin1_wgrad");
    return 0;
}

extern "C" int vqw_rowsum(const float* x, const float* y, float* seg_out, float* total, float alpha, int B,
                          int C, int T, int seg, vqw_stream_t s) {
    VQW_CHECK(x && (seg_out || total), "vqw_rowsum: null pointer");
    VQW_CHECK(B > 0 && C > 0 && T > 0, "vqw_rowsum: bad shape");
    const int rows = B * C;
    if (seg_out) VQW_CHECK(seg >= 1 && T % seg == 0, "vqw_rowsum: seg=%d must divide T=%d", seg, T);
    int lps = (seg_out && seg % 4 == 0) ? seg / 4 : 0;
    const bool aligned = (reinterpret_cast<uintptr_t>(x) & 15u) == 0 && (!y || (reinterpret_cast<uintptr_t>(y) & 15u) == 0);
    const bool fast = aligned && T % 4 == 0 && (!seg_out || (lps >= 1 && lps <= 64 && (lps & (lps - 1)) == 0));
    if (fast)
        hipLaunchKernelGGL(rowsum_kernel, dim3(vqw_cdiv(rows, 4)), dim3(256), 0, (hipStream_t)s, x, y, seg_out, total, alpha, rows, C, T, lps);
    else
        hipLaunchKernelGGL(rowsum_general_kernel, dim3(vqw_cdiv(rows, 4)), dim3(256), 0, (hipStream_t)s, x, y, seg_out, total, alpha, rows, C, T, seg_out ? seg : 0);
    VQW_LAUNCH_CHECK("vqw_rowsum");
    return 0;
}

extern "C" int vqw_mfcc(const float* x, const float* mel, float* out, int B, int T, int frames, int n_mel, int n_keep,
                        int C_out, vqw_stream_t s) {
    VQW_CHECK(x && mel && out, "vqw_mfcc: null pointer");
    VQW_CHECK(B > 0 && T > 0 && frames == (T + 159) / 160, "vqw_mfcc: frames must be ceil(T/160)");
    VQW_CHECK(n_mel >= 1 && n_mel <= 128 && n_keep >= 1 && n_keep <= n_mel && C_out >= n_keep && C_out <= 256, "vqw_mfcc: bad n_mel / n_keep / C_out");
    hipLaunchKernelGGL(mfcc_kernel, dim3(frames, B), dim3(256), 0, (hipStream_t)s, x, mel, out, T, frames, n_mel, n_keep, C_out);
    VQW_LAUNCH_CHECK("vqw_mfcc");
    return 0;
}

extern "C" int vqw_bn_relu_bwd(const float* dx, const float* r, const float* scale, float* dz, int B, int C,
                               int T, vqw_stream_t s) {
    VQW_CHECK(dx && scale && dz && B > 0 && C > 0 && T > 0, "vqw_bn_relu_bwd: bad arguments");
    const size_t n = (size_t)B * C * T;
    hipLaunchKernelGGL(bn_relu_bwd_kernel, dim3(grid_for(n, 256)), dim3(256), 0, (hipStream_t)s, dx, r, scale, dz, C, T, n);
    VQW_LAUNCH_CHECK("vqw_bn_relu_bwd");
    return 0;
}

extern "C" int vqw_bn_relu_bwd_sums(const float* dx, const float* y, const float* r, const float* scale, float* dz, float* dscale,
                                    float* dbeta, float* dbias, int B, int C, int T, vqw_stream_t s) {
    VQW_CHECK(dx && scale && dz && B > 0 && C > 0 && T > 0, "vqw_bn_relu_bwd_sums: bad arguments");
    VQW_CHECK((T & 3) != 0 || ((reinterpret_cast<uintptr_t>(dx) | reinterpret_cast<uintptr_t>(dz) | reinterpret_cast<uintptr_t>(y) |
                                reinterpret_cast<uintptr_t>(r)) & 15u) == 0, "vqw_bn_relu_bwd_sums: tensors must be 16-byte aligned");
    const int rows = B * C;
    hipLaunchKernelGGL(bn_relu_bwd_sums_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)s, dx, y, r, scale, dz, dscale, dbeta, dbias,
                       rows, C, T);
    VQW_LAUNCH_CHECK("vqw_bn_relu_bwd_sums");
    return 0;
}

extern "C" int vqw_relu_bn_fwd(float* x, float* r, const float* scale, const float* shift, int B, int C, int T,
                               vqw_stream_t s) {
    VQW_CHECK(x && B > 0 && C > 0 && T > 0 && (!scale || shift), "vqw_relu_bn_fwd: bad arguments");
    const size_t n = (size_t)B * C * T;
    hipLaunchKernelGGL(relu_bn_fwd_kernel, dim3(grid_for(n, 256)), dim3(256), 0, (hipStream_t)s, x, r, scale, shift, C, T, n);
    VQW_LAUNCH_CHECK("vqw_relu_bn_fwd");
    return 0;
}

extern "C" int vqw_transpose(const float* src, float* dst, int batch, int rows, int cols, vqw_stream_t s) {
    VQW_CHECK(src && dst && batch > 0 && rows > 0 && cols > 0, "vqw_transpose: bad arguments");
    dim3 grid(vqw_cdiv(cols, 32), vqw_cdiv(rows, 32), batch);
    hipLaunchKernelGGL(transpose_kernel, grid, dim3(256), 0, (hipStream_t)s, src, dst, rows, cols);
    VQW_LAUNCH_CHECK("vqw_transpose");
    return 0;
}

extern "C" int vqw_softmax_xent(const float* logits, const int32_t* labels, float* dlogits, float* probs,
                                float* loss_sum, float grad_scale, int B, int Q, int T, vqw_stream_t s) {
    VQW_CHECK(logits && labels && loss_sum, "vqw_softmax_xent: null pointer");
    VQW_CHECK(B > 0 && T > 0 && Q >= 4 && Q % 4 == 0, "vqw_softmax_xent: Q=%d must be a multiple of 4", Q);
    hipLaunchKernelGGL(softmax_xent_kernel<false>, dim3(B * vqw_cdiv(T, 64)), dim3(256), 0, (hipStream_t)s, logits, labels, (const int32_t*)nullptr,
                       (const int32_t*)nullptr, dlogits, probs, loss_sum, grad_scale, Q, T);
    VQW_LAUNCH_CHECK("vqw_softmax_xent");
    return 0;
}

// The loss of a length-masked training step: vqw_softmax_xent over t_begin[b] <= t < t_end[b] alone, zeros elsewhere.
extern "C" int vqw_softmax_xent_ranged(const float* logits, const int32_t* labels, const int32_t* t_begin, const int32_t* t_end,
                                       float* dlogits, float* probs, float* loss_sum, float grad_scale, int B, int Q, int T,
                                       vqw_stream_t s) {
    VQW_CHECK(logits && labels && loss_sum, "vqw_softmax_xent_ranged: null pointer");
    VQW_CHECK(B > 0 && T > 0 && Q >= 4 && Q % 4 == 0, "vqw_softmax_xent_ranged: Q=%d must be a multiple of 4", Q);
    hipLaunchKernelGGL(softmax_xent_kernel<true>, dim3(B * vqw_cdiv(T, 64)), dim3(256), 0, (hipStream_t)s, logits, labels, t_begin, t_end,
                       dlogits, probs, loss_sum, grad_scale, Q, T);
    VQW_LAUNCH_CHECK("vqw_softmax_xent_ranged");
    return 0;
}

// The two entries SURVEY 8(b) names, over the same kernel: forward = the loss sum (+ the probabilities), backward = the gradient
// seed (softmax - onehot) * grad_scale, recomputed from the logits (may be written in place over them).
extern "C" int vqw_softmax_xent_fwd(const float* logits, const int32_t* labels, float* probs, float* loss_sum, int B, int Q, int T,
                                    vqw_stream_t s) {
    VQW_CHECK(logits && labels && loss_sum, "vqw_softmax_xent_fwd: null pointer");
    VQW_CHECK(B > 0 && T > 0 && Q >= 4 && Q % 4 == 0, "vqw_softmax_xent_fwd: Q=%d must be a multiple of 4", Q);
    hipLaunchKernelGGL(softmax_xent_kernel<false>, dim3(B * vqw_cdiv(T, 64)), dim3(256), 0, (hipStream_t)s, logits, labels, (const int32_t*)nullptr,
                       (const int32_t*)nullptr, (float*)nullptr, probs,
                       loss_sum, 0.0f, Q, T);
    VQW_LAUNCH_CHECK("vqw_softmax_xent_fwd");
    return 0;
}

extern "C" int vqw_softmax_xent_bwd(const float* logits, const int32_t* labels, float* dlogits, float grad_scale, int B, int Q, int T,
                                    vqw_stream_t s) {
    VQW_CHECK(logits && labels && dlogits, "vqw_softmax_xent_bwd: null pointer");
    VQW_CHECK(B > 0 && T > 0 && Q >= 4 && Q % 4 == 0, "vqw_softmax_xent_bwd: Q=%d must be a multiple of 4", Q);
    hipLaunchKernelGGL(softmax_xent_kernel<false>, dim3(B * vqw_cdiv(T, 64)), dim3(256), 0, (hipStream_t)s, logits, labels, (const int32_t*)nullptr,
                       (const int32_t*)nullptr, dlogits, (float*)nullptr,
                       (float*)nullptr, grad_scale, Q, T);
    VQW_LAUNCH_CHECK("vqw_softmax_xent_bwd");
    return 0;
}

extern "C" int vqw_adam_ema_step_scaled(float* param, const float* grad, float* m, float* v, float* ema, size_t n,
                                        float lr_t, float beta1, float beta2, float eps, float decay,
                                        float grad_scale, const int32_t* skip, const float* scale, vqw_stream_t s) {
    VQW_CHECK(param && grad && m && v && ema, "vqw_adam_ema_step: null pointer");
    if (n == 0) return 0;
    const uintptr_t al = reinterpret_cast<uintptr_t>(param) | reinterpret_cast<uintptr_t>(grad) |
                         reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v) |
                         reinterpret_cast<uintptr_t>(ema);
    const size_t n4 = (al & 15u) ? 0 : n / 4;
    hipLaunchKernelGGL(scale ? adam_ema_kernel<true> : adam_ema_kernel<false>, dim3(grid_for(n4 ? n4 : n, 256)), dim3(256), 0, (hipStream_t)s,
                       param, grad, m, v, ema, n4, n, lr_t, beta1, beta2, eps, decay, grad_scale, skip, scale);
    VQW_LAUNCH_CHECK("vqw_adam_ema_step");
    return 0;
}

extern "C" int vqw_grad_accumulate(float* out, const float* acc, const float* grad, size_t n, const int32_t* skip, vqw_stream_t s) {
    if (n == 0) return 0;
    VQW_CHECK(out && grad, "vqw_grad_accumulate: null pointer");
    const uintptr_t al = reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(grad) | reinterpret_cast<uintptr_t>(acc);   // (acc NULL: no bits)
    VQW_CHECK((al & 3u) == 0, "vqw_grad_accumulate: pointers must be 4-byte aligned");
    const size_t n4 = (al & 15u) ? 0 : n / 4;
    hipLaunchKernelGGL(acc ? grad_accumulate_kernel<true> : grad_accumulate_kernel<false>, dim3(grid_for(n4 ? n4 : n, 256)), dim3(256), 0,
                       (hipStream_t)s, out, acc, grad, n4, n, skip);
    VQW_LAUNCH_CHECK("vqw_grad_accumulate");
    return 0;
}

extern "C" int vqw_adam_ema_step_guarded(float* param, const float* grad, float* m, float* v, float* ema, size_t n,
                                         float lr_t, float beta1, float beta2, float eps, float decay,
                                         float grad_scale, const int32_t* skip, vqw_stream_t s) {
    return vqw_adam_ema_step_scaled(param, grad, m, v, ema, n, lr_t, beta1, beta2, eps, decay, grad_scale, skip, nullptr, s);
}

extern "C" int vqw_adam_ema_step(float* param, const float* grad, float* m, float* v, float* ema, size_t n,
                                 float lr_t, float beta1, float beta2, float eps, float decay,
                                 float grad_scale, vqw_stream_t s) {
    return vqw_adam_ema_step_guarded(param, grad, m, v, ema, n, lr_t, beta1, beta2, eps, decay, grad_scale, nullptr, s);
}
