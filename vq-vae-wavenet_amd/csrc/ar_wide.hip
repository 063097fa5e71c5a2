// The wide generator: autoregressive WaveNet generation for MANY rows at once (tens to 1024), the third back end beside
// the persistent kernel (ar_persist.hip) and the launch-per-phase path (ar_decode.hip), which stream the weights through
// matrix-vector products and hold at most 8 rows.  Rows never interact (generate.py:40,103-113), so with B rows every layer
// of a step is a GEMM  out[N][B] = W^T[N][ks R] x state[ks R][B]  on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32, the
// instruction conv_gemm.hip uses): the weights are read once per step, not once per row.
//
// State is channel-major with the batch row innermost: cur [R][B], gated [R][B], skip [S][B], h [S][B], logits [Q][B], per
// layer a ring [(ks-1) d][R][B] whose slot is one contiguous [R][B] tile, the input history [pre_k][B].  A row is a GEMM column.
//
// One GEMM kernel with the three epilogues of ar_gemv_kernel (same formulas, same order).  A workgroup owns one 32-row x
// 32-column output tile (MODE_GATE: the filter and the gate tile of the same 32 channels).  Its 4 waves each take one
// quarter of the concatenated K range [0, nseg K) as ONE k-ordered MFMA chain (bit for bit an fmaf chain from zero), and
// the four partial tiles are added in LDS as ((p0 + p1) + p2) + p3.  The order of an output element's sum therefore depends
// on K alone: not on B, not on the column's place in its tile, not on the other columns.  A column past B - 1 of a partial
// tile loads column B - 1 again (nothing is read past it) and is not stored.
//
// The condition projections are computed by the same kernel for a window of AR_WIDE_WINDOW frames at a time, into
// condwin [frames][Mall][B]; the host refreshes the window in stream order when a run reaches its end (ar_wide_plan.h).
//
// A step is one linear chain of ordinary launches on the handle's private stream, captured once into a hipGraph: no kernel
// waits for another, nothing spins.  The step counter lives on the device; the last workgroup of the sampling kernel to
// finish (a ticket, never waited for) advances it.
//
// Code-input mode (vqw_ar_wide_prior_create: the latent prior over VQ codes).  The prior is the same stack, so the GEMMs,
// the rings, the condition window and the step graph are shared; only the two ends of a step differ: arw_pre_code_kernel
// gathers rows of W_pre by the previous codes where arw_pre_kernel convolves a mu-law sample, and arw_sample_kernel<true>
// feeds the drawn index itself back as the next input.
#include <string.h>

#include "ar_host.h"
#include "ar_sampling.h"
#include "ar_wide_plan.h"

namespace {

constexpr int WIDE_MAXB = 1024;
constexpr int TILE = 32;          // rows and columns of a workgroup's output tile (one 32x32 MFMA tile per wave and K quarter)

struct WideState {  // device resident
    int step;       // samples generated since reset
    int run_base;   // value of step when the current run started
    int win_f0;     // first condition frame held by condwin
    int ticket;     // sampling workgroups that have finished this step
    int Tz, ratio, mode, n_steps;
    const float* uniforms;
    float* audio;
    int* indices;
    float* probs_last;
};

struct WideSeg {
    const float* w;  // [K][ldw]
    const float* x;  // [K][B] (plain) or ring base [depth][K][B]
    int depth;       // 0 = plain
    int phase;       // ring slot = (step + phase) % depth
};

enum { MODE_PLAIN = 0, MODE_GATE = 1, MODE_OUT = 2 };

struct WideArgs {
    WideSeg seg[VQW_MAX_TAPS];
    int nseg, K, ldw, B, N, H, S;   // K per segment; N total rows; H gate half; S skip width (MODE_OUT)
    int in_relu;
    const float* bias;
    const float* cond;              // condwin + row offset * B, or null
    long long cond_fstride;         // Mall * B
    int cond_frames;                // frames condwin holds
    float* out;                     // PLAIN: [N][B]; GATE: gated [H][B]; OUT: skip [S][B]
    float* cur;                     // OUT: [N-S][B] residual state (in place)
    float* ring_w;                  // OUT: ring of this layer [depth][N-S][B]
    int ring_depth;
    long long x_zstride, out_zstride;   // per blockIdx.z (the frames of a condition refresh)
    const WideState* st;
};

// wavenet.py:113-124: x = mu_law_encode(input_t); fast_conv1d(k=pre_k, dilation 1, Cin=1), every row in one launch.
// Block: 64 rows x 32 channels; xhist [pre_k][B], slot tau % pre_k holds the input of step tau.
__global__ __launch_bounds__(256) void arw_pre_kernel(const WideState* st, const float* prev, float* xhist, const float* pre_w,
                                                      const float* pre_b, float* cur, int pre_k, int R, int B, const VqwMu mu) {
    __shared__ float taps[64][64];
    const int tb = threadIdx.x & 63, tg = threadIdx.x >> 6;
    const int b = blockIdx.x * 64 + tb;
    const int step = st->step;
    if (b < B) {
        for (int j = tg; j < pre_k; j += 4) {               // tap j multiplies x(t - (pre_k-1-j))
            float v;
            if (j == pre_k - 1) {
                v = vqw_mu_encode_m(prev[b], mu);
                if (blockIdx.y == 0) xhist[(size_t)(step % pre_k) * B + b] = v;   // the slot of t - pre_k: no tap reads it
            } else {
                const int tau = step - (pre_k - 1 - j);
                v = xhist[(size_t)(((tau % pre_k) + pre_k) % pre_k) * B + b];
            }
            taps[j][tb] = v;
        }
    }
    __syncthreads();
    if (b >= B) return;
    for (int i = 0; i < 8; ++i) {
        const int o = blockIdx.y * 32 + tg * 8 + i;
        float acc = pre_b[o];
        for (int j = 0; j < pre_k; ++j) acc = fmaf(pre_w[(size_t)j * R + o], taps[j][tb], acc);
        cur[(size_t)o * B + b] = acc;
    }
}

// Code-input mode (the latent prior, prior.py): the input of step t is the code drawn at step t - 1, a one-hot, so the
// preprocess conv is a gather:  cur[o][b] = b_pre[o] + sum_j W_pre[j][c_j][o],  c_j = row b's code at step t - (pre_k - j),
// W_pre [pre_k][n_codes][R].  Start from the bias, taps in ascending j, one fp32 add per tap that has a code; a step before
// 0 has none (a zero one-hot, not code 0) and adds nothing.  xhist / prev hold code + 1 as floats (exact up to 1024), 0 =
// no code: the persistent kernel's convention, so the zeros of a reset mean "no code yet".  Same block and grid as
// arw_pre_kernel.  A gathered row segment (32 channels) is 128 contiguous bytes: the gather runs with the lanes along the
// channel, two rows per wave; cur has b innermost: the store runs with the lanes along b (256-byte segments); the tile is
// transposed through LDS in between (vqw_prior_input_fwd does the same for the training pass).  Rows of 33 floats (banks are
// dword address mod 32 per 32-lane half): a half of the gather phase writes one row, 33 r + o with o along the lanes, 32
// consecutive banks; a half of the store phase reads one column, 33 r + o with r along the lanes, bank (r + o) mod 32, every
// bank once: neither phase conflicts.  Rows past B - 1 are neither gathered nor stored.
__global__ __launch_bounds__(256) void arw_pre_code_kernel(const WideState* st, const float* prev, float* xhist, const float* pre_w,
                                                           const float* pre_b, float* cur, int pre_k, int n_codes, int R, int B) {
    __shared__ int codes[64][64];       // [tap][row]: the code, or -1 for none
    __shared__ float tile[64][33];      // [row][channel]
    const int tb = threadIdx.x & 63, tg = threadIdx.x >> 6;
    const int b = blockIdx.x * 64 + tb;
    const int step = st->step;
    if (b < B) {
        for (int j = tg; j < pre_k; j += 4) {               // tap j meets the input of step t - (pre_k-1-j)
            float v;
            if (j == pre_k - 1) {
                v = prev[b];                                 // the code drawn at the previous step (+ 1)
                if (blockIdx.y == 0) xhist[(size_t)(step % pre_k) * B + b] = v;   // the slot of t - pre_k: no tap reads it
            } else {
                const int tau = step - (pre_k - 1 - j);
                v = xhist[(size_t)(((tau % pre_k) + pre_k) % pre_k) * B + b];
            }
            const int code = (int)v - 1;
            codes[j][tb] = code < n_codes ? code : -1;
        }
    }
    __syncthreads();
    const int o = threadIdx.x & 31, rh = (threadIdx.x >> 5) & 1;
    const float* wcol = pre_w + blockIdx.y * 32 + o;
    const float bias = pre_b[blockIdx.y * 32 + o];
    for (int i = 0; i < 8; ++i) {
        const int r = 8 * i + 2 * tg + rh;                  // wave tg gathers rows 2 tg, 2 tg + 1 of every group of 8
        if (blockIdx.x * 64 + r >= B) continue;
        float acc = bias;
        for (int j = 0; j < pre_k; ++j) {
            const int code = codes[j][r];
            if (code >= 0) acc += wcol[((size_t)j * n_codes + code) * R];
        }
        tile[r][o] = acc;
    }
    __syncthreads();
    if (b >= B) return;
    for (int i = 0; i < 8; ++i) {
        const int oc = tg * 8 + i;
        cur[(size_t)(blockIdx.y * 32 + oc) * B + b] = tile[tb][oc];
    }
}

// out[n][b] = sum_seg sum_k w[k][n] x[k][b]  (+bias +cond), see the head of the file.  grid (rows/32, ceil(B/32), frames).
template <int MODE>
__global__ __launch_bounds__(256) void arw_gemm_kernel(const WideArgs a) {
    constexpr int MT = (MODE == MODE_GATE) ? 2 : 1;
    __shared__ float red[4][MT][16][64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int c = lane & 31, half = lane >> 5;
    const int step = a.st->step;
    const int B = a.B;
    const int n0 = blockIdx.x * TILE, b0 = blockIdx.y * TILE;   // row tiles fastest: the column tiles of one row tile share an XCD's L2
    constexpr int U = 16;                                        // k-pairs per batch of operand loads
    const int bl = min(b0 + c, B - 1);                      // a column past the batch re-reads the last row's
    const size_t xz = (size_t)blockIdx.z * a.x_zstride;

    f32x16 acc[MT];
#pragma unroll
    for (int e = 0; e < MT; ++e)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[e][r] = 0.0f;

    // this wave's quarter [k_lo, k_hi) of the concatenated K range, segment by segment in ascending k
    const int K = a.K;
    const int Kq = a.nseg * K / 4;
    const int k_lo = wv * Kq, k_hi = k_lo + Kq;
    for (int sgi = 0; sgi < a.nseg; ++sgi) {
        const int s_lo = max(k_lo - sgi * K, 0), s_hi = min(k_hi - sgi * K, K);
        if (s_lo >= s_hi) continue;
        const WideSeg sg = a.seg[sgi];
        const float* xp = sg.x + xz;
        if (sg.depth > 0) xp += (size_t)((step + sg.phase) % sg.depth) * K * B;
        xp += (size_t)(s_lo + half) * B + bl;
        const float* wp = sg.w + (size_t)(s_lo + half) * a.ldw + n0 + c;
        // lane l supplies A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31].  The chain is bound by the latency of
        // its operand loads, not by the MFMAs: batches of U k-pairs, the loads of the next batch issued before the MFMAs
        // of this one.  The MFMAs stay in ascending k whatever the batching.
        const size_t xs = 2 * (size_t)B, wst = 2 * (size_t)a.ldw;
        float wa[2][U], wb[2][U], xv[2][U];
        auto load = [&](int p) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                wa[p][u] = wp[u * wst];
                if constexpr (MT == 2) wb[p][u] = wp[u * wst + a.H];
                xv[p][u] = xp[u * xs];
            }
            wp += U * wst;
            xp += U * xs;
        };
        auto mma = [&](int p) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const float x = a.in_relu ? fmaxf(xv[p][u], 0.0f) : xv[p][u];
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[p][u], x, acc[0], 0, 0, 0);
                if constexpr (MT == 2) acc[MT - 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(wb[p][u], x, acc[MT - 1], 0, 0, 0);
            }
        };
        const int nb = (s_hi - s_lo) / (2 * U);
        if (nb > 0) load(0);
        for (int i = 0; i < nb; i += 2) {
            if (i + 1 < nb) load(1);
            mma(0);
            if (i + 2 < nb) load(0);
            if (i + 1 < nb) mma(1);
        }
        for (int k = s_lo + nb * 2 * U; k < s_hi; k += 2) {
            float x = *xp;
            if (a.in_relu) x = fmaxf(x, 0.0f);
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(wp[0], x, acc[0], 0, 0, 0);
            if constexpr (MT == 2) acc[MT - 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(wp[a.H], x, acc[MT - 1], 0, 0, 0);
            xp += xs;
            wp += wst;
        }
    }
#pragma unroll
    for (int e = 0; e < MT; ++e)
#pragma unroll
        for (int r = 0; r < 16; ++r) red[wv][e][r][lane] = acc[e][r];
    __syncthreads();

    // wave w finishes accumulator registers 4w .. 4w+3: C/D row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5), column = lane & 31
    const int b = b0 + c;
    const bool ok = b < B;
    int frame = 0;
    if (a.cond) {
        frame = step / a.st->ratio;
        if (frame >= a.st->Tz) frame = a.st->Tz - 1;
        frame = min(max(frame - a.st->win_f0, 0), a.cond_frames - 1);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int reg = 4 * wv + i;
        const int n = n0 + i + 8 * wv + 4 * half;
        float v[MT];
#pragma unroll
        for (int e = 0; e < MT; ++e) {
            v[e] = ((red[0][e][reg][lane] + red[1][e][reg][lane]) + red[2][e][reg][lane]) + red[3][e][reg][lane];
            const int ne = n + e * a.H;
            if (a.bias) v[e] += a.bias[ne];
            if (a.cond) v[e] += a.cond[(size_t)frame * a.cond_fstride + (size_t)ne * B + (ok ? b : B - 1)];
        }
        if (!ok) continue;
        if (MODE == MODE_GATE) {
            const float vf = v[0], vg = v[MT - 1];
            const float th = 1.0f - 2.0f / (__expf(2.0f * vf) + 1.0f);
            const float sg = 1.0f / (1.0f + __expf(-vg));
            a.out[(size_t)n * B + b] = th * sg;
        } else if (MODE == MODE_OUT) {
            if (n < a.S) {
                a.out[(size_t)n * B + b] += v[0];           // skip += skip_out   (wavenet.py:142)
            } else {
                const int R = a.N - a.S, r = n - a.S;
                const float old = a.cur[(size_t)r * B + b];
                if (a.ring_w) a.ring_w[((size_t)(step % a.ring_depth) * R + r) * B + b] = old;   // push
                a.cur[(size_t)r * B + b] = old + v[0];      // current += res_out (wavenet.py:143)
            }
        } else {
            a.out[(size_t)blockIdx.z * a.out_zstride + (size_t)n * B + b] = v[0];
        }
    }
}

// The encoding of the window's frames, transposed for the GEMM: enct[f][c][b] = enc[b][c][f0 + f]; records the window.
__global__ void arw_window_kernel(WideState* st, const float* __restrict__ enc, float* enct, int B, int Cc, int Tz, int f0, int nf) {
    const size_t n = (size_t)nf * Cc * B;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int b = (int)(i % B);
        const size_t fc = i / B;
        const int cc = (int)(fc % Cc), f = (int)(fc / Cc);
        enct[i] = enc[((size_t)b * Cc + cc) * Tz + f0 + f];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) st->win_f0 = f0;
}

// softmax (wavenet.py:171) + utils.decode (utils.py:30-46) + mu_law_decode_np of ONE row per workgroup; logits [Q][B].
// A default row: ar_sample_default (softmax with the maximum subtracted, a sequential fp32 cumsum, searchsorted left; greedy =
// the lowest index among the maxima); p is written on the last step of a run only.  A row with settings:
// ar_sample_truncated, by wave 0.
// CODE (the latent prior's handles): the same decision over Q = n_codes classes; the index itself is the next input
// (prev = idx + 1, arw_pre_code_kernel), there is no mu-law decode, and audio (NULL on these handles) is skipped.  u above
// the last cdf value gives Q, which is no code: it is clamped to Q - 1.
template <bool CODE>
__global__ __launch_bounds__(256) void arw_sample_kernel(WideState* st, const float* logits, const ArSampleRow* samp, float* prev,
                                                         int B, int Q, const VqwMu mu) {
    __shared__ float sp[1024];
    __shared__ float redv[4];
    __shared__ int redi[4];
    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    const int step = st->step;
    const int n_steps = st->n_steps;
    const int i_out = step - st->run_base;
    const bool last = i_out == n_steps - 1;
    float* const pl = (last && st->probs_last) ? st->probs_last + (size_t)b * Q : nullptr;
    int idx = 0;
    const ArSampleRow row = samp[b];
    if (row.on) {                          // block-uniform; wave 0 samples the row (ar_sampling.h)
        for (int q = tid; q < Q; q += 256) sp[q] = logits[(size_t)q * B + b];
        __syncthreads();
        if (tid >= 64) return;
        idx = ar_sample_truncated(sp, Q, row, st->uniforms[(size_t)b * n_steps + i_out], pl);
    } else {
        const int mode = st->mode;
        idx = ar_sample_default(logits + b, B, sp, redv, redi, Q, mode, mode ? st->uniforms + (size_t)b * n_steps + i_out : nullptr,
                                pl, nullptr);
        if (tid != 0) return;
        if (mode != 0) idx = min(idx, Q - 1);
    }
    if (tid == 0) {
        if constexpr (CODE) {
            idx = min(idx, Q - 1);
            if (st->audio) st->audio[(size_t)b * n_steps + i_out] = (float)idx;
            st->indices[(size_t)b * n_steps + i_out] = idx;
            prev[b] = (float)(idx + 1);
        } else {
            const float dec = vqw_mu_decode_m((float)idx, mu);
            st->audio[(size_t)b * n_steps + i_out] = dec;
            if (st->indices) st->indices[(size_t)b * n_steps + i_out] = idx;
            prev[b] = dec;
        }
        // every workgroup read `step` before it took its ticket, so the last one may advance it; nobody waits for this
        if (atomicAdd(&st->ticket, 1) == B - 1) {
            st->ticket = 0;
            st->step = step + 1;
        }
    }
}

// Prefill (vqw_ar_wide_prefill_layer): layer inputs of a prompt into the layer's ring.  The source x [nrows][R][ld] is
// contiguous along time, the ring [depth][R][B] along the batch row, with R between them in both: a tile of 32 rows x 32 steps
// of ONE channel is transposed through LDS.  grid (step tiles, row tiles, R).  Loads run with the lanes along time (a half
// wave reads 128 contiguous bytes of one row), stores with the lanes along the batch row (a half wave writes 128 contiguous
// bytes of one slot once the chunk has 32 rows).  Rows of 33 floats, as in arw_pre_code_kernel: a half of the load phase
// writes one LDS row (32 consecutive banks), a half of the store phase reads one column (bank (row + step) mod 32, every bank
// once).  A partial tile neither loads nor stores past its rows or steps (arw_tile_extent).  A copy: no arithmetic touches
// a value.  Step t_lo + s goes to slot arw_ring_slot: where MODE_OUT pushes the layer's input of that step.
__global__ __launch_bounds__(256) void arw_prefill_scatter_kernel(float* ring, int depth, int R, int B, const float* __restrict__ x,
                                                                  int ld, int t_first, int t_lo, int nt, int row0, int nrows) {
    constexpr int PT = AR_WIDE_PREFILL_TILE;
    __shared__ float tile[PT][PT + 1];      // [row][step]
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int r = blockIdx.z;
    const int s0 = blockIdx.x * PT, i0 = blockIdx.y * PT;
    const int ns = arw_tile_extent(nt, blockIdx.x), ni = arw_tile_extent(nrows, blockIdx.y);
    if (tx < ns) {
        const float* src = x + ((size_t)i0 * R + r) * ld + (t_lo - t_first) + s0 + tx;
        for (int i = ty; i < ni; i += 8) tile[i][tx] = src[(size_t)i * R * ld];
    }
    __syncthreads();
    if (tx < ni) {
        for (int s = ty; s < ns; s += 8) {
            const int slot = arw_ring_slot(t_lo + s0 + s, depth);
            ring[((size_t)slot * R + r) * B + row0 + i0 + tx] = tile[tx][s];
        }
    }
}

// Prefill (vqw_ar_wide_prefill_finish): what the input kernels and the sampling kernel leave after step t_end - 1.  xhist slot
// tau % pre_k holds the input of step tau for tau in (t_end - pre_k, t_end), tau >= 0: for tau >= 1 the value of the prompt at
// tau - 1 = tail[b][tau - 1 - (t_end - pre_k)] (mu-law encoded at the handle's level, or code + 1), for tau = 0 what step 0
// stores from the reset's prev = 0 (mu_law_encode(0), or 0 = no code).  The slot of step t_end - pre_k (whose value, for
// t_end > pre_k, lies before the tail) is the one step t_end overwrites before any tap reads it: it keeps the reset's zero.
// prev is the prompt's last value, step the counter.  One thread per (slot, row), the row innermost.
__global__ __launch_bounds__(256) void arw_prefill_finish_kernel(WideState* st, float* prev, float* xhist, int B, int pre_k, int t_end,
                                                                 const float* audio_tail, const int* code_tail, const VqwMu mu) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) st->step = t_end;
    if (i >= B * pre_k) return;
    const int j = i / B, b = i - j * B;                  // tail column j is the prompt's value at t_end - pre_k + j
    const size_t at = (size_t)b * pre_k + j;
    const int tau = t_end - pre_k + j + 1;               // the step whose input that value is
    if (tau >= 1 && tau < t_end)
        xhist[(size_t)(tau % pre_k) * B + b] = audio_tail ? vqw_mu_encode_m(audio_tail[at], mu) : (float)(code_tail[at] + 1);
    if (j == pre_k - 1) {
        prev[b] = audio_tail ? audio_tail[at] : (float)(code_tail[at] + 1);
        if (t_end <= pre_k) xhist[b] = audio_tail ? vqw_mu_encode_m(0.0f, mu) : 0.0f;   // the input of step 0, slot 0
    }
}

}  // namespace

struct vqw_ar_wide : ArTables {
    int B = 0, Mall = 0;
    int n_codes = 0;                 // > 0: code-input mode (vqw_ar_wide_prior_create): w.pre_w is [pre_k][n_codes][R], read in place
    long long steps = 0;             // host mirror of the device step counter (reset: 0; a run adds n_steps)
    WideState* st = nullptr;
    ArSampleRow* samp = nullptr;     // device [B]
    std::vector<ArSampleRow> samp_host;
    float *prev = nullptr, *xhist = nullptr, *cur = nullptr, *gated = nullptr, *skip = nullptr, *h = nullptr,
          *logits = nullptr, *enct = nullptr, *condwin = nullptr;
    std::vector<float*> rings;       // per layer [depth][R][B]
    hipStream_t stream = nullptr;    // private stream (graph capture is illegal on the null stream)
    hipEvent_t ev_in = nullptr;
    ArGraph step;                    // launch_step, captured
    bool pending = false;
    VqwMu mu = {256, 255.0f, 5.5451774444795623f};   // the mu-law level of an audio handle (vqw_ar_wide_set_levels)
};

namespace {

WideArgs base_args(const vqw_ar_wide* h) {
    WideArgs a;
    memset(&a, 0, sizeof(a));
    a.B = h->B;
    a.st = h->st;
    a.cond_fstride = (long long)h->Mall * h->B;
    a.cond_frames = AR_WIDE_WINDOW;
    return a;
}

template <int MODE>
void launch_gemm(const WideArgs& a, int rows, int frames, hipStream_t st) {
    hipLaunchKernelGGL((arw_gemm_kernel<MODE>), dim3(rows / TILE, vqw_cdiv(a.B, TILE), frames), dim3(256), 0, st, a);
}

int launch_step(vqw_ar_wide* h, hipStream_t st) {
    const vqw_ar_weights& w = h->w;
    const int B = h->B, R = w.R, S = w.S, Q = w.Q, ks = w.kernel_size, L = w.n_layers;
    if (h->n_codes)
        hipLaunchKernelGGL(arw_pre_code_kernel, dim3(vqw_cdiv(B, 64), R / 32), dim3(256), 0, st, h->st, h->prev, h->xhist, w.pre_w,
                           w.pre_b, h->cur, w.pre_k, h->n_codes, R, B);
    else
        hipLaunchKernelGGL(arw_pre_kernel, dim3(vqw_cdiv(B, 64), R / 32), dim3(256), 0, st, h->st, h->prev, h->xhist, w.pre_w, w.pre_b,
                           h->cur, w.pre_k, R, B, h->mu);
    // skip = linear(current)  (wavenet.py:127-128)
    WideArgs a = base_args(h);
    a.seg[0] = WideSeg{w.skip0_w, h->cur, 0, 0};
    a.nseg = 1; a.K = R; a.ldw = S; a.N = S; a.bias = w.skip0_b; a.out = h->skip;
    launch_gemm<MODE_PLAIN>(a, S, 1, st);
    for (int l = 0; l < L; ++l) {
        const int d = h->dil[l];
        const int depth = (ks - 1) * d;
        // fast_gated_cnn (wavenet_ops.py:212-237)
        a = base_args(h);
        for (int j = 0; j < ks; ++j) {
            const float* wt = h->gated_w[l] + (size_t)j * R * 2 * R;
            if (j == ks - 1) a.seg[j] = WideSeg{wt, h->cur, 0, 0};
            else a.seg[j] = WideSeg{wt, h->rings[l], depth, j * d};   // x(t-(ks-1-j)d)
        }
        a.nseg = ks; a.K = R; a.ldw = 2 * R; a.N = 2 * R; a.H = R; a.bias = h->gated_b[l];
        a.cond = h->condwin + (size_t)l * 2 * R * B; a.out = h->gated;
        launch_gemm<MODE_GATE>(a, R, 1, st);
        // skip / residual linears + accumulation + queue push (wavenet_ops.py:261-265, wavenet.py:142-143)
        a = base_args(h);
        a.seg[0] = WideSeg{h->out_w[l], h->gated, 0, 0};
        a.nseg = 1; a.K = R; a.ldw = w.out_ld; a.N = S + R; a.S = S; a.bias = h->out_b[l];
        a.out = h->skip; a.cur = h->cur; a.ring_w = h->rings[l]; a.ring_depth = depth;
        launch_gemm<MODE_OUT>(a, S + R, 1, st);
    }
    // postprocess1 (wavenet.py:152-162)
    a = base_args(h);
    a.seg[0] = WideSeg{w.post1_w, h->skip, 0, 0};
    a.nseg = 1; a.K = S; a.ldw = S; a.N = S; a.in_relu = 1; a.bias = w.post1_b;
    a.cond = h->condwin + (size_t)L * 2 * R * B; a.out = h->h;
    launch_gemm<MODE_PLAIN>(a, S, 1, st);
    // postprocess2 (wavenet.py:165-167)
    a = base_args(h);
    a.seg[0] = WideSeg{w.post2_w, h->h, 0, 0};
    a.nseg = 1; a.K = S; a.ldw = Q; a.N = Q; a.in_relu = 1; a.bias = w.post2_b; a.out = h->logits;
    launch_gemm<MODE_PLAIN>(a, Q, 1, st);
    if (h->n_codes)
        hipLaunchKernelGGL(arw_sample_kernel<true>, dim3(B), dim3(256), 0, st, h->st, h->logits, h->samp, h->prev, B, Q, h->mu);
    else
        hipLaunchKernelGGL(arw_sample_kernel<false>, dim3(B), dim3(256), 0, st, h->st, h->logits, h->samp, h->prev, B, Q, h->mu);
    VQW_LAUNCH_CHECK("vqw_ar_wide_run(step)");
    return 0;
}

// project the condition of frames [win.f0, win.f0 + win.nf) into condwin, in stream order behind the steps that read the old one
int refresh_window(vqw_ar_wide* h, const float* encoding, int Tz, const ArWideWindow& win, hipStream_t st) {
    const vqw_ar_weights& w = h->w;
    const int B = h->B, L = w.n_layers;
    const size_t n = (size_t)win.nf * w.Cc * B;
    const int blocks = (int)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024);
    hipLaunchKernelGGL(arw_window_kernel, dim3(blocks), dim3(256), 0, st, h->st, encoding, h->enct, B, w.Cc, Tz, win.f0, win.nf);
    for (int l = 0; l <= L; ++l) {
        WideArgs a = base_args(h);
        a.seg[0] = WideSeg{l < L ? h->cond_w[l] : w.post1_cond_w, h->enct, 0, 0};
        a.nseg = 1; a.K = w.Cc; a.ldw = l < L ? w.cond_ld : w.post1_cond_ld; a.N = l < L ? 2 * w.R : w.S;
        a.out = h->condwin + (size_t)l * 2 * w.R * B;
        a.x_zstride = (long long)w.Cc * B; a.out_zstride = (long long)h->Mall * B;
        launch_gemm<MODE_PLAIN>(a, a.N, win.nf, st);
    }
    VQW_LAUNCH_CHECK("vqw_ar_wide_run(condition window)");
    return 0;
}

void free_all(vqw_ar_wide* h) {
    if (!h) return;
    h->step.drop();
    for (float* p : h->rings) (void)hipFree(p);
    void* bufs[] = {h->st, h->samp, h->prev, h->xhist, h->cur, h->gated, h->skip, h->h, h->logits, h->enct, h->condwin};
    for (void* p : bufs) (void)hipFree(p);
    if (h->ev_in) (void)hipEventDestroy(h->ev_in);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

// both kinds of handle; fn names the entry point in the messages.  n_codes > 0: code-input mode.  Every check comes before
// the first device call.
int wide_create(const char* fn, vqw_ar_wide** out, const vqw_ar_weights* w, int batch, int n_codes) {
#define ARW_CHECK(cond, fmt, ...) VQW_CHECK(cond, "%s: " fmt, fn, ##__VA_ARGS__)
    ARW_CHECK(out && w, "null pointer");
    ARW_CHECK(batch >= 1 && batch <= WIDE_MAXB, "batch=%d must be in 1..%d", batch, WIDE_MAXB);
    if (n_codes >= 0) {
        ARW_CHECK(n_codes >= 32 && n_codes % 32 == 0 && n_codes <= 1024, "n_codes=%d must be a multiple of 32 in 32..1024", n_codes);
        ARW_CHECK(w->Q == n_codes, "n_codes=%d must equal w->Q=%d", n_codes, (int)w->Q);
    }
    ARW_CHECK(w->n_layers >= 1, "n_layers=%d must be >= 1", (int)w->n_layers);
    ARW_CHECK(w->kernel_size >= 2 && w->kernel_size <= VQW_MAX_TAPS, "kernel_size=%d must be in 2..%d", (int)w->kernel_size, VQW_MAX_TAPS);
    ARW_CHECK(w->R >= 32 && w->R % 32 == 0, "R=%d must be a positive multiple of 32", (int)w->R);
    ARW_CHECK(w->S >= 32 && w->S % 32 == 0, "S=%d must be a positive multiple of 32", (int)w->S);
    ARW_CHECK(w->Q >= 32 && w->Q % 32 == 0 && w->Q <= 1024, "Q=%d must be a multiple of 32 in 32..1024", (int)w->Q);
    ARW_CHECK(w->Cc >= 16 && w->Cc % 16 == 0, "Cc=%d must be a positive multiple of 16", (int)w->Cc);
    ARW_CHECK(w->pre_k >= 1 && w->pre_k <= 64, "pre_k=%d must be in 1..64", (int)w->pre_k);
    ARW_CHECK(w->dilations && w->gated_w && w->gated_b && w->cond_w && w->out_w && w->out_b, "null weight table");
    for (int l = 0; l < w->n_layers; ++l)
        ARW_CHECK(w->dilations[l] >= 1, "dilation %d of layer %d must be >= 1", (int)w->dilations[l], l);
#undef ARW_CHECK
    vqw_ar_wide* h = new vqw_ar_wide();
    h->assign(w);
    h->B = batch;
    h->n_codes = n_codes > 0 ? n_codes : 0;
    const int L = w->n_layers;
    h->Mall = L * 2 * w->R + w->S;
    h->samp_host.assign(batch, ArSampleRow{1.0f, 0, 1.0f, 0});
#define ARW_ALLOC(ptr, bytes)                                                          \
    do {                                                                               \
        hipError_t e_ = hipMalloc((void**)&(ptr), (bytes));                            \
        if (e_ != hipSuccess) { free_all(h); return vqw_set_error("%s: hipMalloc of %zu bytes failed: %s", fn, (size_t)(bytes), hipGetErrorString(e_)); } \
    } while (0)
    const size_t B = batch, f4 = sizeof(float);
    ARW_ALLOC(h->st, sizeof(WideState));
    ARW_ALLOC(h->samp, B * sizeof(ArSampleRow));
    ARW_ALLOC(h->prev, B * f4);
    ARW_ALLOC(h->xhist, B * w->pre_k * f4);
    ARW_ALLOC(h->cur, B * w->R * f4);
    ARW_ALLOC(h->gated, B * w->R * f4);
    ARW_ALLOC(h->skip, B * w->S * f4);
    ARW_ALLOC(h->h, B * w->S * f4);
    ARW_ALLOC(h->logits, B * w->Q * f4);
    ARW_ALLOC(h->enct, (size_t)AR_WIDE_WINDOW * w->Cc * B * f4);
    ARW_ALLOC(h->condwin, (size_t)AR_WIDE_WINDOW * h->Mall * B * f4);
    h->rings.assign(L, nullptr);
    for (int l = 0; l < L; ++l) ARW_ALLOC(h->rings[l], h->ring_floats(l, batch) * f4);
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_in, hipEventDisableTiming) != hipSuccess) {
        free_all(h);
        return vqw_set_error("%s: stream/event creation failed", fn);
    }
    const int rc = vqw_ar_wide_reset(h, nullptr);
    if (rc) { free_all(h); return rc; }
    HIPC(hipStreamSynchronize(nullptr));
    *out = h;
    return 0;
}

}  // namespace

extern "C" int vqw_ar_wide_create(vqw_ar_wide** out, const vqw_ar_weights* w, int batch) {
    return wide_create("vqw_ar_wide_create", out, w, batch, -1);
}

extern "C" int vqw_ar_wide_prior_create(vqw_ar_wide** out, const vqw_ar_weights* w, int batch, int n_codes) {
    return wide_create("vqw_ar_wide_prior_create", out, w, batch, n_codes);
}

// The mu-law level of an audio handle: 256 after vqw_ar_wide_create, whatever w->Q is.  Every check comes before any device call.
extern "C" int vqw_ar_wide_set_levels(vqw_ar_wide* h, int levels) {
    VqwMu m;
    const int rc = ar_levels_check("vqw_ar_wide", h, levels, &m);
    if (rc) return rc;
    if (m.levels == h->mu.levels) return 0;
    h->mu = m;
    h->step.drop();   // the captured step carries the level as a kernel argument
    return 0;
}

extern "C" int vqw_ar_wide_reset(vqw_ar_wide* h, vqw_stream_t s) {
    VQW_CHECK(h, "vqw_ar_wide_reset: null handle");
    if (h->pending) {
        const int rcw = vqw_ar_wide_wait(h);
        if (rcw) return rcw;
    }
    hipStream_t st = (hipStream_t)s;
    const size_t B = h->B;
    HIPC(hipMemsetAsync(h->st, 0, sizeof(WideState), st));
    HIPC(hipMemsetAsync(h->prev, 0, B * sizeof(float), st));       // audio = zeros (generate.py:103)
    HIPC(hipMemsetAsync(h->xhist, 0, B * h->w.pre_k * sizeof(float), st));
    for (int l = 0; l < h->w.n_layers; ++l)
        HIPC(hipMemsetAsync(h->rings[l], 0, h->ring_floats(l, h->B) * sizeof(float), st));
    h->steps = 0;
    return 0;
}

// Prefill: see include/vqwave.h.  Every check comes before any device call and names the value.
extern "C" int vqw_ar_wide_prefill_layer(vqw_ar_wide* h, int l, const float* x, int ld, int t_first, int t_end, int row0, int nrows,
                                         vqw_stream_t s) {
    VQW_CHECK(h, "vqw_ar_wide_prefill_layer: null handle");
    VQW_CHECK(l >= 0 && l < h->w.n_layers, "vqw_ar_wide_prefill_layer: layer %d outside 0..%d", l, h->w.n_layers - 1);
    VQW_CHECK(t_end >= 0, "vqw_ar_wide_prefill_layer: t_end=%d < 0", t_end);
    VQW_CHECK(t_first >= 0, "vqw_ar_wide_prefill_layer: t_first=%d < 0", t_first);
    VQW_CHECK(nrows >= 1, "vqw_ar_wide_prefill_layer: nrows=%d < 1", nrows);
    VQW_CHECK(arw_rows_inside(row0, nrows, h->B), "vqw_ar_wide_prefill_layer: rows [%d, %lld) outside the handle's 0..%d", row0,
              (long long)row0 + nrows, h->B - 1);
    const int depth = (h->w.kernel_size - 1) * h->dil[l];
    const int t_lo = arw_prefill_first(t_end, depth), nt = arw_prefill_count(t_end, depth);
    VQW_CHECK(arw_prefill_covers(t_first, ld, t_end, depth),
              "vqw_ar_wide_prefill_layer: columns [%d, %lld) do not cover layer %d's steps [%d, %d)", t_first, (long long)t_first + ld, l,
              t_lo, t_end);
    if (nt == 0) return 0;
    VQW_CHECK(x, "vqw_ar_wide_prefill_layer: null x");
    if (h->pending) {
        const int rcw = vqw_ar_wide_wait(h);
        if (rcw) return rcw;
    }
    hipStream_t st = (hipStream_t)s;
    hipLaunchKernelGGL(arw_prefill_scatter_kernel, dim3(arw_tiles(nt), arw_tiles(nrows), h->w.R), dim3(256), 0, st, h->rings[l], depth,
                       h->w.R, h->B, x, ld, t_first, t_lo, nt, row0, nrows);
    VQW_LAUNCH_CHECK("vqw_ar_wide_prefill_layer");
    return 0;
}

extern "C" int vqw_ar_wide_prefill_finish(vqw_ar_wide* h, int t_end, const float* audio_tail, const int32_t* code_tail,
                                          vqw_stream_t s) {
    VQW_CHECK(h, "vqw_ar_wide_prefill_finish: null handle");
    VQW_CHECK(t_end >= 0, "vqw_ar_wide_prefill_finish: t_end=%d < 0", t_end);
    VQW_CHECK((audio_tail == nullptr) != (code_tail == nullptr),
              "vqw_ar_wide_prefill_finish: exactly one of audio_tail / code_tail must be given (%s)",
              audio_tail ? "both are" : "neither is");
    VQW_CHECK(h->n_codes > 0 ? code_tail != nullptr : audio_tail != nullptr,
              "vqw_ar_wide_prefill_finish: %s handle takes %s", h->n_codes > 0 ? "a code-input" : "an audio",
              h->n_codes > 0 ? "code_tail" : "audio_tail");
    if (h->pending) {
        const int rcw = vqw_ar_wide_wait(h);
        if (rcw) return rcw;
    }
    if (t_end == 0) return 0;
    hipStream_t st = (hipStream_t)s;
    hipLaunchKernelGGL(arw_prefill_finish_kernel, dim3(vqw_cdiv(h->B * h->w.pre_k, 256)), dim3(256), 0, st, h->st, h->prev, h->xhist,
                       h->B, h->w.pre_k, t_end, audio_tail, code_tail, h->mu);
    VQW_LAUNCH_CHECK("vqw_ar_wide_prefill_finish");
    h->steps = t_end;
    return 0;
}

extern "C" int vqw_ar_wide_wait(vqw_ar_wide* h) {
    VQW_CHECK(h, "vqw_ar_wide_wait: null handle");
    if (!h->pending) return 0;
    h->pending = false;
    HIPC(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int vqw_ar_wide_run_async(vqw_ar_wide* h, const float* encoding, int Tz, int ratio, int n_steps, int mode,
                                     const float* uniforms, const vqw_ar_sampling* sampling, float* audio, int32_t* indices,
                                     float* probs_last, vqw_stream_t s) {
    VQW_CHECK(h && encoding, "vqw_ar_wide_run: null pointer");
    if (h->n_codes) {
        VQW_CHECK(!audio, "vqw_ar_wide_run: audio must be NULL on a code handle (vqw_ar_wide_prior_create): it draws codes, not samples");
        VQW_CHECK(indices, "vqw_ar_wide_run: indices is NULL: a code handle (vqw_ar_wide_prior_create) needs it for the codes");
    } else {
        VQW_CHECK(audio, "vqw_ar_wide_run: null pointer");
    }
    VQW_CHECK(Tz > 0 && ratio > 0 && n_steps > 0, "vqw_ar_wide_run: bad Tz/ratio/n_steps (%d, %d, %d)", Tz, ratio, n_steps);
    VQW_CHECK(mode == 0 || (mode == 1 && uniforms), "vqw_ar_wide_run: mode must be 0 (greedy) or 1 (sample, needs uniforms)");
    VQW_CHECK(h->steps + n_steps <= 0x7fffffffLL, "vqw_ar_wide_run: the step counter would pass 2^31 - 1");
    if (h->pending) {
        const int rcw = vqw_ar_wide_wait(h);
        if (rcw) return rcw;
    }
    int any = 0;
    {
        const int rc = ar_sampling_rows(sampling, h->B, h->w.Q, mode, h->samp_host.data(), &any);
        if (rc) return rc;
    }
    hipStream_t st = h->stream;
    HIPC(hipEventRecord(h->ev_in, (hipStream_t)s));
    HIPC(hipStreamWaitEvent(st, h->ev_in, 0));
    // run parameters -> device state (step / run_base live on the device)
    WideState hs;
    memset(&hs, 0, sizeof(hs));
    hs.Tz = Tz; hs.ratio = ratio; hs.mode = mode; hs.n_steps = n_steps;
    hs.uniforms = uniforms; hs.audio = audio; hs.indices = indices; hs.probs_last = probs_last;
    HIPC(hipMemcpyAsync(reinterpret_cast<char*>(h->st) + offsetof(WideState, Tz), reinterpret_cast<char*>(&hs) + offsetof(WideState, Tz),
                        sizeof(WideState) - offsetof(WideState, Tz), hipMemcpyHostToDevice, st));
    HIPC(hipMemcpyAsync(h->samp, h->samp_host.data(), (size_t)h->B * sizeof(ArSampleRow), hipMemcpyHostToDevice, st));
    HIPC(hipMemcpyAsync(&h->st->run_base, &h->st->step, sizeof(int), hipMemcpyDeviceToDevice, st));
    HIPC(hipStreamSynchronize(st));  // `hs` is a stack object; also orders the capture below

    if (!h->step.exec) {
        const int rc = h->step.capture(st, [&] { return launch_step(h, st); }, "vqw_ar_wide_run");
        if (rc) return rc;
    }
    // every run projects its own windows: the encoding may be another one than the last run's
    ArWideWindow win;
    long long t = h->steps, left = n_steps;
    while (left > 0) {
        const int frame = arw_frame(t, ratio, Tz);
        if (!arw_window_holds(win, frame)) {
            win = arw_window_at(frame, Tz);
            const int rc = refresh_window(h, encoding, Tz, win, st);
            if (rc) return rc;
        }
        const long long n = arw_steps_in_window(win, t, left, ratio, Tz);
        for (long long i = 0; i < n; ++i) HIPC(hipGraphLaunch(h->step.exec, st));
        t += n;
        left -= n;
        h->steps = t;
        h->pending = true;
    }
    return 0;
}

extern "C" int vqw_ar_wide_destroy(vqw_ar_wide* h) {
    if (!h) return 0;
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    free_all(h);
    return 0;
}
