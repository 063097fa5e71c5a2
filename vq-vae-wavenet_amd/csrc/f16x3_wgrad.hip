// fp16x3 engine: weight gradients.  Two kernels over one work decomposition (WgArgs, wg_decode) and one slab reduction:
//   wgrad_f16x3_kernel<ODD, BF, S2, QP, PP>  the register loop: at least one operand is read as fp32 and converted on the way to LDS
//   wgrad_f16x3_dma_kernel<BF>               both operands as planes: global -> LDS by LDS-DMA, nothing passes through registers;
//                                            2 x 2 wave tiling, q sums only in the blocks that use them
// wg_kernel() maps a launch to one of the 13 instantiations and its LDS bytes.
#include <string.h>

#include "f16x3.h"
#include "f16x3_wgrad_layout.h"

namespace {

#ifndef VQW_WG_PAT_A
#define VQW_WG_PAT_A 4     // register loop: VALU / LDS instructions per MFMA while a chunk is converted ...
#define VQW_WG_PAT_B 2      // ... and address computations / requests per MFMA in the second stage
#endif
constexpr int NSTG = 4;      // LDS stages of the register kernel
#ifndef VQW_WG_DMA_DEPTH
#define VQW_WG_DMA_DEPTH 2   // LDS-DMA kernel: stages of requests left in flight across a step's barrier
#endif
#ifndef VQW_WG_DMA_PAT_MEM
#define VQW_WG_DMA_PAT_MEM 1 // ... its issue pattern: LDS reads / requests per MFMA ...
#define VQW_WG_DMA_PAT_ALU 2 // ... and address computations / q-sum arithmetic per MFMA
#endif
constexpr int WG_DMA_DEPTH = VQW_WG_DMA_DEPTH, WG_DMA_NSTG = WG_DMA_DEPTH + 2;     // (a stage is requested DEPTH + 1 steps before it is read)

// ---------------------------------------------------------------------------------------------------------------
// Weight gradients on the fp16 matrix pipe:  dW[j][c][o] += sum_{b,t} p[b][c][t + shift_j] * q[b][o][t]
// (TF Conv2DBackpropFilter of conv1d_v2, wavenet_ops.py:83-86; q = [q0; q1] along o).
//
// The contraction index is TIME, which is the contiguous index of both fp32 operands [B][C][T]: an MFMA fragment entry
// (row, 8 consecutive k) is 32 contiguous bytes of global memory.  The operands are therefore read as fp32 (whole
// 128-byte lines per row and 32-step stage pair), scaled by their power-of-two guard scale, split into the two fp16
// planes IN REGISTERS (same bytes as reading ready-made planes, no conversion pass, no plane copy in HBM) and written
// to the same LDS stage image as the kernels above, so the fragment reads and the 3-term MFMA loop are shared.
// Output tile 256 (c) x 256 (o) per block; the K range B*T is cut into `nsplit` contiguous chunks per tile so that
// tiles * nsplit fills the chip once; partial tiles go to a slab [tile][split][256][256] and a second kernel adds them
// up in a fixed order (no atomics: dW is bitwise reproducible).  Needs T % 32 == 0, C % 256 == 0, shifts <= 0.
// One launch carries up to WG_MAX_BATCH independent problems of the same shape (the weight gradients of several layers):
// every problem has its own operands, scales, sums and output, the tiles of all problems share the K split -- the slab
// holds tiles x splits <= CUs partial tiles whatever the batch size, so a batch of n layers writes and re-reads 1/n of
// the slab bytes per layer that n single launches would.
constexpr int WG_MAX_BATCH = 32;
struct WgProblem {
    const float* p;
    const float* q0;
    const float* q1;
    float* dw;
    const float* sp;      // device scalars (or NULL = 1): power-of-two scales of p, q0, q1
    const float* sq0;
    const float* sq1;
    // sums of q over time, formed from the registers that hold q anyway (blocks of the problem's first row tile and tap only):
    float* q_total;       // [Q0 + Q1] += sum_{b,t} q[b][o][t]  (bias gradients) or NULL
    float* q_seg;         // [B][seg_bstride/..]: q_seg[b * seg_bstride + o * seg_T + t / seg_ratio] += q[b][o][t] (the transpose of
                          //   add_condition's upsampling, wavenet_ops.py:98-100) or NULL; seg_ratio % 32 == 0
    const void* qp;       // QP kernels: q as operand planes [planes][q_KC chunks][B*T rows][8] (scaled by *sq0 * q_hscale), chunks from q_kc0
    int q_KC, q_kc0;
    float q_hscale;       // host-side part of the planes' scale (a power of two; 1 where the scale lives on the device)
    const void* pp;       // PP kernels: p as operand planes, likewise
    int p_KC, p_kc0;
    float p_hscale;
    int pkoff[VQW_MAX_TAPS];   // PP: chunk offset of tap j's rows (space-to-depth planes of a stride-2 conv's input: the parity block)
    int shift[VQW_MAX_TAPS];
};
struct WgArgs {
    WgProblem pr[WG_MAX_BATCH];
    float* slab;
    int nprob;
    int B, T, Cp, Q0, Q1, ntaps;
    int Tp;               // row length of p (= T, or the input length of a stride-2 conv: p index 2 t + shift)
    int p_relu;           // p := max(p, 0) on the way in (the convs behind a relu, wavenet.py:79, 93)
    int nsplit, pairs_row, pairs_total, n_nt;
    long seg_bstride;
    int seg_T, seg_ratio;
    int total_o0, total_o1;   // q_total covers columns [total_o0, total_o1) only (e.g. the residual rows S..S+R)
    long lddw, dw_tap_stride; // (the reduction)
};
// Work item w (after the XCD remap: consecutive w on one XCD) -> (K split, problem, row tile, column tile, tap), taps fastest:
// the taps of one tile and K range read the same q panel and p panels that are the same cache lines a few elements apart, the
// column tiles of a row tile share its p panel, and everything of one K range sits on as few XCDs (L2s) as possible.
struct WgItem {
    int prob, tap, rtl, nt, split, gtile;      // rtl: 256-row tile within the problem; gtile: slab / reduction index
};
__device__ __forceinline__ WgItem wg_decode(int w, const WgArgs& a) {
    const int cpt = a.Cp / 256;
    WgItem it;
    it.tap = w % a.ntaps; w /= a.ntaps;
    it.nt = w % a.n_nt; w /= a.n_nt;
    const int rows_all = a.nprob * cpt, rt = w % rows_all;
    it.split = w / rows_all;
    it.prob = rt / cpt;
    it.rtl = rt - it.prob * cpt;
    it.gtile = ((it.prob * a.ntaps + it.tap) * cpt + it.rtl) * a.n_nt + it.nt;
    // The divisions run on the vector ALU, so the compiler takes everything derived from them for lane-dependent: the problem's
    // pointers were fetched per lane, the buffer resources built from them lived in VGPRs and every operand request of the main
    // loop became a readfirstlane "waterfall" loop of its own (26 of them in the planes variant, each a scheduling barrier
    // between the MFMAs).  One readfirstlane per field states what is true anyway.
    it.prob = __builtin_amdgcn_readfirstlane(it.prob); it.tap = __builtin_amdgcn_readfirstlane(it.tap);
    it.rtl = __builtin_amdgcn_readfirstlane(it.rtl); it.nt = __builtin_amdgcn_readfirstlane(it.nt);
    it.split = __builtin_amdgcn_readfirstlane(it.split); it.gtile = __builtin_amdgcn_readfirstlane(it.gtile);
    return it;
}

template <bool BF>
__device__ __forceinline__ uint2 split4(const f32x4 v, float sc, uint2& lo) {
    u16 a[4], b[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float xs = v[e] * sc;
        if (BF) { a[e] = bf16_bits(xs); b[e] = 0; continue; }
        const _Float16 h1 = (_Float16)xs;
        a[e] = f16_bits(h1);
        b[e] = f16_bits((_Float16)(xs - (float)h1));
    }
    lo = make_uint2(b[0] | ((unsigned)b[1] << 16), b[2] | ((unsigned)b[3] << 16));
    return make_uint2(a[0] | ((unsigned)a[1] << 16), a[2] | ((unsigned)a[3] << 16));
}

// ODD: some tap shift is not a multiple of 4 (compile-time: a branch would cut the loop body into scheduling regions)
// S2: p is the input of a stride-2 convolution (encoder.py:17-18): dW[j][c][o] += sum p[b][c][2 t + shift_j] q[b][o][t], shifts of
// either sign, indices outside [0, Tp) are the conv's zero padding.  p is then fetched one float per request (stride 8 bytes
// between the four of a chunk), each one range-checked on its own through the buffer descriptor.
// QP: q is not read as fp32 but as the OPERAND PLANES its producer wrote anyway (gate backward writes dpre as planes for the input
// gradient; with this variant it no longer writes the 109 MB of fp32 dpre per layer at all).  Planes are channel-chunk-major --
// 16 bytes = 8 channels of one time step -- while this contraction runs over TIME: the 16-byte entries go to LDS as they are, as a
// [time step][channel] image per plane (rows of 512 + 64 bytes: the four rows of a transposed read fall into four different
// 16-bank groups), and the B fragments are fetched with ds_read_b64_tr_b16, which hands lane (channel n, k half) its 4 + 4
// consecutive time steps.  No conversion arithmetic for q (two thirds of the conversions of the gate kernels' gradient).
constexpr int WG_QSTR = 576, WG_QPL = 16 * WG_QSTR;                       // bytes per time step / per plane of a stage's q image
// PP: the same for p (the layer input planes the forward pass wrote, the gated planes): a tap's shift is then a row offset of
// the planes -- no unaligned 16-byte windows, no ODD variant -- and the loop converts nothing at all.
// QP && PP is a kernel of its own, wgrad_f16x3_dma_kernel below.
template <bool QP, bool PP, bool BF> struct WgStage {
    static constexpr int BOFF = PP ? (BF ? 1 : 2) * WG_QPL : 16 * 1024;      // q image behind the p image
    static constexpr int BYTES = BOFF + (QP ? (BF ? 1 : 2) * WG_QPL : 16 * 1024);
    static constexpr int STAGES = NSTG;
};
__device__ __forceinline__ uint2 wg_tr_read(const char* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef __fp16 h4 __attribute__((__vector_size__(4 * sizeof(__fp16))));
    const h4 v = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) h4*)(p));
    return __builtin_bit_cast(uint2, v);
#else
    return make_uint2(0, 0);
#endif
}

// ---- what the register kernel and the LDS-DMA kernel share as functions.  Their prologue (work item -> tile, scales, plane bases),
// flush_pair, the q_total add and the slab store stand in both kernel bodies: as functions of their own, or in another order, they
// compile to other code (tools/isa_identity.py).
// 12 MFMAs: row tiles i, i+1 (A fragments fa, both planes) x the wave's 2 column tiles (B fragments b), the three terms outermost
// (small first) so that two MFMAs into the same accumulator are three independent ones apart
template <bool BF>
__device__ __forceinline__ void wg_mfma_rows(f32x16 (&acc)[8][2], const uint4 (&fa)[8][2], const uint4 (&b)[2][2], int i) {
    if constexpr (BF) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            acc[i + (q >> 1)][q & 1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fa[i + (q >> 1)][0]), __builtin_bit_cast(bf16x8, b[q & 1][0]), acc[i + (q >> 1)][q & 1], 0, 0, 0);
    } else {
#pragma unroll
        for (int term = 0; term < 3; ++term)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int ii = i + (q >> 1), j = q & 1;
                const int pa = term == 1 ? 1 : 0, pb = term == 0 ? 1 : 0;
                acc[ii][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, fa[ii][pa]), __builtin_bit_cast(f16x8, b[j][pb]), acc[ii][j], 0, 0, 0);
            }
    }
}

// q sums from the B fragments (q as planes): lane (channel n of column tile j, k half) holds 8 consecutive time steps of its channel
// per plane: their sum, over both planes, descaled -- the fp32 value to 2^-22 (the planes carry 22-23 significand bits)
template <bool BF>
__device__ __forceinline__ void wg_sum_frag(float (&qs_pair)[2], const uint4 (&b)[2][2], float inv_scq) {
#ifdef VQW_ABL_WG_NOSUM
    return;
#endif
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        float acc_ = 0.0f;
#pragma unroll
        for (int pl = 0; pl < (BF ? 1 : 2); ++pl) {
            const unsigned wds[4] = {b[j][pl].x, b[j][pl].y, b[j][pl].z, b[j][pl].w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (BF) {
                    acc_ += __uint_as_float(wds[e] << 16) + __uint_as_float(wds[e] & 0xffff0000u);
                } else {
                    acc_ += (float)__builtin_bit_cast(_Float16, (u16)(wds[e] & 0xffffu)) + (float)__builtin_bit_cast(_Float16, (u16)(wds[e] >> 16));
                }
            }
        }
        qs_pair[j] += acc_ * inv_scq;
    }
}

// ---- the register kernel: an operand read as fp32 passes through registers (rgp / rgq), where it is converted; so does one read
// as planes, which goes to the padded [time step][channel] image.  A ring of NSTG 16-step stages, one __syncthreads() per pair.
template <bool ODD, bool BF, bool S2 = false, bool QP = false, bool PP = false>
__global__ __launch_bounds__(256, 1) void wgrad_f16x3_kernel(const WgArgs a) {
    static_assert(!(QP && PP), "both operands as planes: wgrad_f16x3_dma_kernel");
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    constexpr int STGB = WgStage<QP, PP, BF>::BYTES, BOFF = WgStage<QP, PP, BF>::BOFF, NPL = BF ? 1 : 2;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l31 = lane & 31, lhi = lane >> 5;
    const WgItem it = wg_decode(vqw_xcd_remap(blockIdx.x, gridDim.x), a);
    const WgProblem& pr = a.pr[it.prob];
    const int split = it.split, tap = it.tap, c0 = it.rtl * 256;
    const int shift = pr.shift[tap];
    const int o0 = it.nt * 256;
    const bool from_q1 = o0 >= a.Q0;
    const float* qsrc = from_q1 ? pr.q1 : pr.q0;
    const int Qs = from_q1 ? a.Q1 : a.Q0, oq = from_q1 ? o0 - a.Q0 : o0;
    const float scp = dev_scale(pr.sp) * (PP ? pr.p_hscale : 1.0f), scq = dev_scale(from_q1 ? pr.sq1 : pr.sq0) * (QP ? pr.q_hscale : 1.0f);
    const float plo = a.p_relu ? 0.0f : -INFINITY;
    const int T = a.T;
    const int s_begin = (int)((long)split * a.pairs_total / a.nsplit), s_end = (int)((long)(split + 1) * a.pairs_total / a.nsplit);
    const __amdgpu_buffer_rsrc_t rp = vqw_make_rsrc(PP ? reinterpret_cast<const float*>(pr.pp) : pr.p, (unsigned)((size_t)a.B * a.Cp * (S2 ? a.Tp : T) * 4));
    const __amdgpu_buffer_rsrc_t rq = vqw_make_rsrc(QP ? reinterpret_cast<const float*>(pr.qp) : qsrc, (unsigned)((size_t)a.B * Qs * T * 4));
    // QP: one resource per plane, based at this block's first chunk (32 chunks = its 256 q rows)
    const size_t NBq = (size_t)a.B * T;
    const char* qpb = reinterpret_cast<const char*>(pr.qp) + (QP ? ((size_t)pr.q_kc0 + o0 / 8) * NBq * 16 : 0);
    const unsigned qspan = (unsigned)(32 * NBq * 16 < 0x7fffffffull ? 32 * NBq * 16 : 0x7fffffffull);
    const __amdgpu_buffer_rsrc_t rqp0 = vqw_make_rsrc(qpb, qspan);
    const __amdgpu_buffer_rsrc_t rqp1 = vqw_make_rsrc(qpb + (QP && !BF ? (size_t)pr.q_KC * NBq * 16 : 0), qspan);
    const char* ppb = reinterpret_cast<const char*>(pr.pp) + (PP ? ((size_t)pr.p_kc0 + pr.pkoff[tap] + c0 / 8) * NBq * 16 : 0);
    const __amdgpu_buffer_rsrc_t rpp0 = vqw_make_rsrc(ppb, qspan);
    const __amdgpu_buffer_rsrc_t rpp1 = vqw_make_rsrc(ppb + (PP && !BF ? (size_t)pr.p_KC * NBq * 16 : 0), qspan);
    float* const q_total = pr.q_total;
    float* const q_seg = pr.q_seg;

    // One load instruction of a wave = 32 rows x 32 bytes (lane -> row lane/2, 16-byte half lane%2); chunk n of a
    // thread: 32-row group g = wv*2 + n/4, quarter nn = n%4 of the 128-byte line = stage nn/2 of the pair, k half nn%2.
    // The four quarters of a line are requested back to back, so the line is fetched once.
    f32x4 rgp[8], rgq[8];
    const int rsub = lane >> 1, hsel = lane & 1;
    int pb = 0, pt0 = 0;                                // batch row / first time step of the pair being requested
    auto issue_one = [&](int n) {
        const int g = wv * 2 + (n >> 2), nn = n & 3;
        const int row = g * 32 + rsub;
        const int tq = pt0 + 8 * nn + 4 * hsel;
        // (S2: T need not be a multiple of the 32-step stage pairs -- steps behind the row's end read as zero)
        if constexpr (QP) {
            // item n of this thread: plane n / 4, chunks (n % 4) * 8 + lane % 8, time step 8 wv + lane / 8 of the pair's 32 --
            // eight lanes = eight chunks of one step (128 contiguous bytes of LDS), eight lane groups = the eight steps of one
            // 128-byte line per chunk
            if (n < 4 * NPL) {
                const int chunk = (n & 3) * 8 + (lane & 7), t = 8 * wv + (lane >> 3);
                // (steps behind the row's end read as zero; with one operand as fp32 T is a multiple of the 32-step pairs and there are none)
                const int off = (pt0 + t < T) ? (int)(((size_t)chunk * NBq + (size_t)pb * T + pt0 + t) * 16) : (int)0x80000000;
                rgq[n] = vqw_buf_load4((n >> 2) ? rqp1 : rqp0, off, 0);
            }
        } else {
            rgq[n] = vqw_buf_load4(rq, (!S2 || tq < T) ? (int)((((size_t)pb * Qs + oq + row) * T + tq) * 4) : (int)0x80000000, 0);
        }
        if constexpr (PP) {      // the same item geometry as QP; the tap's shift is a row offset, rows before the batch row read as zero
            if (n < 4 * NPL) {
                const int chunk = (n & 3) * 8 + (lane & 7), tt = pt0 + 8 * wv + (lane >> 3) + shift;
                // (tt >= T: only with the positive row shifts of a stride-2 conv's taps -- its right zero padding)
                const int off = (tt >= 0 && tt < T) ? (int)(((size_t)chunk * NBq + (size_t)pb * T + tt) * 16) : (int)0x80000000;
                rgp[n] = vqw_buf_load4((n >> 2) ? rpp1 : rpp0, off, 0);
            }
            return;
        }
        if (S2) {
            const size_t prow = ((size_t)pb * a.Cp + c0 + row) * a.Tp;
            f32x4 w;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int idx = 2 * (tq + e) + shift;
                w[e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rp, (idx >= 0 && idx < a.Tp && tq < T) ? (int)((prow + idx) * 4) : (int)0x80000000, 0, 0));
            }
            rgp[n] = w;
            return;
        }
        const int tp = tq + shift;                      // shift <= 0: never past the row's end
        const size_t prow = ((size_t)pb * a.Cp + c0 + row) * T;
        // a 16-byte window that straddles t = 0 (only with shifts that are not multiples of 4) is read from t = 0 and moved
        // up inside the register below; windows entirely before t = 0 read as zero through the buffer range check
        const int tl = tp >= 0 ? tp : (tp > -4 ? 0 : -1);
        // (ODD: the straddling window is moved up when the registers are CONVERTED, commit_one -- doing it here, on the value just
        // requested, made every request of the unaligned variant wait for its own data: 205 instead of 150 us per gate kernel)
        rgp[n] = vqw_buf_load4(rp, tl >= 0 ? (int)((prow + tl) * 4) : (int)0x80000000, 0);
    };
    auto set_pair = [&](int s) { pb = s / a.pairs_row; pt0 = (s - pb * a.pairs_row) * 32; };
    int pt0_c = 0;                                      // first time step of the pair being converted (ODD only)
    auto set_commit_pair = [&](int s) { if (ODD) pt0_c = (s % a.pairs_row) * 32; };
    auto commit_one = [&](int n, int pair) {     // raw registers -> two fp16 planes -> LDS stage (2 pair + nn/2) % 4
        const int g = wv * 2 + (n >> 2), nn = n & 3;
        char* st = smem + ((2 * pair + (nn >> 1)) % NSTG) * STGB + ((nn & 1) * 32 + rsub) * 16 + hsel * 8;
        uint2 lo;
        uint2 hi;
        f32x4 pv = rgp[n];
        if constexpr (PP) {
            if (n < 4 * NPL) {
                const int chunk = (n & 3) * 8 + (lane & 7), t = 8 * wv + (lane >> 3);
                char* dp_ = smem + ((2 * pair + (t >> 4)) % NSTG) * STGB + (n >> 2) * WG_QPL + (t & 15) * WG_QSTR + chunk * 16;
                *reinterpret_cast<f32x4*>(dp_) = pv;
            }
        } else {
        if (ODD && !S2) {
            const int tp = pt0_c + 8 * nn + 4 * hsel + shift;
            const int k = (tp < 0 && tp > -4) ? -tp : 0;      // the window was read from t = 0: its first k elements lie before the row
            const f32x4 w = pv;
            pv[0] = k == 0 ? w[0] : 0.0f;
            pv[1] = k == 0 ? w[1] : (k == 1 ? w[0] : 0.0f);
            pv[2] = k == 0 ? w[2] : (k == 1 ? w[1] : (k == 2 ? w[0] : 0.0f));
            pv[3] = k == 0 ? w[3] : (k == 1 ? w[2] : (k == 2 ? w[1] : w[0]));
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) pv[e] = fmaxf(pv[e], plo);
        hi = split4<BF>(pv, scp, lo);
        *reinterpret_cast<uint2*>(st + (g * 2 + 0) * 1024) = hi;
        if (!BF) *reinterpret_cast<uint2*>(st + (g * 2 + 1) * 1024) = lo;
        }
        if constexpr (QP) {
            if (n < 4 * NPL) {     // the plane entry as it is: [time step][channel] image of its plane and stage
                const int chunk = (n & 3) * 8 + (lane & 7), t = 8 * wv + (lane >> 3);
                char* dq = smem + ((2 * pair + (t >> 4)) % NSTG) * STGB + BOFF + (n >> 2) * WG_QPL + (t & 15) * WG_QSTR + chunk * 16;
                *reinterpret_cast<f32x4*>(dq) = rgq[n];
            }
        } else {
            hi = split4<BF>(rgq[n], scq, lo);
            *reinterpret_cast<uint2*>(st + BOFF + (g * 2 + 0) * 1024) = hi;
            if (!BF) *reinterpret_cast<uint2*>(st + BOFF + (g * 2 + 1) * 1024) = lo;
        }
    };
    // q sums (bias / condition gradients): the thread's two q rows (groups wv*2 and wv*2+1), its half of the 32 steps
    const bool do_sum = it.rtl == 0 && tap == 0 && (q_seg != nullptr || (q_total != nullptr && o0 < a.total_o1 && o0 + 256 > a.total_o0));
    float qs_pair[2] = {0.f, 0.f}, qs_tot[2] = {0.f, 0.f};
    auto sum_one = [&](int n) {            // called with commit_one(n): rgq[n] still holds the raw fp32 values
#ifdef VQW_ABL_WG_NOSUM
        return;
#endif
        if constexpr (QP) return;          // (QP: the sums are formed from the B fragments, sum_frag)
        const f32x4 v = rgq[n];
        qs_pair[n >> 2] += (v[0] + v[1]) + (v[2] + v[3]);
    };
    const float inv_scq = __builtin_amdgcn_rcpf(scq);
    // (through a lambda, here and in the LDS-DMA kernel: called directly the helper compiles to other code)
    auto sum_frag = [&](const uint4 (&b)[2][2]) { if constexpr (QP) wg_sum_frag<BF>(qs_pair, b, inv_scq); };
    auto flush_pair = [&](int s) {         // pair s is complete in qs_pair: add it to its condition frame, fold it into the totals
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            // the partner lane holds the other 16 steps (QP: the other k half of the fragment)
            const float both = qs_pair[h] + __shfl_xor(qs_pair[h], QP ? 32 : 1, 64);
            qs_tot[h] += qs_pair[h];
            qs_pair[h] = 0.f;
            if (q_seg && (QP ? lhi == 0 : hsel == 0)) {
                const int b = s / a.pairs_row, t0 = (s - b * a.pairs_row) * 32;
                const int row = o0 + (wv * 2 + h) * 32 + (QP ? l31 : rsub);
                unsafeAtomicAdd(q_seg + (size_t)b * a.seg_bstride + (size_t)row * a.seg_T + t0 / a.seg_ratio, both);
            }
        }
    };
    uint4 fa[8][2], fb[2][2];                        // A fragments (both planes) of 8 row tiles, B fragments of this wave's 2 column tiles
    // transposed reads (QP / PP): 16-lane group G = lane / 16 reads rows (time steps) 8 (G / 2) + 4 r + 0..3, 16 columns (channels)
    // from 16 (G % 2) of the 32-channel tile; its lane 4 q + p supplies the address of row q, columns 4 p .. 4 p + 3 and receives
    // column lane % 16
    const int tr_lane = (8 * (lane >> 5) + ((lane & 15) >> 2)) * WG_QSTR + (16 * ((lane >> 4) & 1) + 4 * (lane & 3)) * 2;
    auto read_a = [&](int i, int stage) {
        if constexpr (PP) {
            const char* st = smem + (stage % NSTG) * STGB + tr_lane + i * 64;
#pragma unroll
            for (int pl = 0; pl < NPL; ++pl) {
                const uint2 k0 = wg_tr_read(st + pl * WG_QPL), k1 = wg_tr_read(st + pl * WG_QPL + 4 * WG_QSTR);
                fa[i][pl] = make_uint4(k0.x, k0.y, k1.x, k1.y);
            }
        } else {
            const char* st = smem + (stage % NSTG) * STGB + lane * 16;
            fa[i][0] = *reinterpret_cast<const uint4*>(st + (i * 2 + 0) * 1024);
            if (!BF) fa[i][1] = *reinterpret_cast<const uint4*>(st + (i * 2 + 1) * 1024);
        }
    };
    auto read_b = [&](uint4 (&b)[2][2], int stage) {
        if constexpr (QP) {
            const char* st = smem + (stage % NSTG) * STGB + BOFF + tr_lane + wv * 128;
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int pl = 0; pl < NPL; ++pl) {
                    const uint2 k0 = wg_tr_read(st + j * 64 + pl * WG_QPL), k1 = wg_tr_read(st + j * 64 + pl * WG_QPL + 4 * WG_QSTR);
                    b[j][pl] = make_uint4(k0.x, k0.y, k1.x, k1.y);
                }
        } else {
            const char* st = smem + (stage % NSTG) * STGB + lane * 16 + BOFF;
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int pl = 0; pl < NPL; ++pl) b[j][pl] = *reinterpret_cast<const uint4*>(st + ((wv * 2 + j) * 2 + pl) * 1024);
        }
    };
    f32x16 acc[8][2];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int npairs = s_end - s_begin;
    if (npairs > 0) {
        set_pair(s_begin);
        set_commit_pair(s_begin);
#pragma unroll
        for (int n = 0; n < 8; ++n) issue_one(n);
#pragma unroll
        for (int n = 0; n < 8; ++n) { commit_one(n, 0); sum_one(n); }
        if (!QP && do_sum) flush_pair(s_begin);
        set_pair(s_begin + 1);
#pragma unroll
        for (int n = 0; n < 8; ++n) issue_one(n);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 8; ++i) read_a(i, 0);
        read_b(fb, 0);
        sum_frag(fb);
        for (int it = 0; it < npairs; ++it) {
            // Stages 2it, 2it+1 (pair `it`) are in LDS, the fragments of stage 2it in registers; the raw operands of pair
            // it+1 are in rgp / rgq (requested one iteration ago).  Row tile by row tile: 6 MFMAs of the first stage, behind
            // them the tile's fragments of the second stage are fetched and one chunk of pair it+1 is converted and written
            // to the two LDS stages pair it-1 was read from; then the second stage's MFMAs with the requests of pair it+2
            // behind them.  VALU / LDS / VMEM work is issued in the shadow of the MFMAs.
            // (No conditionals inside: past the block's last pair the conversion rewrites stale registers into LDS stages
            // nobody reads again and the requests fall behind the end of the buffers, where raw buffer loads return zero --
            // branches would cut the body into scheduling regions and the MFMAs could no longer be interleaved.)
            set_commit_pair(s_begin + it + 1);
#pragma unroll
            for (int i = 0; i < 8; i += 2) {
                wg_mfma_rows<BF>(acc, fa, fb, i);
                read_a(i, 2 * it + 1);
                read_a(i + 1, 2 * it + 1);
                commit_one(i, it + 1);
                commit_one(i + 1, it + 1);
                sum_one(i);
                sum_one(i + 1);
#pragma unroll
                for (int k_ = 0; k_ < 12; ++k_) {         // 1 MFMA, then ~1/12 of the group's VALU / LDS work in its shadow
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x002 | 0x100 | 0x200, VQW_WG_PAT_A, 0);
                }
            }
            if (!QP && do_sum && it + 1 < npairs) flush_pair(s_begin + it + 1);
            set_pair(s_begin + it + 2);
            read_b(fb, 2 * it + 1);        // (after the first stage's last use of fb: 16 registers instead of 32)
            sum_frag(fb);
            if (QP && do_sum) flush_pair(s_begin + it);     // both stages of pair `it` have been read
#pragma unroll
            for (int i = 0; i < 8; i += 2) {
                wg_mfma_rows<BF>(acc, fa, fb, i);
                issue_one(i);
                issue_one(i + 1);
#pragma unroll
                for (int k_ = 0; k_ < 12; ++k_) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x002 | 0x004 | 0x020, VQW_WG_PAT_B, 0);
                }
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < 8; ++i) read_a(i, 2 * it + 2);
            read_b(fb, 2 * it + 2);
            sum_frag(fb);                  // (behind the last pair: a stale stage, never flushed)
        }
    }
    if (do_sum && q_total) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float both = qs_tot[h] + __shfl_xor(qs_tot[h], QP ? 32 : 1, 64);
            const int row = o0 + (wv * 2 + h) * 32 + (QP ? l31 : rsub);
            if ((QP ? lhi == 0 : hsel == 0) && row >= a.total_o0 && row < a.total_o1) unsafeAtomicAdd(q_total + row, both);
        }
    }
    // ---- partial tile -> slab [tile][split][256][256], rows c, columns o (32 lanes = 128 contiguous bytes)
    const float inv = __builtin_amdgcn_rcpf(scp * scq);
    float* out = a.slab + ((size_t)it.gtile * a.nsplit + split) * 65536;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int v4 = 0; v4 < 4; ++v4)
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    out[(32 * i + 8 * v4 + 4 * lhi + e) * 256 + 64 * wv + 32 * j + l31] = acc[i][j][v4 * 4 + e] * inv;
}

// ---- the LDS-DMA kernel: both operands as planes.  Nothing is converted, so nothing needs to pass through registers -- both operands
// go global -> LDS by LDS-DMA (x3_dma16) into a ring of WG_DMA_NSTG 16-step stages, as in the conv main loop (f16x3_mainloop): no
// rgp / rgq, no ds_write, no commit.  A DMA writes lane-linear 1-KiB pieces, which rules the padded rows out: the image is the
// XOR-permuted one of f16x3_wgrad_layout.h (8 KiB per plane and stage, no padding).  A tap's shift is a row offset of p's planes.
// The four waves tile the block 2 x 2 (128 rows x 128 columns each, acc[4][4]: 8 A + 8 B fragments per step where 256 rows x 64
// columns took 16 + 4), and the q sums are formed only where they are used: the loop body is chosen in front of the loop.
template <bool BF> struct WgDmaStage {
    static constexpr int BOFF = (BF ? 1 : 2) * wgl::PLANE, BYTES = 2 * BOFF, STAGES = WG_DMA_NSTG;      // q image behind the p image
};
// 12 MFMAs (bf16: 4): row tile i x the wave's 4 column tiles, the three terms outermost (small first): two MFMAs into the same
// accumulator are three independent ones apart, and every accumulator sees its terms in wg_mfma_rows' order
template <bool BF>
__device__ __forceinline__ void wg_mfma_row4(f32x16 (&acc)[4][4], const uint4 (&fa)[4][2], const uint4 (&b)[4][2], int i) {
    if constexpr (BF) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fa[i][0]), __builtin_bit_cast(bf16x8, b[j][0]), acc[i][j], 0, 0, 0);
    } else {
#pragma unroll
        for (int term = 0; term < 3; ++term)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int pa = term == 1 ? 1 : 0, pb = term == 0 ? 1 : 0;
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, fa[i][pa]), __builtin_bit_cast(f16x8, b[j][pb]), acc[i][j], 0, 0, 0);
            }
    }
}

template <bool BF>
__global__ __launch_bounds__(256, 1) void wgrad_f16x3_dma_kernel(const WgArgs a) {
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    constexpr int STGB = WgDmaStage<BF>::BYTES, BOFF = WgDmaStage<BF>::BOFF, NPL = BF ? 1 : 2;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l31 = lane & 31, lhi = lane >> 5;
    const WgItem it = wg_decode(vqw_xcd_remap(blockIdx.x, gridDim.x), a);
    const WgProblem& pr = a.pr[it.prob];
    const int split = it.split, tap = it.tap, c0 = it.rtl * 256;
    const int shift = pr.shift[tap];
    const int o0 = it.nt * 256;
    const bool from_q1 = o0 >= a.Q0;
    const float scp = dev_scale(pr.sp) * pr.p_hscale, scq = dev_scale(from_q1 ? pr.sq1 : pr.sq0) * pr.q_hscale;
    const int T = a.T;
    const int s_begin = (int)((long)split * a.pairs_total / a.nsplit), s_end = (int)((long)(split + 1) * a.pairs_total / a.nsplit);
    // one resource per wave (below), based at this block's first chunk of its operand and plane (32 chunks = its 256 rows)
    const size_t NBq = (size_t)a.B * T;
    const char* qpb = reinterpret_cast<const char*>(pr.qp) + ((size_t)pr.q_kc0 + o0 / 8) * NBq * 16;
    const unsigned qspan = (unsigned)(32 * NBq * 16 < 0x7fffffffull ? 32 * NBq * 16 : 0x7fffffffull);
    const size_t pl1q = !BF ? (size_t)pr.q_KC * NBq * 16 : 0;
    const char* ppb = reinterpret_cast<const char*>(pr.pp) + ((size_t)pr.p_kc0 + pr.pkoff[tap] + c0 / 8) * NBq * 16;
    const size_t pl1p = !BF ? (size_t)pr.p_KC * NBq * 16 : 0;
    float* const q_total = pr.q_total;
    float* const q_seg = pr.q_seg;
    const int wvu = __builtin_amdgcn_readfirstlane(wv);
    // 2 x 2 wave tiling (f16x3_wgrad_layout.h): wave (wr, wc) owns row tiles 4 wr + i, column tiles 4 wc + j
    const int wr = wvu >> 1, wc = wvu & 1;
    // q sums, from the B fragments: lane (channel l31, k half lhi) of column tiles j = 2 wr, 2 wr + 1 of the wave's four
    const bool do_sum = it.rtl == 0 && tap == 0 && (q_seg != nullptr || (q_total != nullptr && o0 < a.total_o1 && o0 + 256 > a.total_o0));
    float qs_pair[2] = {0.f, 0.f}, qs_tot[2] = {0.f, 0.f};
    const float inv_scq = __builtin_amdgcn_rcpf(scq);
    const int sum_row0 = o0 + (4 * wc + 2 * wr) * 32 + l31;
    static_assert(wgl::wave_b_tile(0, wgl::wave_sum_j(0, 0)) == 0 && wgl::wave_b_tile(1, wgl::wave_sum_j(1, 0)) == 4 &&
                  wgl::wave_b_tile(2, wgl::wave_sum_j(2, 0)) == 2 && wgl::wave_b_tile(3, wgl::wave_sum_j(3, 0)) == 6, "first summed column tile: 4 wc + 2 wr");
    auto sum_frag = [&](const uint4 (&b)[2][2]) { wg_sum_frag<BF>(qs_pair, b, inv_scq); };
    auto flush_pair = [&](int s) {         // pair s is complete in qs_pair: add it to its condition frame, fold it into the totals
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float both = qs_pair[h] + __shfl_xor(qs_pair[h], 32, 64);      // the partner lane holds the other k half
            qs_tot[h] += qs_pair[h];
            qs_pair[h] = 0.f;
            if (q_seg && lhi == 0) {
                const int b = s / a.pairs_row, t0 = (s - b * a.pairs_row) * 32;
                const int row = sum_row0 + h * 32;
                unsafeAtomicAdd(q_seg + (size_t)b * a.seg_bstride + (size_t)row * a.seg_T + t0 / a.seg_ratio, both);
            }
        }
    };
    uint4 fa[4][2], fb[4][2];                        // A fragments (both planes) of the wave's 4 row tiles, B fragments of its 4 column tiles
    f32x16 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    const int npairs = s_end - s_begin;
    // One step = one 16-step stage, as in the register kernel: per accumulator the stages and the three terms come in its order,
    // so dW is the same bit for bit (only the order ACROSS accumulators differs).
    constexpr int P = 4 * NPL;             // 1-KiB pieces a wave requests per stage: 2 operands x NPL planes x 8 pieces over 4 waves
    // Piece w = wvu * P + k of a stage, in image order: operand (p, q), plane, time half, chunk group.  Two planes: wave 0 / 1 move
    // p's plane 0 / 1, wave 2 / 3 q's; one plane (bf16): wave 0 / 1 move p's time half 0 / 1, wave 2 / 3 q's.  A wave therefore
    // requests from ONE resource with ONE shift (q: none).  (Which wave MOVES a piece has nothing to do with which waves read it.)
    const bool w_is_p = wvu < 2;
    const int w_plane = BF ? 0 : (wvu & 1), w_shift = w_is_p ? shift : 0;
    // (requests past the block's last stage, rows outside the batch row and steps behind T carry the offset 2^31, outside every
    // resource -- qspan < 2^31 -- whatever the problem and the number of planes: they land as zeros)
    const u32x4 rs = x3_rsrc_words((w_is_p ? ppb : qpb) + (w_plane ? (w_is_p ? pl1p : pl1q) : 0), qspan);
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
    const unsigned wdst = lds0 + (unsigned)(wvu * P * wgl::PIECE);
    // lane = 8 step + slot fetches chunk swz(step, slot) of the piece's chunk group at time step `step` of the piece's time half
    const int dstep = lane >> 3;
    const int lane_off = (int)((size_t)wgl::swz(dstep, lane & 7) * NBq * 16) + (dstep + w_shift) * 16;
    const int cg_off = (int)(8 * NBq * 16);                    // one chunk group further
    // the stage being requested: batch row (as a byte offset of its first row) and first time step, advanced by 16 steps at a time
    const int row_steps = a.pairs_row * 32;
    int rq_b = s_begin / a.pairs_row, rq_t = (s_begin - rq_b * a.pairs_row) * 32, rq_n = 0;
    int rq_row = rq_b * T * 16;
    const int nsteps = 2 * npairs;
    auto request = [&](int k0, int k1) {       // pieces [k0, k1) of the wave's P of stage rq_n
        const unsigned dst = wdst + (unsigned)((rq_n % WG_DMA_NSTG) * STGB);
        const bool live = rq_n < nsteps;
#pragma unroll
        for (int k = k0; k < k1; ++k) {
            const int th = BF ? (wvu & 1) : (k >> 2), cg = k & 3;
            const int tt = rq_t + 8 * th + dstep + w_shift;
            const int off = (live && tt >= 0 && tt < T) ? lane_off + rq_row + (rq_t + 8 * th) * 16 + cg * cg_off : (int)0x80000000;
            x3_dma16(rs, dst + (unsigned)(k * wgl::PIECE), off);
        }
    };
    auto advance = [&]() {
        ++rq_n;
        rq_t += 16;
        const bool wrap = rq_t >= row_steps;
        rq_t = wrap ? 0 : rq_t;
        rq_row += wrap ? T * 16 : 0;
    };
    const int trl = wgl::tr_lane(lane);
    const int a_off = wr * wgl::wave_a_off(2), b_off = BOFF + wc * wgl::wave_b_off(1);
    static_assert(wgl::wave_a_off(0) == 0 && wgl::wave_a_off(1) == 0 && wgl::wave_a_off(3) == wgl::wave_a_off(2) &&
                  wgl::wave_b_off(0) == 0 && wgl::wave_b_off(2) == 0 && wgl::wave_b_off(3) == wgl::wave_b_off(1), "wave terms of the read maps");
    auto read_frag = [&](uint4 (&f)[4][2], int k, int base, int stage) {     // wgl::wave_addr_split
        const char* st = smem + (stage % WG_DMA_NSTG) * STGB + base + wgl::piece_off(0, 0, k >> 1) + (trl ^ ((k & 1) * 64));
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl) {
            const uint2 k0 = wg_tr_read(st + pl * wgl::PLANE), k1 = wg_tr_read(st + pl * wgl::PLANE + 4 * wgl::SLOTS * 16);
            f[k][pl] = make_uint4(k0.x, k0.y, k1.x, k1.y);
        }
    };
    auto read_a = [&](int i, int stage) { read_frag(fa, i, a_off, stage); };
    auto read_b = [&](uint4 (&b)[4][2], int stage) {
#pragma unroll
        for (int j = 0; j < 4; ++j) read_frag(b, j, b_off, stage);
    };
    // The compiler does not count the requests (x3_dma16): every wait for them is written here.  Never __syncthreads() while one
    // is in flight -- its fence would drain the ring.
    auto wait_barrier = [&](auto n_c) {
        constexpr int N = decltype(n_c)::value;
        static_assert(N < 64, "vmcnt is a 6-bit counter");
        asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" :: "n"(N) : "memory");
    };
    if (npairs > 0) {
        uint4 fbn[4][2];
#pragma unroll
        for (int s = 0; s < WG_DMA_NSTG; ++s) { request(0, P); advance(); }
        wait_barrier(std::integral_constant<int, (WG_DMA_NSTG - 1) * P>{});
#pragma unroll
        for (int i = 0; i < 4; ++i) read_a(i, 0);
        read_b(fb, 0);
        // Step s (one barrier): the wait retires this wave's pieces of stage s + 1 (DEPTH newer stages stay in flight) and its
        // fragment reads of stage s; behind the barrier stage s + 1 is complete and slot s % NSTG is free, so stage s + NSTG is
        // requested into it, in four even parts, each behind a row tile's MFMAs and the refill of its A fragments from stage
        // s + 1 -- all in the shadow of stage s's MFMAs.  No conditionals in the body; the last step re-reads its own stage
        // (never used).
        // The body exists three times, chosen once in front of the loop (do_sum is block-uniform, wr wave-uniform; the waves of a
        // block meet at the barriers whichever body they run): SUMS = 0 without q sums -- two thirds of the gate batches' blocks
        // and every block of the skip halves, where the sums were formed and dropped --, SUMS = 1 / 2 with the sums of column
        // tiles 0, 1 / 2, 3 of the wave's four.
        // (flush_on is do_sum again, hidden from the compiler: with the flush behind a branch the summing body is the loop it was
        // before the bodies were split -- packed adds, 204 vector ALU instructions per pair; with the flush inline the six-layer
        // batch, whose summing blocks finish last, took 731-734 instead of 718-726 us.)
        int flush_on = __builtin_amdgcn_readfirstlane((int)do_sum);
        asm volatile("" : "+s"(flush_on));
        auto loop = [&](auto sums_c) {
            constexpr int SUMS = decltype(sums_c)::value;
            auto step = [&](const uint4 (&bc)[4][2], uint4 (&bn)[4][2], int s) {
                wait_barrier(std::integral_constant<int, WG_DMA_DEPTH * P>{});
                const int sn = s + 1 < nsteps ? s + 1 : s;
                if constexpr (SUMS != 0) {
                    constexpr int j0 = wgl::wave_sum_j(2 * (SUMS - 1), 0);
                    static_assert(wgl::wave_sum_j(2 * (SUMS - 1), 1) == j0 + 1 && wgl::wave_sum_j(2 * (SUMS - 1) + 1, 0) == j0, "the wave's summed column tiles");
                    const uint4 bs[2][2] = {{bc[j0][0], bc[j0][1]}, {bc[j0 + 1][0], bc[j0 + 1][1]}};
                    sum_frag(bs);
                }
                read_b(bn, sn);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    wg_mfma_row4<BF>(acc, fa, bc, i);
                    read_a(i, sn);
                    request(P * i / 4, P * (i + 1) / 4);
                }
                advance();
#pragma unroll
                for (int k_ = 0; k_ < (BF ? 2 : 6) * 8; ++k_) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x100 | 0x200 | 0x020, BF ? 2 : VQW_WG_DMA_PAT_MEM, 0);
                    __builtin_amdgcn_sched_group_barrier(0x002 | 0x004, VQW_WG_DMA_PAT_ALU, 0);
                }
            };
            for (int s = 0; s < nsteps; s += 2) {
                step(fb, fbn, s);
                step(fbn, fb, s + 1);
                if constexpr (SUMS != 0) {
                    if (flush_on) flush_pair(s_begin + (s >> 1));     // both stages of the pair are in qs_pair
                }
            }
        };
        if (!do_sum) loop(std::integral_constant<int, 0>{});
        else if (wr == 0) loop(std::integral_constant<int, 1>{});
        else loop(std::integral_constant<int, 2>{});
        // the requests past the last stage: nothing of the loop may be in flight when the slab stores start
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    if (do_sum && q_total) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float both = qs_tot[h] + __shfl_xor(qs_tot[h], 32, 64);
            const int row = sum_row0 + h * 32;
            if (lhi == 0 && row >= a.total_o0 && row < a.total_o1) unsafeAtomicAdd(q_total + row, both);
        }
    }
    // ---- partial tile -> slab [tile][split][256][256], rows c, columns o (32 lanes = 128 contiguous bytes): the wave's quadrant
    const float inv = __builtin_amdgcn_rcpf(scp * scq);
    float* out = a.slab + ((size_t)it.gtile * a.nsplit + split) * 65536 + (128 * wr) * 256 + 128 * wc;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int v4 = 0; v4 < 4; ++v4)
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    out[(32 * i + 8 * v4 + 4 * lhi + e) * 256 + 32 * j + l31] = acc[i][j][v4 * 4 + e] * inv;
}

// dW[tap][c][o] += sum over splits (fixed order) of the slab tiles; grid (64, tiles of all problems)
__global__ void wgrad_reduce_kernel(const WgArgs a) {
    const int gtile = blockIdx.y, cpt = a.Cp / 256, nsplit = a.nsplit;
    int w = gtile;
    const int nt = w % a.n_nt; w /= a.n_nt;
    const int rtl = w % cpt; w /= cpt;
    const int tap = w % a.ntaps, prob = w / a.ntaps;
    const int idx = (blockIdx.x * blockDim.x + threadIdx.x) * 4;     // 4 consecutive columns
    if (idx >= 65536) return;
    const int r = idx >> 8, col = idx & 255;
    const float* sp = a.slab + (size_t)gtile * nsplit * 65536 + idx;
    // four running sums (splits k = 0, 1, 2, 3 mod 4), combined at the end: a FIXED order, eight loads in flight per thread
    f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0, s2 = s0, s3 = s0;
    int k = 0;
    for (; k + 8 <= nsplit; k += 8) {
        f32x4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(sp + (size_t)(k + u) * 65536));
        s0 += v[0]; s1 += v[1]; s2 += v[2]; s3 += v[3];
        s0 += v[4]; s1 += v[5]; s2 += v[6]; s3 += v[7];
    }
    for (; k < nsplit; ++k) {
        const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(sp + (size_t)k * 65536));
        switch (k & 3) { case 0: s0 += v; break; case 1: s1 += v; break; case 2: s2 += v; break; default: s3 += v; }
    }
    const f32x4 sum = (s0 + s1) + (s2 + s3);
    float* d = a.pr[prob].dw + (size_t)tap * a.dw_tap_stride + (size_t)(rtl * 256 + r) * a.lddw + nt * 256 + col;
    f32x4 old = *reinterpret_cast<const f32x4*>(d);
    *reinterpret_cast<f32x4*>(d) = old + sum;
}

// (odd, bf, s2, qp, pp) -> the kernel and its dynamic LDS: the 13 instantiations
struct WgKernel { void (*fn)(WgArgs); int lds; };
template <bool ODD, bool BF, bool S2, bool QP, bool PP> WgKernel wg_reg() {
    return {wgrad_f16x3_kernel<ODD, BF, S2, QP, PP>, WgStage<QP, PP, BF>::BYTES * WgStage<QP, PP, BF>::STAGES};
}
template <bool BF> WgKernel wg_dma() { return {wgrad_f16x3_dma_kernel<BF>, WgDmaStage<BF>::BYTES * WgDmaStage<BF>::STAGES}; }
WgKernel wg_kernel(bool odd, bool bf, bool s2, bool qp, bool pp) {
    if (s2) return wg_reg<false, false, true, false, false>();
    if (pp && qp) return bf ? wg_dma<true>() : wg_dma<false>();
    // (p as planes: a tap's shift is a row offset -- the unaligned-window variant is not needed)
    if (pp) return bf ? wg_reg<false, true, false, false, true>() : wg_reg<false, false, false, false, true>();
    if (qp) return odd ? (bf ? wg_reg<true, true, false, true, false>() : wg_reg<true, false, false, true, false>())
                       : (bf ? wg_reg<false, true, false, true, false>() : wg_reg<false, false, false, true, false>());
    return odd ? (bf ? wg_reg<true, true, false, false, false>() : wg_reg<true, false, false, false, false>())
               : (bf ? wg_reg<false, true, false, false, false>() : wg_reg<false, false, false, false, false>());
}

}  // namespace

extern "C" {

int vqw_f16x3_wgrad_batch(const vqw_f16x3_wgrad_desc* dp, int nprob, vqw_stream_t s_) {
    hipStream_t st = (hipStream_t)s_;
    VQW_CHECK(dp, "vqw_f16x3_wgrad: null descriptor");
    VQW_CHECK(nprob >= 1 && nprob <= WG_MAX_BATCH, "vqw_f16x3_wgrad_batch: 1..%d problems per launch (got %d)", WG_MAX_BATCH, nprob);
    const vqw_f16x3_wgrad_desc& d = dp[0];
    VQW_CHECK(d.slab, "vqw_f16x3_wgrad: null operand");
    VQW_CHECK(d.B > 0 && d.T > 0 && (d.T % 32 == 0 || (d.p_stride == 2 && d.T % 4 == 0) || (d.p_planes && d.q_planes && !d.q_seg)),
              "vqw_f16x3_wgrad: T must be a positive multiple of 32 (of 4 with p_stride 2; any with both operands as planes) (got %d)", d.T);
    VQW_CHECK(d.Cp > 0 && d.Cp % 256 == 0 && d.Q0 > 0 && d.Q0 % 256 == 0 && d.Q1 >= 0 && d.Q1 % 256 == 0,
              "vqw_f16x3_wgrad: Cp, Q0, Q1 must be multiples of 256 (Cp=%d Q0=%d Q1=%d)", d.Cp, d.Q0, d.Q1);
    VQW_CHECK(d.ntaps >= 1 && d.ntaps <= VQW_MAX_TAPS, "vqw_f16x3_wgrad: 1..%d taps", VQW_MAX_TAPS);
    VQW_CHECK(d.p_stride == 0 || d.p_stride == 1 || d.p_stride == 2, "vqw_f16x3_wgrad: p_stride is 1 or 2 (got %d)", d.p_stride);
    const bool s2 = d.p_stride == 2;
    const int Tp = s2 ? d.Tp : d.T;
    VQW_CHECK(!s2 || (Tp > 0 && !(d.mode & 1)), "vqw_f16x3_wgrad: p_stride 2 needs Tp > 0 and the fp16x3 mode (Tp=%d mode=%d)", Tp, d.mode);
    const size_t pbytes = (size_t)d.B * d.Cp * Tp * 4, qbytes = (size_t)d.B * (d.Q0 > d.Q1 ? d.Q0 : d.Q1) * d.T * 4;
    VQW_CHECK(pbytes < ((size_t)1 << 31) && qbytes < ((size_t)1 << 31), "vqw_f16x3_wgrad: operands exceed 2 GiB");
    const int lddw = d.lddw > 0 ? d.lddw : d.Q0 + d.Q1;
    VQW_CHECK(lddw >= d.Q0 + d.Q1 && lddw % 4 == 0, "vqw_f16x3_wgrad: lddw must be a multiple of 4 and >= Q0 + Q1");
    VQW_CHECK(d.mode >= 0 && d.mode <= 3, "vqw_f16x3_wgrad: mode is a bit set of VQW_X3_BF16 | VQW_X3_HALF_BLOCKS (the latter has no effect here)");
    WgArgs a;
    memset(&a, 0, sizeof(a));
    bool odd = false;
    for (int i = 0; i < nprob; ++i) {
        const vqw_f16x3_wgrad_desc& e = dp[i];
        // one shape per launch: only the operands, scales, sums, tap shifts and the output differ between the problems
        VQW_CHECK(e.B == d.B && e.T == d.T && e.Cp == d.Cp && e.Q0 == d.Q0 && e.Q1 == d.Q1 && e.ntaps == d.ntaps && e.lddw == d.lddw &&
                  e.dw_tap_stride == d.dw_tap_stride && e.seg_bstride == d.seg_bstride && e.seg_T == d.seg_T && e.total_o0 == d.total_o0 &&
                  e.total_o1 == d.total_o1 && e.mode == d.mode && e.p_relu == d.p_relu && e.p_stride == d.p_stride && e.Tp == d.Tp &&
                  e.slab == d.slab && (e.q_seg != nullptr) == (d.q_seg != nullptr),
                  "vqw_f16x3_wgrad_batch: problem %d differs from problem 0 in shape or layout", i);
        VQW_CHECK((e.p || e.p_planes) && (e.q0 || e.q_planes) && e.dw && (e.Q1 == 0 || e.q1), "vqw_f16x3_wgrad: null operand (problem %d)", i);
        VQW_CHECK((e.q_planes != nullptr) == (d.q_planes != nullptr) && (e.p_planes != nullptr) == (d.p_planes != nullptr),
                  "vqw_f16x3_wgrad_batch: an operand as planes in every problem or in none");
        if (e.p_planes) {
            const int kc = e.p_planes_KC > 0 ? e.p_planes_KC : d.Cp / 8;
            for (int j = 0; j < d.ntaps; ++j)
                VQW_CHECK(e.p_planes_kc0 >= 0 && e.p_tap_chunk[j] >= 0 && e.p_planes_kc0 + e.p_tap_chunk[j] + d.Cp / 8 <= kc,
                          "vqw_f16x3_wgrad: bad chunk range of the p planes (kc0=%d tap %d chunk offset %d KC=%d)", e.p_planes_kc0, j, e.p_tap_chunk[j], kc);
        }
        if (e.q_planes) {
            const int kc = e.q_planes_KC > 0 ? e.q_planes_KC : d.Q0 / 8;
            VQW_CHECK(e.q_planes_kc0 >= 0 && e.q_planes_kc0 + d.Q0 / 8 <= kc, "vqw_f16x3_wgrad: bad chunk range of the q planes (kc0=%d KC=%d)", e.q_planes_kc0, kc);
        }
        VQW_CHECK((reinterpret_cast<uintptr_t>(e.dw) & 15u) == 0, "vqw_f16x3_wgrad: dw must be 16-byte aligned (problem %d)", i);
        WgProblem& q = a.pr[i];
        q.p = e.p; q.q0 = e.q0; q.q1 = e.q1; q.dw = e.dw; q.sp = e.p_scale; q.sq0 = e.q0_scale; q.sq1 = e.q1_scale;
        q.q_total = e.q_total; q.q_seg = e.q_seg;
        q.qp = e.q_planes; q.q_KC = e.q_planes_KC > 0 ? e.q_planes_KC : d.Q0 / 8; q.q_kc0 = e.q_planes_kc0;
        q.q_hscale = e.q_planes_scale > 0.0f ? e.q_planes_scale : 1.0f;
        q.pp = e.p_planes; q.p_KC = e.p_planes_KC > 0 ? e.p_planes_KC : d.Cp / 8; q.p_kc0 = e.p_planes_kc0;
        q.p_hscale = e.p_planes_scale > 0.0f ? e.p_planes_scale : 1.0f;
        for (int j = 0; j < d.ntaps; ++j) {
            VQW_CHECK(((s2 || e.p_planes) ? e.tap_shift[j] < (1 << 24) : e.tap_shift[j] <= 0) && e.tap_shift[j] > -(1 << 24),
                      "vqw_f16x3_wgrad: tap shifts must be <= 0 unless p_stride is 2 or p comes as planes (problem %d, tap %d: %d)", i, j, e.tap_shift[j]);
            q.shift[j] = e.tap_shift[j];
            q.pkoff[j] = e.p_planes ? e.p_tap_chunk[j] : 0;
            odd |= (e.tap_shift[j] & 3) != 0;
        }
    }
    a.slab = d.slab; a.nprob = nprob;
    a.B = d.B; a.T = d.T; a.Cp = d.Cp; a.Q0 = d.Q0; a.Q1 = d.Q1; a.ntaps = d.ntaps; a.Tp = Tp; a.p_relu = d.p_relu;
    a.pairs_row = (d.T + 31) / 32; a.pairs_total = d.B * a.pairs_row;
    a.n_nt = (d.Q0 + d.Q1) / 256;
    const int tiles = nprob * d.ntaps * (d.Cp / 256) * a.n_nt;
    int nsplit = d.nsplit > 0 ? d.nsplit : vqw_device_cus() / tiles;     // one round of blocks
    if (nsplit < 1) nsplit = 1;
    if (nsplit > a.pairs_total) nsplit = a.pairs_total;
    a.nsplit = nsplit;
    a.seg_bstride = (long)d.seg_bstride; a.seg_T = d.seg_T;
    a.total_o0 = d.total_o0; a.total_o1 = d.total_o1 > 0 ? d.total_o1 : d.Q0 + d.Q1;
    a.seg_ratio = 1;
    if (d.q_seg) {
        VQW_CHECK(d.seg_T > 0 && d.T % d.seg_T == 0 && (d.T / d.seg_T) % 32 == 0 && d.seg_bstride >= (int64_t)(d.Q0 + d.Q1) * d.seg_T,
                  "vqw_f16x3_wgrad: q_seg needs T / seg_T to be a multiple of 32 (T=%d seg_T=%d)", d.T, d.seg_T);
        a.seg_ratio = d.T / d.seg_T;
    }
    a.lddw = lddw;
    a.dw_tap_stride = d.dw_tap_stride > 0 ? (long)d.dw_tap_stride : (long)d.Cp * lddw;
    VQW_CHECK((size_t)tiles * nsplit * 65536 <= (size_t)d.slab_floats, "vqw_f16x3_wgrad: slab too small (%d tiles x %d splits x 65536 floats)", tiles, nsplit);
    const bool qp = d.q_planes != nullptr, pp = d.p_planes != nullptr, bf = (d.mode & 1) != 0;
    VQW_CHECK(!qp || (!s2 && d.Q1 == 0 && (size_t)32 * d.B * d.T * 16 < ((size_t)1 << 31)),
              "vqw_f16x3_wgrad: q as planes needs p_stride 1, Q1 = 0 and B * T < 4 M");
    VQW_CHECK(!pp || (!s2 && !d.p_relu && (size_t)32 * d.B * d.T * 16 < ((size_t)1 << 31)),
              "vqw_f16x3_wgrad: p as planes needs p_stride 1, no p_relu and B * T < 4 M");
    const WgKernel k = wg_kernel(odd, bf, s2, qp, pp);
    if (const int rc = x3_launch(k.fn, tiles * nsplit, k.lds, st, a, "vqw_f16x3_wgrad")) return rc;
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(65536 / 4 / 256, tiles), dim3(256), 0, st, a);
    VQW_LAUNCH_CHECK("vqw_f16x3_wgrad");
    return 0;
}

int vqw_f16x3_wgrad(const vqw_f16x3_wgrad_desc* dp, vqw_stream_t s_) { return vqw_f16x3_wgrad_batch(dp, 1, s_); }

}  // extern "C"
