// The fp16x3 engine: every contraction of the decoder's residual stack -- the gate conv
// (wavenet_ops.py:104-114), the 1x1 residual conv (:135-136), the skip path of all layers as ONE contraction (:132-133,
// wavenet.py:72), gate backward, the gate conv's input gradient and both weight gradients -- as fp32-accurate
// contractions on the fp16 matrix pipe of gfx950: every fp32 operand is split into two fp16 pieces, x = h1 + h2,
// h2 = fp16(x - h1), and  a*b ~ a1 b1 + a1 b2 + a2 b1  (every term exact in the fp32 accumulator of
// v_mfma_f32_32x32x16_f16; the dropped a2 b2 is 2^-22 per product).  Same bytes per operand element as fp32, three
// MFMAs of the fast pipe instead of eight fp32 ones per 32x32x16 block.  Device-side range guards (power-of-two scales
// from measured max-abs values, a range flag) keep the leading planes inside fp16; the same kernels instantiated with
// one bf16 plane and one bf16 MFMA per product are the bf16 engine of BASELINE.json configs[4].
// This header: what more than one of the five sources uses -- f16x3_planes.hip (operand planes, range-guard scales),
// f16x3_conv.hip (gate / out / head convs), f16x3_gate_bwd.hip, f16x3_sconv.hip (stride-2 convs), f16x3_wgrad.hip.
//
// Conv kernels: block = 256 (or 128) output rows x 256 time steps, four waves of all rows x 64 time steps (16 or 8
// accumulator tiles); K step = 16 input channels of one tap; operands by LDS-DMA into an LDS ring, one barrier per
// step, the MFMAs issued with the step's memory instructions interleaved behind them (f16x3_mainloop).
#pragma once
#include <type_traits>

#include "vqw_common.h"

namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned short u16;

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ u16 f16_bits(_Float16 h) { return __builtin_bit_cast(u16, h); }
__device__ __forceinline__ u16 bf16_bits(float x) { return __builtin_bit_cast(u16, (__bf16)x); }   // round to nearest even
// BF (every template below): the bf16 engine -- ONE bf16 plane per operand, one v_mfma_f32_32x32x16_bf16 per product
// (bf16 storage + fp32 accumulate, BASELINE.json configs[4]) instead of two fp16 planes and three fp16 MFMA terms.
template <bool BF = false>
__device__ __forceinline__ void split8(const float (&x)[8], uint4& p0, uint4& p1) {
    u16 a[8], b[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        if (BF) { a[e] = bf16_bits(x[e]); b[e] = 0; continue; }
        // Both pieces come from ONE fp32 value the compiler cannot look through: left to itself it rounds the caller's scale * x once more
        // as v_fma_mixlo_f16(scale, x, 0) for the residual of two of the eight elements, and (-0) * scale + 0 = +0 makes the residual
        // of x = -0 come out as -0 there instead of +0 (tests/test_x3_range_gpu.py, plane bytes).  No instruction is emitted.
        float xe = x[e];
        asm volatile("" : "+v"(xe));
        const _Float16 h1 = (_Float16)xe;              // round to nearest even
        a[e] = f16_bits(h1);
        b[e] = f16_bits((_Float16)(xe - (float)h1));   // the difference is exact in fp32
    }
    p0 = make_uint4(a[0] | ((unsigned)a[1] << 16), a[2] | ((unsigned)a[3] << 16), a[4] | ((unsigned)a[5] << 16), a[6] | ((unsigned)a[7] << 16));
    p1 = make_uint4(b[0] | ((unsigned)b[1] << 16), b[2] | ((unsigned)b[3] << 16), b[4] | ((unsigned)b[5] << 16), b[6] | ((unsigned)b[7] << 16));
}

// ---- range guards: the leading plane of scale * x must stay inside fp16 (|.| <= 65504).  Scales are
// powers of two held in DEVICE memory (chosen from measured max-abs values, vqw_f16x3_update_scales); a kernel that
// writes planes reports the max-abs of its fp32 values (atomicMax on the bit pattern: monotonic for non-negative
// floats) and raises `flag` when an element leaves the range or is not finite -- the host then repeats the step on the
// fp32 engine.
constexpr float F16_MAX = 65504.0f;
__device__ __forceinline__ float dev_scale(const float* p) { return p ? *p : 1.0f; }
// 1 / (sa * sb) for powers of two (v_rcp_f32 is exact on them)
__device__ __forceinline__ float inv_scales(float host_inv, const float* sa, const float* sb) {
    return (sa || sb) ? host_inv * __builtin_amdgcn_rcpf(dev_scale(sa) * dev_scale(sb)) : host_inv;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
// called by all lanes of a wave: amax of the wave's fp32 values (`m`, NaN-propagating through `bad`), range check of m * ps
__device__ __forceinline__ void guard_report(float m, bool bad, float ps, unsigned* amax, int* flag) {
    if (!amax && !flag) return;
    const float wm = wave_max(m);
    const bool wbad = __any(bad || !(m * ps <= F16_MAX));
    if ((threadIdx.x & 63) == 0) {
        // look before the atomic: tens of thousands of waves hitting ONE address serialise (53 k contended atomics cost
        // ~300 us); after the first few, a plain (L2-coherent) read shows a value that is already at least as large
        const unsigned bits = __float_as_uint(wm);
        if (amax && bits > __hip_atomic_load(amax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(amax, bits);
        if (flag && wbad) atomicOr(flag, 1);
    }
}

// LDS-DMA of the conv main loop: 16 bytes per lane from raw buffer `rsrc` (as vqw_make_rsrc builds it) at byte offset `voff` into
// the 1 KiB of LDS at the wave-uniform byte address `lds_dst` (lane i lands at + 16 i; an out-of-range lane gets zeros).  As inline
// assembly and not through vqw_buf_load_lds16: the compiler orders every LDS read behind every LDS-DMA it knows of -- an
// `s_waitcnt vmcnt(0)` in front of the first ds_read that follows a request, which would empty the ring in every K step.  Hidden
// from it the requests are ordered by f16x3_mainloop's own counted waits and barriers.  M0 (the destination) is the compiler's
// register: written and restored inside the statement.
__device__ __forceinline__ void x3_dma16(u32x4 rsrc, unsigned lds_dst, int voff) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tbuffer_load_dwordx4 %2, %3, 0 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "s"(lds_dst), "v"(voff), "s"(rsrc) : "memory");
}
__device__ __forceinline__ u32x4 x3_rsrc_words(const void* p, unsigned bytes) {
    const size_t a = reinterpret_cast<size_t>(p);
    return u32x4{(unsigned)a, (unsigned)(a >> 32) & 0xffffu, bytes, 0x00020000u};      // stride 0, raw: offsets are checked against `bytes`
}

struct OutArgs {
    vqw_f16x3_out_desc d;
    int NB;
};

#ifndef VQW_X3_TAP_MINOR
#define VQW_X3_TAP_MINOR 1      // K order of the conv main loop (0: taps outermost, as in round 1)
#endif
#ifndef VQW_X3_PAT_MEM
#define VQW_X3_PAT_MEM 1      // issue pattern of the conv main loop: LDS / global-memory instructions per MFMA ...
#define VQW_X3_PAT_ALU 2      // ... and address computations per MFMA (tools/x3_bench.py: 1/2 measured best)
#endif

// Geometry of one block's contraction: 256 weight rows from row m_row0 of planes with M rows, K = ks taps x Cin
// input channels, 256 activation rows from row n0 (time t0 of its batch row) of planes with NB rows.
struct LoopGeom {
    const void* wp;
    const void* xp;
    int M, Cin, ks, dilation, NB, m_row0, n0, t0;
    int xKC, xkc0;   // chunks per plane of xp and the first chunk of this contraction (planes may hold more channels)
    int dir, T;      // dir > 0: tap j reads x[t - (ks-1-j) d] (causal conv); dir < 0: x[t + (ks-1-j) d] (its input gradient)
    // TAB (stride-2 convs, encoder.py:17-18): the loop's tap i is tap j = tj0 + tjstep * i of a kernel with `wks` taps (the weight
    // planes hold all of them); with e = j - toff it reads activation row t - tsgn * (e >> 1) of chunk block (ts2d ? e & 1 : 0):
    //   forward over space-to-depth planes (chunk block = parity of the input sample): tsgn = -1, toff = pad_left, ts2d = 1;
    //   input gradient of output parity r: tj0 = (r + pad_left) & 1, tjstep = 2, toff = r + pad_left, tsgn = +1, ts2d = 0.
    // n0 may lie anywhere in the flat (batch, time) row space: rows outside the lane's own batch row read as zero.
    int wks, tj0, tjstep, toff, tsgn, ts2d;
    int sb, sn;      // TAB: this block's K steps [sb, sb + sn) of the ks * Cin / 16 (split-K of the short encoder layers); sn even
};

// acc[i][j] += W[m_row0 + 32 i .., :] X[:, n0 + 64 wv + 32 j ..]: MR x 2 accumulator tiles per wave, operands by LDS-DMA
// into an LDS ring, one barrier per K step of 16.
//   MR = 8: block = 256 rows x 256 columns, 16 accumulator tiles (256 AGPRs) per wave, one block per CU, 4 LDS stages of
//           32 KiB, three stages of requests in flight.
//   MR = 4: block = 128 rows x 256 columns, 8 accumulator tiles per wave, 256 registers per wave => TWO blocks per CU
//           (3 stages of 24 KiB each, two stages of requests in flight): while one block is in its HBM-bound epilogue (all blocks of a one-block-per-CU
//           grid reach it together: gate backward spent 64 % of its time there) the other block's MFMAs run; each weight
//           panel is read by twice as many blocks (all of the loop's data movement is 16 % of the MR = 8 kernel).
// Two blocks that share a CU start together and would reach their epilogues together; the blocks of every second
// batch of `CUs` block ids wait a fraction of a main loop first, so that one block stores while the other multiplies.
#ifndef VQW_X3_STAGGER
#define VQW_X3_STAGGER 0      // in units of 8128 cycles (~3.7 us)
#endif
__device__ __forceinline__ void x3_stagger(int n) {
    if (VQW_X3_STAGGER > 0 && ((blockIdx.x >> 8) & 1))
        for (int i = 0; i < n; ++i) __builtin_amdgcn_s_sleep(127);
}
template <int MR> struct X3Shape {
    static constexpr int NSTAGE = MR == 8 ? 4 : 3;
    static constexpr int STAGE_BYTES = (MR * 2 + 16) * 1024;     // MR*2 weight pieces + 16 activation pieces of 1 KiB
    static constexpr int LDS_BYTES = NSTAGE * STAGE_BYTES;
    static constexpr int DEPTH = MR == 8 ? 2 : 1;                 // stages of requests left in flight across a step's barrier
};
template <bool BF, int MR, bool TAB = false, int DEPTH = X3Shape<MR>::DEPTH>
__device__ __forceinline__ void f16x3_mainloop(f32x16 (&acc)[MR][2], char* smem, const LoopGeom& g, int wv_, int lane_) {
    // The loop's own copies of the wave and lane index.  The callers' are live from the top of the kernel to the end of the epilogue;
    // used in here as well they get a register of the loop's choosing, which the epilogues -- 256 + 256 registers, every one taken --
    // then spill (8 bytes of scratch in the 256-row head conv, 4 more in the bf16 gate conv).
    int wv = wv_, lane = lane_;
    asm volatile("" : "+v"(wv), "+v"(lane));
    constexpr int NP = BF ? 1 : 2;        // planes per operand
    constexpr int NA = MR * NP / 4, NBP = 2 * NP;      // weight / activation pieces a wave moves per step
    if (MR == 4) x3_stagger(VQW_X3_STAGGER);
    constexpr int NSTG_ = DEPTH + 2, STGB = X3Shape<MR>::STAGE_BYTES, BOFF = MR * 2 * 1024;      // (a stage is requested DEPTH + 1 steps before it is read)
    const int l31 = lane & 31, lhi = lane >> 5;
    const int KCA = (TAB ? g.wks : g.ks) * g.Cin / 8, KCB = g.Cin / 8, spt = g.Cin / 16;   // spt: K steps per tap
    // Live taps (not TAB): a tap whose shift puts every one of the block's 256 columns before its batch row (causal padding; behind
    // it for an input gradient) multiplies nothing but zeros -- all of its Cin / 16 steps would request zeros, read them and issue
    // their MFMAs.  Such taps are left out of the K range: `live` lists the others in ascending order, four bits each (ks <= 8 is
    // checked by the callers), and a step looks its tap up by shifting that scalar.  The result keeps its bits: the accumulators
    // start at +0, the weights are finite, and a skipped step would have added products with an all-zero B fragment -- zeros of
    // either sign, which leave an accumulator that is not -0 as it is (and none ever becomes -0: that takes two -0 addends).  The
    // steps that remain run in the order they had.  The tap with shift 0 is always live: n_live >= 1, nsteps stays even with spt.
    unsigned live = 0;
    int n_live = 0;
    if constexpr (!TAB) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int sh = (g.ks - 1 - j) * g.dilation * (g.dir < 0 ? -1 : 1);
            const bool on = j < g.ks && g.t0 + 255 - sh >= 0 && g.t0 - sh < g.T;
            live |= on ? (unsigned)j << (4 * n_live) : 0u;
            n_live += on ? 1 : 0;
        }
        // (block-uniform by construction; said so, the list and its length sit in scalar registers whatever unit built them)
        live = __builtin_amdgcn_readfirstlane(live);
        n_live = __builtin_amdgcn_readfirstlane(n_live);
    }
    const int nsteps = TAB ? g.sn : n_live * spt;
    // Weight resource `ra` (below): NP planes -- the requests past the last K step must fall outside the resource, and read as zero,
    // in bf16 mode too, where the weight planes end after ONE plane.
    // One buffer resource per activation plane, based at the contraction's first chunk: 32-bit offsets then only span the
    // chunks this contraction reads (checked by the callers: Cin / 8 * NB * 16 < 2 GiB), not the planes tensor -- the gated planes
    // of all layers side by side are 3.3 GB at batch 16 and neither their size nor the distance between the two planes may
    // decide whether the engine can run.
    const size_t plane_bytes = (size_t)g.xKC * g.NB * 16, span = (size_t)(g.xKC - g.xkc0) * g.NB * 16;
    const char* xbase = reinterpret_cast<const char*>(g.xp) + (size_t)g.xkc0 * g.NB * 16;
    const unsigned xspan = span < 0x7fffffffu ? (unsigned)span : 0x7fffffffu;
    // Stage image: MR*2 weight pieces (row tile i, plane p at (i * 2 + p) KiB), then 16 activation pieces.  lane = (k half, row)
    // as the MFMA wants it.
    int voffA[NA], voffB[NBP], trow[NBP];
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const int q = wv * NA + i, tile = q / NP, p = q % NP;
        voffA[i] = ((p * KCA + lhi) * g.M + g.m_row0 + tile * 32 + l31) * 16;
    }
#pragma unroll
    for (int i = 0; i < NBP; ++i) {
        const int tile = (wv * NBP + i) / NP;
        voffB[i] = (lhi * g.NB + g.n0 + tile * 32 + l31) * 16;      // (plane p = i % NP: its own resource)
        trow[i] = TAB ? (g.n0 + tile * 32 + l31) % g.T : g.t0 + tile * 32 + l31;      // time of this lane's activation row
    }
    // Stage s: global -> LDS by LDS-DMA (x3_dma16: no VGPRs, no ds_write).  A 1-KiB piece is the lane-linear image one such
    // instruction writes (wave-uniform base + 16 * lane); a lane whose row lies before / behind its batch row (causal, batch-boundary
    // and stride-2 padding) or past the end of the planes requests an out-of-range offset and gets zeros in its 16 bytes of LDS,
    // as it would in a VGPR.  Piece q of the wave's P = NA + NBP: weights first.
    constexpr int P = NA + NBP;
    const u32x4 ra = x3_rsrc_words(g.wp, (unsigned)((size_t)NP * KCA * g.M * 16));
    const u32x4 rb0 = x3_rsrc_words(xbase, xspan), rb1 = x3_rsrc_words(xbase + (NP > 1 ? plane_bytes : 0), xspan);
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
    const int wvu = __builtin_amdgcn_readfirstlane(wv);
    struct StageReq { int woff, xoff, shift; unsigned dst; };
    auto stage_req = [&](int s_) {
        const int s = TAB ? s_ + g.sb : s_;
#if VQW_X3_TAP_MINOR
        // K order: channel chunk outermost, taps innermost -- the taps of one chunk read the same activation lines a few rows apart,
        // in consecutive steps instead of Cin / 16 steps apart, while they are still in L2 (HBM reads of the gate conv d=8: 172 -> 104 MB)
        const int ji = TAB ? s / spt : s % n_live, kc = TAB ? (s - ji * spt) * 2 : (s / n_live) * 2;
#else
        const int ji = s / spt, kc = (s - ji * spt) * 2;
#endif
        const int j = TAB ? g.tj0 + g.tjstep * ji : (int)((live >> ((4 * ji) & 31)) & 7u);      // (past the last step: any tap, into a slot nobody reads)
        const int e_ = TAB ? j - g.toff : 0;
        const int shift = TAB ? g.tsgn * (e_ >> 1) : (g.ks - 1 - j) * g.dilation * (g.dir < 0 ? -1 : 1);   // rows before / behind the batch row read as zero
        const int kcx = TAB ? kc + (g.ts2d ? (e_ & 1) * KCB : 0) : kc;
        return StageReq{(j * KCB + kc) * g.M * 16, (kcx * g.NB - shift) * 16, shift, lds0 + (unsigned)((s_ % NSTG_) * STGB)};
    };
    auto dma_piece = [&](const StageReq& r, int q) {
#ifndef VQW_ABL_NODMA
        if (q < NA) {
            const int w = wvu * NA + q;
            x3_dma16(ra, r.dst + (unsigned)((w / NP * 2 + w % NP) * 1024), voffA[q] + r.woff);
        } else {
            const int i = q - NA, w = wvu * NBP + i, tr = trow[i] - r.shift;
            const int vb = (tr >= 0 && tr < g.T) ? voffB[i] + r.xoff : (int)0x80000000;   // out of range -> 0
            // (wv * NBP is even: plane = i % NP at compile time)
            x3_dma16((i % NP) ? rb1 : rb0, r.dst + (unsigned)(BOFF + (w / NP * 2 + w % NP) * 1024), vb);
        }
#endif
    };
    // Fragments: ONE set of A fragments (MR row tiles x NP planes) that is refilled row tile by row tile -- right behind the
    // MFMAs of a row tile its fragments of the NEXT stage are fetched from LDS, a whole step before they are used -- and two
    // sets of this wave's B fragments.
    uint4 fa[MR][NP], fb[2][NP], fbn[2][NP];
    auto read_a = [&](int i, int s) {
        const char* st = smem + (s % NSTG_) * STGB + lane * 16;
#pragma unroll
        for (int p = 0; p < NP; ++p) fa[i][p] = *reinterpret_cast<const uint4*>(st + (i * 2 + p) * 1024);
    };
    auto read_b = [&](uint4 (&b)[2][NP], int s) {
        const char* st = smem + (s % NSTG_) * STGB + lane * 16 + BOFF;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int p = 0; p < NP; ++p) b[j][p] = *reinterpret_cast<const uint4*>(st + ((wv * 2 + j) * 2 + p) * 1024);
    };
#pragma unroll
    for (int i = 0; i < MR; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    // Two row tiles x two column tiles at a time, the three terms outermost (small terms first): an MFMA that accumulates
    // into the same tile as its predecessor waits for that one's whole latency, so the four independent accumulators are
    // rotated through between two terms of the same tile.
    auto mfma_rows = [&](int i, const uint4 (&b)[2][NP]) {
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
                    const int pa = term == 1 ? 1 : 0, pb = term == 0 ? 1 : 0;      // h1 h2, h2 h1, h1 h1
                    acc[ii][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, fa[ii][pa]), __builtin_bit_cast(f16x8, b[j][pb]), acc[ii][j], 0, 0, 0);
                }
        }
    };

    // P requests per wave and stage.  All NSTG_ = DEPTH + 2 slots of the ring are requested up front; the counted wait before a
    // stage is read leaves the wave's newer stages in flight (NSTG_ - 1 here, DEPTH in the loop), the raw barrier behind it
    // covers the other waves' pieces.  The compiler does not count these requests (x3_dma16): every wait for them is written here.
    auto wait_barrier = [&](auto n_c) {
        constexpr int N = decltype(n_c)::value;
        static_assert(N < 64, "vmcnt is a 6-bit counter");
        asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" :: "n"(N) : "memory");
    };
#pragma unroll
    for (int s = 0; s < NSTG_; ++s) {
        const StageReq r = stage_req(s);
#pragma unroll
        for (int q = 0; q < P; ++q) dma_piece(r, q);
    }
    wait_barrier(std::integral_constant<int, (NSTG_ - 1) * P>{});
#pragma unroll
    for (int i = 0; i < MR; ++i) read_a(i, 0);
    read_b(fb, 0);
    // One step s (one barrier).  The wait retires this wave's pieces of stage s + 1 (the DEPTH stages requested after it stay in
    // flight) and the fragment reads of stage s it issued in step s - 1; behind the barrier stage s + 1 is therefore complete in
    // LDS and the slot of stage s is free (every wave's fragments of it are in registers): stage s + NSTG_ is requested into that
    // slot -- DEPTH + 1 steps before it is read -- and the MFMAs of stage s run row-tile pair by row-tile pair with the LDS reads
    // of stage s + 1 behind them.  nsteps is even (Cin % 32 == 0 is checked by the callers).
    auto step = [&](const uint4 (&bc)[2][NP], uint4 (&bn)[2][NP], int s) {
        wait_barrier(std::integral_constant<int, DEPTH * P>{});
        const int sn = s + 1 < nsteps ? s + 1 : s;          // (the last step re-reads its own stage: no branch in the body)
        // No conditionals in the body (they would cut it into scheduling regions): the requests past the last stage land in
        // slots nobody reads again (the last step's own re-read is never used), from wherever their addresses point -- past the
        // end of the weight planes raw buffer loads return zero.
        // (VQW_ABL_*: timing ablations, wrong results, never shipped -- which of the data paths bounds the loop)
#ifndef VQW_ABL_NOLDSREAD
        read_b(bn, sn);
#endif
        const StageReq r = stage_req(s + NSTG_);
#pragma unroll
        for (int i = 0; i < MR; i += 2) {
            mfma_rows(i, bc);
#ifndef VQW_ABL_NOLDSREAD
            read_a(i, sn);
            read_a(i + 1, sn);
#endif
            // the wave's P requests in MR / 2 even parts, one behind the fragment reads of each row-tile pair: inline asm keeps its
            // place among the LDS reads, which the issue pattern below spreads over the MFMAs
#pragma unroll
            for (int q = P * (i / 2) / (MR / 2); q < P * (i / 2 + 1) / (MR / 2); ++q) dma_piece(r, q);
        }
        // issue order: one MFMA, then one LDS / global-memory instruction and a few address computations in its shadow
#pragma unroll
        for (int k_ = 0; k_ < (BF ? 2 : 6) * MR; ++k_) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x100 | 0x200 | 0x020, BF ? 2 : VQW_X3_PAT_MEM, 0);
            __builtin_amdgcn_sched_group_barrier(0x002 | 0x004, VQW_X3_PAT_ALU, 0);
        }
    };
    for (int s = 0; s < nsteps; s += 2) {
        step(fb, fbn, s);
        step(fbn, fb, s + 1);
    }
    // the requests past the last stage: nothing of the loop may be in flight when the epilogue starts counting its own loads (or
    // when an input gradient's second run refills the ring)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// Epilogue request depth.  An epilogue works through NG groups -- four channels x two column tiles per lane -- and each
// group reads operands from memory (old value, bias, condition, mask, saved activations) before it stores.  Outputs may alias
// inputs by contract, so the compiler keeps every load behind the stores written before it; loads and stores share vmcnt and
// retire in issue order, so a wave that loads, computes and stores one group at a time has one group of requests in flight and
// pays a memory round trip plus a store acknowledge per group.  Here the operands of group g + DEPTH are requested BEFORE group g is
// computed and stored: the wait for group g + 1 then leaves the stores of g and the loads of g + 2 outstanding.
// Aliasing stays legal: every element is read and written by the same lane in the same group, and groups touch disjoint
// elements, so a load hoisted over the stores of earlier groups never reads an element one of those stores writes.
// The prefetch buffers are named values rotated by hand -- never an array indexed by the group -- and the loop unrolls fully.
template <int NG, int DEPTH, typename Ops, typename Req, typename Fin>
__device__ __forceinline__ void x3_epilogue_pipeline(Req&& request, Fin&& finish) {
    static_assert(NG % 2 == 0 && DEPTH >= 0 && DEPTH <= 2, "two named buffers");
    Ops p0, p1;
    request(0, p0);
    if constexpr (DEPTH == 0) {      // (no prefetch: a group is requested, computed and stored before the next one)
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            if (g > 0) request(g, p0);
            finish(g, p0);
        }
    } else if constexpr (DEPTH == 2) {
        request(1, p1);
#pragma unroll
        for (int g = 0; g < NG; g += 2) {
            { const Ops c = p0; if (g + 2 < NG) request(g + 2, p0); finish(g, c); }
                { const Ops c = p1; if (g + 3 < NG) request(g + 3, p1); finish(g + 1, c); }
            }
    } else {
#pragma unroll
        for (int g = 0; g < NG; g += 2) {
            request(g + 1, p1);
            finish(g, p0);
                if (g + 2 < NG) request(g + 2, p0);
            finish(g + 1, p1);
            }
    }
}
// An optional operand that is absent reads a valid dummy address and is then taken as +0: as a bit mask, not as a select on the
// block-uniform "is it there" condition -- the optimiser turns such a select into a branch around the load, and the merge behind
// the branch waits for the load right where it was issued (vmcnt(0) after every single load of a prefetched group).
__device__ __forceinline__ unsigned x3_present(bool present) {
    unsigned m = __builtin_amdgcn_readfirstlane(present ? 0xffffffffu : 0u);
    asm volatile("" : "+s"(m));      // (opaque: not to be recognised as a select again)
    return m;
}
__device__ __forceinline__ float x3_masked(float v, unsigned m) { return __uint_as_float(__float_as_uint(v) & m); }
__device__ __forceinline__ int x3_masked(int i, unsigned m) { return (int)((unsigned)i & m); }      // (the index of an absent operand: 0)
// The max-abs / finiteness folds of a group are pinned where they are written: left alone, the optimiser sinks them into the
// conditional guard_report at the end of the kernel and keeps every value of the whole epilogue alive until then (spills).
__device__ __forceinline__ void x3_pin_guard(float& gmax, bool& gbad) {
    int gb_i = (int)gbad;
    asm volatile("" : "+v"(gmax), "+v"(gb_i));
    gbad = gb_i != 0;
}
#ifndef VQW_X3_EPI_DEPTH
#define VQW_X3_EPI_DEPTH 2
#endif
constexpr int EPI_DEPTH = VQW_X3_EPI_DEPTH;

// Four consecutive channels (rows 4 lhi .. 4 lhi + 3 of chunk kc) of one (batch, time) row as the lane's 8-byte
// half of the 16-byte plane entries: the 64 lanes of a wave cover 32 rows x 16 bytes = 512 contiguous bytes per plane.
template <bool BF>
__device__ __forceinline__ void store_plane_quad(void* planes, int KC, int NB, int kc, int row, int lhi, const float (&x)[4], float scale = 1.0f) {
    u16 h1[4], h2[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float xs = x[e] * scale;
        if (BF) { h1[e] = bf16_bits(xs); h2[e] = 0; continue; }
        const _Float16 a = (_Float16)xs;
        h1[e] = f16_bits(a);
        h2[e] = f16_bits((_Float16)(xs - (float)a));
    }
    char* base = reinterpret_cast<char*>(planes) + ((size_t)kc * NB + row) * 16 + lhi * 8;
    *reinterpret_cast<uint2*>(base) = make_uint2(h1[0] | ((unsigned)h1[1] << 16), h1[2] | ((unsigned)h1[3] << 16));
    if (!BF) *reinterpret_cast<uint2*>(base + (size_t)KC * NB * 16) = make_uint2(h2[0] | ((unsigned)h2[1] << 16), h2[2] | ((unsigned)h2[3] << 16));
}

// What every entry point's launch ends in: reserve the kernel's dynamic LDS, launch blocks of 256 threads, report under `name`.
template <typename Args>
int x3_launch(void (*kfn)(Args), unsigned grid, int lds, hipStream_t st, const Args& a, const char* name) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess)
        return vqw_set_error("%s: cannot reserve %d bytes of LDS", name, lds);
    hipLaunchKernelGGL(kfn, dim3(grid), dim3(256), lds, st, a);
    VQW_LAUNCH_CHECK(name);
    return 0;
}

}  // namespace

// vqw_f16x3_out_conv's gate-backward half (f16x3_gate_bwd.hip): picks the instantiation for a descriptor that has passed
// out_conv's checks and launches it.  Internal to the library.
__attribute__((visibility("hidden"))) int x3_gate_bwd_launch(const vqw_f16x3_out_desc& d, hipStream_t st);
