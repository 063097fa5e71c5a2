// fp16x3 engine: strided convs
#include "f16x3.h"

namespace {

#ifndef VQW_SCONV_64
#define VQW_SCONV_64 1        // strided conv: 64-row blocks for launches that would leave three quarters of the chip idle
#endif
#ifndef VQW_SCONV_192
#define VQW_SCONV_192 1       // strided conv: 192-row blocks where they fill more CUs than 256-row blocks (tools/sconv_bench.py)
#endif

// The encoder's stride-2 convs (encoder.py:17-18: conv k=5 stride 2 SAME -> relu -> BatchNorm affine) and their input
// gradients on the same main loop (LoopGeom TAB).  128-row blocks (two per CU), 256 flat (batch, time) columns per block;
// a column tile may straddle two batch rows (T = 1664 is not a multiple of 256): every lane carries its own (batch, time).
//   forward:  out[b][m][t] = bn_scale[m] * relu(sum_j sum_c W[j][c][m] x[b][c][2t + j - pad] + bias[m]) + bn_shift[m],
//             x as space-to-depth planes (split_act_kernel, s2d); relu output optionally saved for the backward pass
//   dgrad:    dx[b][m][2u + r] = sum_{j = r + pad (mod 2)} sum_o Wt[j][o][m] dy[b][o][u + (r + pad - j) / 2], both parities
//             r by the same block one after the other (their stores interleave in the same lines)
struct SconvArgs {
    vqw_f16x3_sconv_desc d;
    int NB;
    int S;           // SPLIT: K splits per tile (1: only the parities of an input gradient are spread over blocks)
};

// Split-K of a conv tile (SPLIT): the S blocks of a tile each run 1/S of the K steps and put their partial accumulators into the slab
// (in register order: 16 bytes per lane, coalesced); the block that arrives LAST at the tile's ticket counter adds the S partial tiles
// up in split order -- its own included, so the sum does not depend on who came last: results stay bitwise reproducible -- and runs
// the ordinary epilogue.  The counter is back at zero when the launch ends.  Returns false for the blocks that are done.
#ifndef VQW_SPLIT_SC1
#define VQW_SPLIT_SC1 1
#endif
#ifndef VQW_SCONV_SPLIT_MAX
#define VQW_SCONV_SPLIT_MAX 8
#endif
template <int MR>
__device__ __forceinline__ bool sconv_split_fixup(f32x16 (&acc)[MR][2], float* slab, int* counter, int S, int ksp, int tid) {
    __shared__ int s_last;
    constexpr int TILE = MR * 32 * 256;
    // The partial tiles cross XCDs (one L2 each): they are written through and read past the L2 (sc1, as agent-scope atomics are)
    // instead of fencing -- a release / acquire fence pair writes back and invalidates the whole L2 of the XCD under the other
    // blocks' main loops (measured: 12 splits of 20 K steps took longer than one block of 240).
    const __amdgpu_buffer_rsrc_t rs = vqw_make_rsrc(slab, (unsigned)((size_t)S * TILE * 4));
    constexpr int SC1 = VQW_SPLIT_SC1 ? 16 : 0;
#pragma unroll
    for (int i = 0; i < MR; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int v4 = 0; v4 < 4; ++v4) {
                const f32x4 v = f32x4{acc[i][j][v4 * 4], acc[i][j][v4 * 4 + 1], acc[i][j][v4 * 4 + 2], acc[i][j][v4 * 4 + 3]};
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rs, (ksp * TILE + ((i * 2 + j) * 4 + v4) * 1024 + tid * 4) * 4, 0, SC1);
            }
    if (VQW_SPLIT_SC1) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // every store of this wave has reached memory
    else __threadfence();
    __syncthreads();
    if (tid == 0) {
        const int old = __hip_atomic_fetch_add(counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = old == S - 1;
        if (old == S - 1) __hip_atomic_store(counter, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (!s_last) return false;
    if (!VQW_SPLIT_SC1) __threadfence();
#pragma unroll
    for (int i = 0; i < MR; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    // split order 0 .. S-1 whoever came last; the loads of the next split are in flight while one is added
    constexpr int CH = MR * 8 < 32 ? MR * 8 : 32, NH = MR * 8 / CH;      // 16-byte entries per fetch, fetches per partial tile
    f32x4 nx[CH];
    auto fetch = [&](int k, int h) {
#pragma unroll
        for (int q = 0; q < CH; ++q)
            nx[q] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, (k * TILE + (h * CH + q) * 1024 + tid * 4) * 4, 0, SC1));
    };
    fetch(0, 0);
    for (int k = 0; k < S; ++k) {
#pragma unroll
        for (int h = 0; h < NH; ++h) {
            f32x4 cur[CH];
#pragma unroll
            for (int q = 0; q < CH; ++q) cur[q] = nx[q];
            if (h + 1 < NH) fetch(k, h + 1);
            else if (k + 1 < S) fetch(k + 1, 0);
#pragma unroll
            for (int q = 0; q < CH; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int qq = h * CH + q;
                    acc[qq >> 3][(qq >> 2) & 1][(qq & 3) * 4 + e] += cur[q][e];
                }
        }
    }
    return true;
}

template <int MR, int DEPTH, bool DGRAD, bool SPLIT = false>
__global__ __launch_bounds__(256, (MR == 4 && DEPTH == 1) ? 2 : 1) void sconv_f16x3_kernel(const SconvArgs a) {
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    constexpr int HB = 32 * MR;
    const vqw_f16x3_sconv_desc& d = a.d;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l31 = lane & 31, lhi = lane >> 5;
    const int T = d.T, M = d.M;
    const int n_mt = M / HB;
    int bid = vqw_xcd_remap(blockIdx.x, gridDim.x);
    // SPLIT: block -> (K split, [parity of an input gradient,] tile), splits fastest
    int ksp = 0, par = 0, tile_id = 0;
    if constexpr (SPLIT) {
        ksp = bid % a.S; bid /= a.S;
        tile_id = bid;
        if (DGRAD) { par = bid & 1; bid >>= 1; }
    }
    const int mt = bid % n_mt, n0 = (bid / n_mt) * 256;
    const float winv = inv_scales(d.w_scale_inv, d.x_scale, d.w_scale);
    int bcol[2], tcol[2];
    bool cv[2];                      // the last column tile may reach past B * T (its operand rows read garbage or zero, nothing is stored)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = n0 + 64 * wv + 32 * j + l31;
        cv[j] = n < a.NB;
        bcol[j] = n / T;
        tcol[j] = n - bcol[j] * T;
    }
    f32x16 acc[MR][2];
    LoopGeom g;
    g.wp = d.wp; g.xp = d.xp; g.M = M; g.Cin = d.Cin; g.dilation = 1; g.NB = a.NB; g.xkc0 = 0; g.dir = 1; g.T = T;
    g.m_row0 = mt * HB; g.n0 = n0; g.t0 = 0; g.wks = d.ks;
    if constexpr (!DGRAD) {
        g.ks = d.ks; g.xKC = 2 * d.Cin / 8; g.tj0 = 0; g.tjstep = 1; g.toff = d.pad_left; g.tsgn = -1; g.ts2d = 1;
        g.sn = g.ks * (d.Cin / 16) / (SPLIT ? a.S : 1); g.sb = ksp * g.sn;
        f16x3_mainloop<false, MR, true, DEPTH>(acc, smem, g, wv, lane);
        if constexpr (SPLIT)
            if (a.S > 1 && !sconv_split_fixup<MR>(acc, d.split_slab + (size_t)tile_id * a.S * (HB * 256), d.split_counters + tile_id, a.S, ksp, tid)) return;
        const bool hb = d.bias != nullptr, hs = d.bn_scale != nullptr, sv = d.save_r != nullptr;
        const float* bp = hb ? d.bias : reinterpret_cast<const float*>(d.wp);
        const float* sp = hs ? d.bn_scale : reinterpret_cast<const float*>(d.wp);
        const float* hp = hs ? d.bn_shift : reinterpret_cast<const float*>(d.wp);
        // one 64-bit base per column, 32-bit row offsets inside (out and save_r are < 2 GiB each); the per-row constants are
        // fetched group by group (64-bit lane addresses per element and constants fetched up front spilled 570 registers)
        float* po[2];
        float* pr[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const size_t cb = (size_t)bcol[j] * M * T + tcol[j];
            po[j] = d.out + cb;
            pr[j] = sv ? d.save_r + cb : d.out + cb;
        }
        const float rlo = d.relu ? 0.0f : -INFINITY;
#pragma unroll
        for (int i = 0; i < MR; ++i)
#pragma unroll
            for (int v4 = 0; v4 < 4; ++v4) {
                const int m0 = mt * HB + 32 * i + 8 * v4 + 4 * lhi;      // first of this lane's four rows
                const f32x4 bq = hb ? *reinterpret_cast<const f32x4*>(bp + m0) : f32x4{0.f, 0.f, 0.f, 0.f};
                const f32x4 sq = hs ? *reinterpret_cast<const f32x4*>(sp + m0) : f32x4{1.f, 1.f, 1.f, 1.f};
                const f32x4 hq = hs ? *reinterpret_cast<const f32x4*>(hp + m0) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int ro = (m0 + e) * T;
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        const float y = fmaxf(acc[i][j][v4 * 4 + e] * winv + bq[e], rlo);
                        if (sv && cv[j]) pr[j][ro] = y;
                        if (cv[j]) po[j][ro] = sq[e] * y + hq[e];
                    }
                }
            }
    } else {
        g.xKC = d.Cin / 8; g.tjstep = 2; g.tsgn = 1; g.ts2d = 0;
#pragma unroll 1
        for (int r = SPLIT ? par : 0; r < (SPLIT ? par + 1 : 2); ++r) {
            g.tj0 = (r + d.pad_left) & 1; g.toff = r + d.pad_left;
            g.ks = (d.ks - g.tj0 + 1) / 2;                       // taps of this parity (>= 1 for ks >= 2)
            g.sn = g.ks * (d.Cin / 16) / (SPLIT ? a.S : 1); g.sb = ksp * g.sn;
            if (!SPLIT && r) __syncthreads();                    // the first run's last stage is still being read
            f16x3_mainloop<false, MR, true, DEPTH>(acc, smem, g, wv, lane);
            if constexpr (SPLIT)
                if (a.S > 1 && !sconv_split_fixup<MR>(acc, d.split_slab + (size_t)tile_id * a.S * (HB * 256), d.split_counters + tile_id, a.S, ksp, tid)) return;
            float* pd[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) pd[j] = d.out + (size_t)bcol[j] * M * (2 * T) + 2 * tcol[j] + r;
#pragma unroll
            for (int i = 0; i < MR; ++i)
#pragma unroll
                for (int v4 = 0; v4 < 4; ++v4) {
                    const int m0 = mt * HB + 32 * i + 8 * v4 + 4 * lhi;
#pragma unroll
                    for (int e = 0; e < 4; ++e)
#pragma unroll
                        for (int j = 0; j < 2; ++j)
                            if (cv[j]) pd[j][(m0 + e) * (2 * T)] = acc[i][j][v4 * 4 + e] * winv;
                }
        }
    }
}

}  // namespace

extern "C" {

int vqw_f16x3_strided_conv(const vqw_f16x3_sconv_desc* dp, vqw_stream_t s_) {
    hipStream_t st = (hipStream_t)s_;
    VQW_CHECK(dp, "vqw_f16x3_strided_conv: null descriptor");
    const vqw_f16x3_sconv_desc& d = *dp;
    VQW_CHECK(d.xp && d.wp && d.out, "vqw_f16x3_strided_conv: null operand");
    VQW_CHECK(d.B > 0 && d.T > 0, "vqw_f16x3_strided_conv: bad shape (B=%d T=%d)", d.B, d.T);
    VQW_CHECK(d.Cin >= 64 && d.Cin % 32 == 0 && d.M > 0 && d.M % 128 == 0, "vqw_f16x3_strided_conv: Cin %% 32, M %% 128 (Cin=%d M=%d)", d.Cin, d.M);
    VQW_CHECK(d.ks >= 2 && d.ks <= 8 && d.pad_left >= 0 && d.pad_left < d.ks, "vqw_f16x3_strided_conv: 2..8 taps, 0 <= pad_left < ks (ks=%d pad_left=%d)", d.ks, d.pad_left);
    VQW_CHECK(!d.bn_scale || d.bn_shift, "vqw_f16x3_strided_conv: bn_scale needs bn_shift");
    VQW_CHECK(d.w_scale_inv > 0.0f, "vqw_f16x3_strided_conv: w_scale_inv must be positive");
    const size_t xbytes = (size_t)2 * (d.dgrad ? 1 : 2) * (d.Cin / 8) * d.B * d.T * 16, obytes = (size_t)d.B * d.M * d.T * (d.dgrad ? 2 : 1) * 4;
    VQW_CHECK(xbytes < ((size_t)1 << 31) && obytes < ((size_t)1 << 31) && (size_t)2 * d.ks * (d.Cin / 8) * d.M * 16 < ((size_t)1 << 31),
              "vqw_f16x3_strided_conv: operands exceed 2 GiB");
    SconvArgs a;
    a.d = d;
    a.NB = d.B * d.T;
    // block shape (d.shape forces one).  Measured on the benchmark's layers (tools/sconv_bench.py, us, shapes 1 / 2 / 3 / 4):
    //   forward  T=1664: 299 / 290 / 228 / 196   T=832: 154 / 129 / 196 / 155   T=416: 150 / 125 / 196 / 152
    //   dgrad    T=1664: 314 / 311 / 303 / 236   T=832: 198 / 142 / 275 / 184   T=416: 196 / 134 / 273 / 182
    // -> 256-row blocks for a launch that fills more than half of the chip with them, otherwise the deep 128-row shape
    const int cus = vqw_device_cus(), nt = (a.NB + 255) / 256;      // (a partial last column tile is masked in the epilogue)
    int shape = d.shape;
    if (shape == 0) shape = (d.M % 256 == 0 && (d.M / 256) * nt * 2 > cus) ? 3 : 2;
    // 192-row blocks where they fill more CUs than 256-row blocks without a second round (768 rows x 52 column tiles: 208 blocks
    // instead of 156 on 256 CUs)
    if (d.shape == 0 && shape == 3 && d.M % 192 == 0 && (d.M / 192) * nt <= cus && VQW_SCONV_192) shape = 4;
    // 64-row blocks for the shortest layers (encoder layers 4 and 5: 42 / 24 blocks of 128 rows on 256 CUs): twice the blocks at half
    // the MFMAs per step -- 105 against 125 us per launch, tools/sconv_bench.py (a step then costs ~880 cycles for 384 of MFMA: the
    // issue pattern has 12 MFMA shadows for ~20 memory instructions; four stages of requests in flight measured no better, 108 us)
    if (d.shape == 0 && shape == 2 && (d.M / 128) * nt * 4 <= cus && VQW_SCONV_64) shape = 5;
    VQW_CHECK(shape >= 1 && shape <= 5 && (shape != 3 || d.M % 256 == 0) && (shape != 4 || d.M % 192 == 0) && (shape != 5 || d.M % 64 == 0),
              "vqw_f16x3_strided_conv: shape is 0 (auto), 1, 2, 3 (256-row blocks: M %% 256 == 0), 4 (192-row blocks: M %% 192 == 0) or 5 (64-row blocks)");
    typedef void (*kfn_t)(SconvArgs);
    // Split-K (scratch given): a launch of few 128-row tiles cuts each tile's K steps over S blocks -- as many as fill the chip once, the
    // steps of every parity in even parts of at least 8 steps, at most 8 partial tiles per fix-up (256-row tiles measured slower at every
    // split count, tools/sconv_bench.py, and their fix-up does not fit the register file).
    if (d.split_slab && d.ksplit != 1 && (d.shape == 0 || d.shape == 2)) {
        VQW_CHECK(d.split_counters, "vqw_f16x3_strided_conv: split_slab needs split_counters");
        const int spt = d.Cin / 16, par = d.dgrad ? 2 : 1;
        const int st0 = d.dgrad ? ((d.ks - (d.pad_left & 1) + 1) / 2) * spt : d.ks * spt;          // K steps of parity 0 / the forward conv
        const int st1 = d.dgrad ? ((d.ks - ((1 + d.pad_left) & 1) + 1) / 2) * spt : st0;
        auto fits = [&](int S) { return S >= 1 && st0 % (2 * S) == 0 && st1 % (2 * S) == 0 && st0 / S >= 8 && st1 / S >= 8; };
        const int tiles = (d.M / 128) * nt * par;
        int S = d.ksplit;
        if (S == 0) {
            // one round of blocks; tools/sconv_bench.py (us per launch, 24 tiles: S = 2 / 4 / 8 / 10 / 12 -> 82 / 54 / 47.5 / 49 / 65): a K step
            // costs ~0.55 us, a partial tile in the fix-up ~2.5 us.  Where even two blocks per tile do not fit in one round but the unsplit
            // launch would leave two thirds of the chip idle (the input gradient of layer 3: 78 blocks of 120 steps), up to two rounds
            // (130 -> 90 us with three splits).
            for (int c = 2; c <= VQW_SCONV_SPLIT_MAX; ++c) if (fits(c) && tiles * c <= cus) S = c;
            if (S == 0 && (tiles / par) * 3 <= cus)
                for (int c = 2; c <= VQW_SCONV_SPLIT_MAX; ++c) if (fits(c) && tiles * c <= 2 * cus) S = c;
        }
        if (S > 1) {
            VQW_CHECK(fits(S), "vqw_f16x3_strided_conv: the K steps (%d / %d) do not divide into %d even parts of >= 8", st0, st1, S);
            VQW_CHECK(tiles <= d.split_counters_n && (int64_t)tiles * S * 128 * 256 <= d.split_slab_floats,
                      "vqw_f16x3_strided_conv: split scratch too small (%d tiles x %d splits)", tiles, S);
            a.S = S;
            const kfn_t kfn = d.dgrad ? sconv_f16x3_kernel<4, 2, true, true> : sconv_f16x3_kernel<4, 2, false, true>;
            return x3_launch(kfn, tiles * S, 4 * (4 * 2 + 16) * 1024, st, a, "vqw_f16x3_strided_conv");
        }
    }
    a.S = 1;
    // shape 1..5 -> kernel (forward, input gradient), rows of a block / 32, LDS stages (DEPTH + 2)
    const struct { kfn_t kfn[2]; int mr, nstage; } shapes[5] = {
        {{sconv_f16x3_kernel<4, 1, false>, sconv_f16x3_kernel<4, 1, true>}, 4, 3},
        {{sconv_f16x3_kernel<4, 2, false>, sconv_f16x3_kernel<4, 2, true>}, 4, 4},
        {{sconv_f16x3_kernel<8, 2, false>, sconv_f16x3_kernel<8, 2, true>}, 8, 4},
        {{sconv_f16x3_kernel<6, 2, false>, sconv_f16x3_kernel<6, 2, true>}, 6, 4},
        {{sconv_f16x3_kernel<2, 2, false>, sconv_f16x3_kernel<2, 2, true>}, 2, 4}};
    const auto& sh = shapes[shape - 1];
    return x3_launch(sh.kfn[d.dgrad ? 1 : 0], (d.M / (32 * sh.mr)) * nt, sh.nstage * (sh.mr * 2 + 16) * 1024, st, a, "vqw_f16x3_strided_conv");
}

}  // extern "C"
