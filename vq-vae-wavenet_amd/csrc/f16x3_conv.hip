// fp16x3 engine: forward convs
#include "f16x3.h"

namespace {

struct GateArgs {
    vqw_f16x3_gate_desc d;
    int NB;        // B * T rows of the activation planes
    int ratio;     // T / cond_T
};

template <bool BF, int MR>
__global__ __launch_bounds__(256, MR == 8 ? 1 : 2) void gate_f16x3_kernel(const GateArgs a) {
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    const vqw_f16x3_gate_desc& d = a.d;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l31 = lane & 31, lhi = lane >> 5;
    const int R = d.R, T = d.T;
    constexpr int HB = 32 * MR, HH = HB / 2;                 // block rows: HH filter channels, then the HH matching gate channels
    const int n_mt = R / HH;
    const int bid = vqw_xcd_remap(blockIdx.x, gridDim.x);
    const int mt = bid % n_mt, n0 = (bid / n_mt) * 256;     // 256 | T: a block never straddles two batch rows
    const int b = n0 / T, t0 = n0 - b * T;
    f32x16 acc[MR][2];
    {
        LoopGeom g;
        g.wp = d.wp; g.xp = d.xp; g.M = 2 * R; g.Cin = R; g.ks = d.ks; g.dilation = d.dilation; g.NB = a.NB;
        g.xKC = R / 8; g.xkc0 = 0; g.dir = 1; g.T = T;
        g.m_row0 = mt * HB; g.n0 = n0; g.t0 = t0;
        f16x3_mainloop<BF, MR>(acc, smem, g, wv, lane);
    }

    // ---- epilogue: + bias + upsampled condition (add_condition, wavenet_ops.py:93-101), tanh(filter) * sigmoid(gate).
    // With one block per CU nothing overlaps it, so it is kept lean: one 64-bit row offset per four channels, 32-bit
    // offsets inside, v_rcp_f32 instead of IEEE divisions (1 ulp; the quotients feed tanh/sigmoid values in [-1, 1]).
    // The per-row constants, bias[c] + cond[b][c][frame], depend on neither the lane's column nor the group: requested group by
    // group (24 loads of L2 hits, every lane of a half-wave the same word, and a wait before anything is computed) they cost
    // 2 MR exposed round trips per block and 24 registers.  LDSC, the 128-row blocks: the block's four waves fetch them ONCE
    // instead, into the ring the main loop has left: HB channels x the frames its 256 columns touch -- at most 8 (32 | ratio), all
    // 8 slots are filled, the frames past the block's last one with that one's values -- as table[frame - first frame][block row],
    // the sums formed as the groups form them (bias + cond, an absent operand masked to +0: x3_masked), so that a group reads four
    // rows of one frame with one 16-byte LDS read that every lane of a half-wave shares.  The 256-row blocks keep the requests:
    // with every register taken they need 20-50 bytes more scratch per lane for the table's reads than for the loads.
    constexpr bool LDSC = MR == 4;
    const bool hb = d.bias != nullptr, hc = d.cond != nullptr;
    const float* bp = hb ? d.bias : reinterpret_cast<const float*>(d.wp);      // absent operands read a valid dummy address
    const float* cb = hc ? d.cond + (size_t)b * d.cond_bstride : reinterpret_cast<const float*>(d.wp);
    const int tcol = t0 + 64 * wv + l31;
    const unsigned mb = x3_present(hb), mc = x3_present(hc);
    const int tzb = t0 / a.ratio, tzl = (t0 + 255) / a.ratio;      // the block's first and last frame
    // (32 | ratio: one frame per tile row; without a condition ratio is 1 and every frame index is masked to 0)
    const int tz0 = (t0 + 64 * wv) / a.ratio, tz1 = (t0 + 64 * wv + 32) / a.ratio;
    const int fz0 = x3_masked(tz0 - tzb, mc), fz1 = x3_masked(tz1 - tzb, mc);
    const float* table = reinterpret_cast<const float*>(smem);
    if constexpr (LDSC) {
        __syncthreads();      // every wave has drained its own requests (f16x3_mainloop) and read its last fragments: the ring is dead
        constexpr int NV = HB * 8 / 256;
        float tb[NV], tc[NV];
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const int idx = tid + 256 * v, row = idx >> 3, f = idx & 7;      // (frames innermost: a channel's frames are one 32-byte read)
            const int c = (row < HH ? 0 : R - HH) + HH * mt + row;
            const int tz = tzb + f < tzl ? tzb + f : tzl;
            tb[v] = bp[x3_masked(c, mb)];
            tc[v] = cb[x3_masked(c * d.cond_T + tz, mc)];
        }
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const int idx = tid + 256 * v, row = idx >> 3, f = idx & 7;
            reinterpret_cast<float*>(smem)[f * HB + row] = x3_masked(tb[v], mb) + x3_masked(tc[v], mc);
        }
        __syncthreads();
    }
    const float winv = inv_scales(d.w_scale_inv, d.x_scale, d.w_scale);
    // STEP: the outputs the training step asks for (sigmoid + gated planes) are known at compile time -- no branch around any
    // store; every other combination takes the same body with its block-uniform conditions tested at run time
    auto epilogue = [&](auto step_c) {
        constexpr bool STEP = decltype(step_c)::value;
        const bool s0 = STEP ? false : d.save0 != nullptr, s1 = STEP ? true : d.save1 != nullptr;
        const bool w0 = STEP ? false : d.out0 != nullptr, wp_ = STEP ? true : d.out_planes != nullptr;
        struct OpsMem { float bf[4], bg[4], f0[4], f1[4], g0[4], g1[4]; };
        struct OpsLds { float4 f0, f1, g0, g1; };
        typedef std::conditional_t<LDSC, OpsLds, OpsMem> Ops;
        auto request = [&](int g, Ops& o) {
            const int i = g >> 2, v4 = g & 3;
            const int r0 = 32 * i + 8 * v4 + 4 * lhi;          // first of this lane's four filter rows of the block; gate rows: + HH
            if constexpr (LDSC) {
                o.f0 = *reinterpret_cast<const float4*>(table + fz0 * HB + r0); o.f1 = *reinterpret_cast<const float4*>(table + fz1 * HB + r0);
                o.g0 = *reinterpret_cast<const float4*>(table + fz0 * HB + HH + r0); o.g1 = *reinterpret_cast<const float4*>(table + fz1 * HB + HH + r0);
            } else {
                const int c0 = HH * mt + r0;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    o.bf[e] = bp[x3_masked(c0 + e, mb)]; o.bg[e] = bp[x3_masked(R + c0 + e, mb)];
                    const int cf = (c0 + e) * d.cond_T, cg = (R + c0 + e) * d.cond_T;
                    o.f0[e] = cb[x3_masked(cf + tz0, mc)]; o.f1[e] = cb[x3_masked(cf + tz1, mc)];
                    o.g0[e] = cb[x3_masked(cg + tz0, mc)]; o.g1[e] = cb[x3_masked(cg + tz1, mc)];
                }
            }
        };
        auto finish = [&](int g, const Ops& o) {
            const int i = g >> 2, v4 = g & 3;
            const int c0 = HH * mt + 32 * i + 8 * v4 + 4 * lhi;          // first of this lane's four channels
            float addf[4][2], addg[4][2];
            if constexpr (LDSC) {
                const float tf[2][4] = {{o.f0.x, o.f0.y, o.f0.z, o.f0.w}, {o.f1.x, o.f1.y, o.f1.z, o.f1.w}};
                const float tg[2][4] = {{o.g0.x, o.g0.y, o.g0.z, o.g0.w}, {o.g1.x, o.g1.y, o.g1.z, o.g1.w}};
#pragma unroll
                for (int e = 0; e < 4; ++e) { addf[e][0] = tf[0][e]; addf[e][1] = tf[1][e]; addg[e][0] = tg[0][e]; addg[e][1] = tg[1][e]; }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float bfv = o.bf[e], bgv = o.bg[e], f0 = o.f0[e], f1 = o.f1[e], g0 = o.g0[e], g1 = o.g1[e];
                    addf[e][0] = x3_masked(bfv, mb) + x3_masked(f0, mc); addf[e][1] = x3_masked(bfv, mb) + x3_masked(f1, mc);
                    addg[e][0] = x3_masked(bgv, mb) + x3_masked(g0, mc); addg[e][1] = x3_masked(bgv, mb) + x3_masked(g1, mc);
                }
            }
            const size_t off = ((size_t)b * R + c0) * T + tcol;
            float* po = (w0 ? d.out0 : d.save1) + off;
            float* p0 = s0 ? d.save0 + off : po;
            float* p1 = s1 ? d.save1 + off : po;
            float gq[2][4];
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const float xf = acc[i][j][v4 * 4 + e] * winv + addf[e][j];
                    const float xg = acc[i + MR / 2][j][v4 * 4 + e] * winv + addg[e][j];
                    const float th = 1.0f - 2.0f * __builtin_amdgcn_rcpf(__expf(2.0f * xf) + 1.0f);
                    const float sg = __builtin_amdgcn_rcpf(1.0f + __expf(-xg));
                    const int o_ = e * T + 32 * j;
                    gq[j][e] = th * sg;
                    // (the fp32 product itself goes into the planes, also where no fp32 copy of it is stored: unpinned, a body that
                    // only writes planes rounds th * sg to fp16 in one step -- v_fma_mixlo_f16 -- and the plane bits change)
                    if constexpr (STEP) asm volatile("" : "+v"(gq[j][e]));
                    if (s0) p0[o_] = th;
                    if (s1) p1[o_] = sg;
                    if (w0) po[o_] = gq[j][e];        // (optional where every reader takes the planes: 54 MB less per layer)
                }
            if (wp_) {
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    store_plane_quad<BF>(d.out_planes, d.out_planes_KC > 0 ? d.out_planes_KC : R / 8, a.NB, d.out_planes_kc0 + (HH / 8) * mt + 4 * i + v4,
                                     n0 + 64 * wv + 32 * j + l31, lhi, gq[j]);
            }
        };
        // (a group is requested, computed and stored before the next one: the 256-row blocks have no registers for a second
        // group of 24 loads -- 40-240 bytes of scratch per lane at depth 1 and 2 --, and the table's reads are LDS reads)
        x3_epilogue_pipeline<MR * 2, 0, Ops>(request, finish);
    };
    if (!d.out0 && !d.save0 && d.save1 && d.out_planes) epilogue(std::true_type{});
    else epilogue(std::false_type{});
}

// The layer's 1x1 skip + residual conv (wavenet_ops.py:132-136, wavenet.py:72-73) on the gated planes:
// rows 0..S-1: skip += W_s g + b_s; rows S..S+R-1: net' = net + W_r g + b_r (and net' as planes for the next gate conv).
template <bool BF, int MR>
__global__ __launch_bounds__(256, MR == 8 ? 1 : 2) void out_f16x3_kernel(const OutArgs a) {
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    const vqw_f16x3_out_desc& d = a.d;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l31 = lane & 31, lhi = lane >> 5;
    const int R = d.R, S = d.S, T = d.T, M = S + R;      // S skip rows, then R residual rows (either may be 0)
    const int Cin = d.Cin > 0 ? d.Cin : R;
    constexpr int HB = 32 * MR;
    const int n_mt = M / HB;
    const int bid = vqw_xcd_remap(blockIdx.x, gridDim.x);
    const int mt = bid % n_mt, n0 = (bid / n_mt) * 256;
    const int b = n0 / T, t0 = n0 - b * T;
    f32x16 acc[MR][2];
    {
        LoopGeom g;
        g.wp = d.wp; g.xp = d.xp; g.M = M; g.Cin = Cin; g.ks = d.ks > 0 ? d.ks : 1; g.dilation = d.dilation > 0 ? d.dilation : 1; g.NB = a.NB;
        g.xKC = d.xp_KC > 0 ? d.xp_KC : Cin / 8; g.xkc0 = d.xp_kc0; g.dir = d.dir < 0 ? -1 : 1; g.T = T;
        g.m_row0 = mt * HB; g.n0 = n0; g.t0 = t0;
        f16x3_mainloop<BF, MR>(acc, smem, g, wv, lane);
    }
    const bool is_skip = mt * HB < S;     // 256 | S: a block is all skip rows or all residual rows
    const bool hb = d.bias != nullptr;
    const float* bp = hb ? d.bias : reinterpret_cast<const float*>(d.wp);
    const int tcol = t0 + 64 * wv + l31;
    const float winv = inv_scales(d.w_scale_inv, d.x_scale, d.w_scale);
    const float ps = (d.plane_scale > 0.0f ? d.plane_scale : 1.0f) * dev_scale(d.out_scale);
    const bool hin = is_skip || d.net_in != nullptr;
    const unsigned mb = x3_present(hb), min_ = x3_present(hin);
    // (chosen once, not per group: a block reads and writes either skip rows or residual rows)
    const float* in_base = is_skip ? d.skip : (d.net_in ? d.net_in : d.net_out);
    float* out_base = is_skip ? d.skip : d.net_out;
    const int nrows = is_skip ? S : R, mrow0 = is_skip ? 0 : S;
    // net_out may be net_in (and skip is updated in place): the old values of group g + 2 are requested before group g is stored,
    // which is legal because a lane reads and writes the same elements within one group and groups are disjoint (x3_epilogue_pipeline)
    struct Ops { float bq[4], old[2][4]; };
    // PL: this block writes planes (and reports to the range guard) -- block-uniform, decided once in front of the epilogue
    auto epilogue = [&](auto pl_c) {
        constexpr bool PL = decltype(pl_c)::value;
        float gmax = 0.0f;
        bool gbad = false;
        auto offset = [&](int g, int& m0) {
            const int i = g >> 2, v4 = g & 3;
            m0 = mt * HB + 32 * i + 8 * v4 + 4 * lhi;      // first of this lane's four rows
            return ((size_t)b * nrows + (m0 - mrow0)) * T + tcol;
        };
        auto request = [&](int g, Ops& o) {
            int m0;
            const size_t off = offset(g, m0);
            const float* pin = in_base + off;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                o.bq[e] = bp[x3_masked(m0 + e, mb)];
#pragma unroll
                for (int j = 0; j < 2; ++j) o.old[j][e] = pin[e * T + 32 * j];
            }
        };
        auto finish = [&](int g, const Ops& o) {
            const int i = g >> 2, v4 = g & 3;
            int m0;
            const size_t off = offset(g, m0);
            float* pout = out_base + off;
            float bq[4], old[2][4], nq[2][4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float bv = o.bq[e];
                bq[e] = x3_masked(bv, mb);
#pragma unroll
                for (int j = 0; j < 2; ++j) { const float ov = o.old[j][e]; old[j][e] = x3_masked(ov, min_); }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    nq[j][e] = old[j][e] + (acc[i][j][v4 * 4 + e] * winv + bq[e]);
                    pout[e * T + 32 * j] = nq[j][e];
                }
            if constexpr (PL) {
#pragma unroll
                for (int j = 0; j < 2; ++j) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) { gmax = fmaxf(gmax, fabsf(nq[j][e])); gbad |= !(fabsf(nq[j][e]) <= 3.0e38f); }
                    store_plane_quad<BF>(d.net_out_planes, d.planes_KC > 0 ? d.planes_KC : R / 8, a.NB, d.planes_kc0 + (m0 - S) / 8,
                                     n0 + 64 * wv + 32 * j + l31, lhi, nq[j], ps);
                }
                x3_pin_guard(gmax, gbad);
            }
        };
        x3_epilogue_pipeline<MR * 4, EPI_DEPTH, Ops>(request, finish);
        if constexpr (PL) guard_report(gmax, gbad, ps, d.out_amax, d.flag);
    };
    if (!is_skip && d.net_out_planes) epilogue(std::true_type{});
    else epilogue(std::false_type{});
}

// The 1x1 convs around the residual stack (wavenet.py:53-54, 72, 80-96) and their input gradients, epi = 2:
//   out[b][m][t] = mask * (net_in[b][m][t] + (W x)[m] + bias[m] + cond[b][m][t / ratio]),   mask = (aux0[b][m][t] > 0) or 1
// (net_in, bias, cond, aux0 optional; out may be net_in and / or aux0: every element is read and written by one lane), and
// out -- or relu(out), flags bit 0 -- once more as planes for the next contraction, range-checked like the others.
template <int MR, bool BF = false>
__global__ __launch_bounds__(256, MR == 8 ? 1 : 2) void head_f16x3_kernel(const OutArgs a) {
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    const vqw_f16x3_out_desc& d = a.d;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l31 = lane & 31, lhi = lane >> 5;
    const int M = d.R, T = d.T;
    constexpr int HB = 32 * MR;
    const int n_mt = M / HB;
    const int bid = vqw_xcd_remap(blockIdx.x, gridDim.x);
    const int mt = bid % n_mt, n0 = (bid / n_mt) * 256;
    const int b = n0 / T, t0 = n0 - b * T;
    f32x16 acc[MR][2];
    {
        LoopGeom g;
        g.wp = d.wp; g.xp = d.xp; g.M = M; g.Cin = d.Cin; g.ks = 1; g.dilation = 1; g.NB = a.NB;
        g.xKC = d.xp_KC > 0 ? d.xp_KC : d.Cin / 8; g.xkc0 = d.xp_kc0; g.dir = 1; g.T = T;
        g.m_row0 = mt * HB; g.n0 = n0; g.t0 = t0;
        f16x3_mainloop<BF, MR>(acc, smem, g, wv, lane);
    }
    const bool hb = d.bias != nullptr, hc = d.cond != nullptr, hin = d.net_in != nullptr, hm = d.aux0 != nullptr;
    const bool relu_planes = (d.flags & 1) != 0;
    const float* bp = hb ? d.bias : reinterpret_cast<const float*>(d.wp);      // absent operands read a valid dummy address
    const float* cb = hc ? d.cond + (size_t)b * d.cond_bstride : reinterpret_cast<const float*>(d.wp);
    const int ratio = hc ? T / d.cond_T : 1;
    const int tz[2] = {(t0 + 64 * wv) / ratio, (t0 + 64 * wv + 32) / ratio};   // 32 | ratio: one frame per tile row
    const int tcol = t0 + 64 * wv + l31;
    const float winv = inv_scales(d.w_scale_inv, d.x_scale, d.w_scale);
    const float ps = (d.plane_scale > 0.0f ? d.plane_scale : 1.0f) * dev_scale(d.out_scale);
    const int PKC = d.planes_KC > 0 ? d.planes_KC : M / 8;
    const unsigned mb = x3_present(hb), mc = x3_present(hc), min_ = x3_present(hin), mnm = x3_present(!hm);
    const float* in_base = hin ? d.net_in : d.net_out;        // absent operands read net_out's own (valid) addresses
    const float* mask_base = hm ? d.aux0 : d.net_out;
    // net_out may be net_in and / or aux0: a lane reads its elements of group g + 2 before group g is stored, and groups are
    // disjoint (x3_epilogue_pipeline)
    struct Ops { float bv[4], c0[4], c1[4], old[2][4], mv[2][4]; };
    auto epilogue = [&](auto pl_c) {      // PL: planes (and the range guard) are written
        constexpr bool PL = decltype(pl_c)::value;
        float gmax = 0.0f;
        bool gbad = false;
        auto request = [&](int g, Ops& o) {
            const int i = g >> 2, v4 = g & 3;
            const int m0 = mt * HB + 32 * i + 8 * v4 + 4 * lhi;      // first of this lane's four rows
            const size_t off = ((size_t)b * M + m0) * T + tcol;
            const float* pin = in_base + off;
            const float* pm = mask_base + off;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                o.bv[e] = bp[x3_masked(m0 + e, mb)];
                const int cr = (m0 + e) * d.cond_T;
                o.c0[e] = cb[x3_masked(cr + tz[0], mc)]; o.c1[e] = cb[x3_masked(cr + tz[1], mc)];
#pragma unroll
                for (int j = 0; j < 2; ++j) { o.old[j][e] = pin[e * T + 32 * j]; o.mv[j][e] = pm[e * T + 32 * j]; }
            }
        };
        auto finish = [&](int g, const Ops& o) {
            const int i = g >> 2, v4 = g & 3;
            const int m0 = mt * HB + 32 * i + 8 * v4 + 4 * lhi;
            const size_t off = ((size_t)b * M + m0) * T + tcol;
            float* pout = d.net_out + off;
            float add[4][2], old[2][4], mk[2][4], nq[2][4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float bv = o.bv[e], c0 = o.c0[e], c1 = o.c1[e];
                add[e][0] = x3_masked(bv, mb) + x3_masked(c0, mc);
                add[e][1] = x3_masked(bv, mb) + x3_masked(c1, mc);
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const float ov = o.old[j][e], mv = o.mv[j][e];
                    old[j][e] = x3_masked(ov, min_);
                    mk[j][e] = x3_masked(1.0f, (mv > 0.0f ? 0xffffffffu : 0u) | mnm);
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    nq[j][e] = mk[j][e] * (old[j][e] + (acc[i][j][v4 * 4 + e] * winv + add[e][j]));
                    pout[e * T + 32 * j] = nq[j][e];
                }
            if constexpr (PL) {
#pragma unroll
                for (int j = 0; j < 2; ++j) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        // (the stored fp32 value itself goes into the planes: unpinned, the body without relu contracts the product
                        // above into the fp16 conversions and the plane bits change)
                        asm volatile("" : "+v"(nq[j][e]));
                        gbad |= !(fabsf(nq[j][e]) <= 3.0e38f);
                        if (relu_planes) nq[j][e] = fmaxf(nq[j][e], 0.0f);
                        gmax = fmaxf(gmax, fabsf(nq[j][e]));
                    }
                    store_plane_quad<BF>(d.net_out_planes, PKC, a.NB, d.planes_kc0 + m0 / 8, n0 + 64 * wv + 32 * j + l31, lhi, nq[j], ps);
                }
                x3_pin_guard(gmax, gbad);
            }
        };
        // depth 1: a group has 28 operand registers (the 128-row bf16 instantiation has none to spare: it keeps the plain order)
        x3_epilogue_pipeline<MR * 4, (MR == 4 && BF) ? 0 : 1, Ops>(request, finish);
        if constexpr (PL) guard_report(gmax, gbad, ps, d.out_amax, d.flag);
    };
    if (d.net_out_planes) epilogue(std::true_type{});
    else epilogue(std::false_type{});
}

}  // namespace

extern "C" {

int vqw_f16x3_out_conv(const vqw_f16x3_out_desc* dp, vqw_stream_t s_) {
    hipStream_t st = (hipStream_t)s_;
    VQW_CHECK(dp, "vqw_f16x3_out_conv: null descriptor");
    const vqw_f16x3_out_desc& d = *dp;
    VQW_CHECK(d.xp && d.wp, "vqw_f16x3_out_conv: null operand");
    VQW_CHECK((d.S == 0 || d.skip) && (d.R == 0 || d.net_out || (d.epi == 1 && d.net_out_planes)), "vqw_f16x3_out_conv: null output");
    VQW_CHECK(d.ks >= 0 && d.ks <= 8 && d.dilation >= 0, "vqw_f16x3_out_conv: bad kernel size %d / dilation %d", d.ks, d.dilation);
    VQW_CHECK(d.B > 0 && d.T > 0 && d.T % 256 == 0, "vqw_f16x3_out_conv: T must be a positive multiple of 256 (got %d)", d.T);
    VQW_CHECK(d.R >= 0 && d.R % 256 == 0 && d.S >= 0 && d.S % 256 == 0 && d.S + d.R > 0, "vqw_f16x3_out_conv: R and S must be multiples of 256 (R=%d S=%d)", d.R, d.S);
    const int cin = d.Cin > 0 ? d.Cin : d.R, xkc = d.xp_KC > 0 ? d.xp_KC : cin / 8;
    VQW_CHECK(cin >= 64 && cin % 32 == 0 && d.xp_kc0 >= 0 && d.xp_kc0 + cin / 8 <= xkc && (d.ks <= 1 || d.xp_kc0 == 0), "vqw_f16x3_out_conv: bad contraction range (Cin=%d kc0=%d KC=%d)", cin, d.xp_kc0, xkc);
    VQW_CHECK((size_t)(cin / 8) * d.B * d.T * 16 < (size_t)1 << 31, "vqw_f16x3_out_conv: the chunks of one contraction (Cin = %d) exceed 2 GiB per plane: cut it into channel groups", cin);
    VQW_CHECK(d.w_scale_inv > 0.0f, "vqw_f16x3_out_conv: w_scale_inv must be positive");
    OutArgs a;
    a.d = d;
    a.NB = d.B * d.T;
    VQW_CHECK(d.mode >= 0 && d.mode <= 3, "vqw_f16x3_out_conv: mode is a bit set of VQW_X3_BF16 | VQW_X3_HALF_BLOCKS");
    const bool bf = (d.mode & 1) != 0, half = (d.mode & VQW_X3_HALF_BLOCKS) != 0;
    typedef void (*kfn_t)(OutArgs);
    const kfn_t kouts[4] = {out_f16x3_kernel<false, 8>, out_f16x3_kernel<true, 8>, out_f16x3_kernel<false, 4>, out_f16x3_kernel<true, 4>};
    const int lds = half ? X3Shape<4>::LDS_BYTES : X3Shape<8>::LDS_BYTES, hb = half ? 128 : 256;
    if (d.epi == 2) {
        VQW_CHECK(d.S == 0 && d.R > 0 && d.net_out && d.Cin > 0 && d.ks <= 1, "vqw_f16x3_out_conv: epi 2 needs S = 0, net_out, Cin and a 1x1 kernel");
        VQW_CHECK(!d.cond || (d.cond_T > 0 && d.T % d.cond_T == 0 && (d.T / d.cond_T) % 32 == 0 && d.cond_bstride >= (int64_t)d.R * d.cond_T),
                  "vqw_f16x3_out_conv: T / cond_T must be a multiple of 32 (T=%d cond_T=%d)", d.T, d.cond_T);
        const kfn_t kfn = bf ? (half ? head_f16x3_kernel<4, true> : head_f16x3_kernel<8, true>) : (half ? head_f16x3_kernel<4> : head_f16x3_kernel<8>);
        return x3_launch(kfn, (d.R / hb) * (a.NB / 256), lds, st, a, "vqw_f16x3_out_conv");
    }
    if (d.epi == 1) {
        VQW_CHECK(d.S == 0 && d.R > 0 && d.aux0 && d.aux1 && d.Cin > 0, "vqw_f16x3_out_conv: gate backward needs S = 0, saved tanh (aux0) and sigmoid (aux1), Cin");
        // flags bit 2: aux0 = the gated planes [planes][aux0_KC][B*T][8] from chunk aux0_kc0
        VQW_CHECK(!(d.flags & 4) || (d.aux0_kc0 >= 0 && d.aux0_kc0 + d.R / 8 <= (d.aux0_KC > 0 ? d.aux0_KC : d.R / 8)), "vqw_f16x3_out_conv: bad chunk range of the gated planes");
        return x3_gate_bwd_launch(d, st);
    }
    return x3_launch(kouts[(bf ? 1 : 0) + (half ? 2 : 0)], ((d.S + d.R) / hb) * (a.NB / 256), lds, st, a, "vqw_f16x3_out_conv");
}

int vqw_f16x3_gate_conv(const vqw_f16x3_gate_desc* dp, vqw_stream_t s_) {
    hipStream_t st = (hipStream_t)s_;
    VQW_CHECK(dp, "vqw_f16x3_gate_conv: null descriptor");
    const vqw_f16x3_gate_desc& d = *dp;
    VQW_CHECK(d.xp && d.wp && (d.out0 || (d.out_planes && d.save1)), "vqw_f16x3_gate_conv: null operand (out0 may be NULL only with out_planes and save1)");
    VQW_CHECK(d.B > 0 && d.T > 0 && d.T % 256 == 0, "vqw_f16x3_gate_conv: T must be a positive multiple of 256 (got %d)", d.T);
    VQW_CHECK(d.R > 0 && d.R % 128 == 0, "vqw_f16x3_gate_conv: R must be a multiple of 128 (got %d)", d.R);
    VQW_CHECK(d.ks >= 1 && d.ks <= 8 && d.dilation >= 1, "vqw_f16x3_gate_conv: bad kernel size %d / dilation %d", d.ks, d.dilation);
    VQW_CHECK((size_t)(d.R / 8) * d.B * d.T * 16 < (size_t)1 << 31, "vqw_f16x3_gate_conv: one activation plane exceeds 2 GiB");
    VQW_CHECK(d.out_planes_KC == 0 || (d.out_planes_kc0 >= 0 && d.out_planes_kc0 + d.R / 8 <= d.out_planes_KC),
              "vqw_f16x3_gate_conv: bad output plane range (kc0=%d KC=%d)", d.out_planes_kc0, d.out_planes_KC);
    VQW_CHECK(d.w_scale_inv > 0.0f, "vqw_f16x3_gate_conv: w_scale_inv must be positive");
    GateArgs a;
    a.d = d;
    a.NB = d.B * d.T;
    a.ratio = 1;
    if (d.cond) {
        VQW_CHECK(d.cond_T > 0 && d.T % d.cond_T == 0 && (d.T / d.cond_T) % 32 == 0,
                  "vqw_f16x3_gate_conv: T / cond_T must be a multiple of 32 (T=%d cond_T=%d)", d.T, d.cond_T);
        a.ratio = d.T / d.cond_T;
    }
    VQW_CHECK(d.mode >= 0 && d.mode <= 3, "vqw_f16x3_gate_conv: mode is a bit set of VQW_X3_BF16 | VQW_X3_HALF_BLOCKS");
    const bool bf = (d.mode & 1) != 0, half = (d.mode & VQW_X3_HALF_BLOCKS) != 0;
    typedef void (*kfn_t)(GateArgs);
    const kfn_t ks4[4] = {gate_f16x3_kernel<false, 8>, gate_f16x3_kernel<true, 8>, gate_f16x3_kernel<false, 4>, gate_f16x3_kernel<true, 4>};
    const kfn_t kfn = ks4[(bf ? 1 : 0) + (half ? 2 : 0)];
    const int lds = half ? X3Shape<4>::LDS_BYTES : X3Shape<8>::LDS_BYTES;
    return x3_launch(kfn, (d.R / (half ? 64 : 128)) * (a.NB / 256), lds, st, a, "vqw_f16x3_gate_conv");
}

}  // extern "C"
