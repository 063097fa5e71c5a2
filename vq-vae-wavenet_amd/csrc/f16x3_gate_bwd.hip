// fp16x3 engine: gate backward
#include "f16x3.h"

namespace {

// Gate backward (the transpose of gated_cnn's tanh * sigmoid, wavenet_ops.py:112-113, behind the transposed 1x1 convs):
// dg = W_out^T [dskip; dnet] over the gradient planes (dskip in chunks 0..S/8-1, dnet behind it), then
// dpre[filter c] = dg * sg * (1 - th^2), dpre[gate c] = dg * th * sg * (1 - sg); dpre also as planes for the input gradient.
template <bool BF, int MR, int FG = 0>      // FG 1: aux0 holds tanh * sigmoid instead of tanh; 2: ... as the gated PLANES of the forward pass
__global__ __launch_bounds__(256, MR == 8 ? 1 : 2) void gate_bwd_f16x3_kernel(const OutArgs a) {
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    const vqw_f16x3_out_desc& d = a.d;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l31 = lane & 31, lhi = lane >> 5;
    const int R = d.R, T = d.T;
    constexpr int HB = 32 * MR;
    const int n_mt = R / HB;
    const int bid = vqw_xcd_remap(blockIdx.x, gridDim.x);
    const int mt = bid % n_mt, n0 = (bid / n_mt) * 256;
    const int b = n0 / T, t0 = n0 - b * T;
    f32x16 acc[MR][2];
    {
        LoopGeom g;
        g.wp = d.wp; g.xp = d.xp; g.M = R; g.Cin = d.Cin; g.ks = 1; g.dilation = 1; g.NB = a.NB;
        g.m_row0 = mt * HB; g.n0 = n0; g.t0 = t0;
        g.xKC = d.xp_KC > 0 ? d.xp_KC : d.Cin / 8; g.xkc0 = d.xp_kc0; g.dir = 1; g.T = T;
        f16x3_mainloop<BF, MR>(acc, smem, g, wv, lane);
    }
    const int tcol = t0 + 64 * wv + l31;
    const float ps = (d.plane_scale > 0.0f ? d.plane_scale : 1.0f) * dev_scale(d.out_scale);
    const float winv = inv_scales(d.w_scale_inv, d.x_scale, d.w_scale);
    const int PKC = d.planes_KC > 0 ? d.planes_KC : 2 * R / 8;
    const int AKC = d.aux0_KC > 0 ? d.aux0_KC : R / 8;
    // The saved activations of group g + 2 are requested before group g is stored (x3_epilogue_pipeline); aux0 as planes: this
    // lane's four channels of one (batch, time) row = 8 bytes of the row's plane entry (store_plane_quad's layout), kept as
    // loaded and decoded when the group is computed.
    struct Ops { float th[2][4], sg[2][4]; uint2 h1[2], h2[2]; };
    // STEP: what the training step asks for -- planes only, no fp32 dpre -- known at compile time: no branch around any store.
    // Every other combination takes the same body with its block-uniform conditions tested at run time.
    auto epilogue = [&](auto step_c) {
        constexpr bool STEP = decltype(step_c)::value;
        const bool w32 = STEP ? false : d.net_out != nullptr, wpl = STEP ? true : d.net_out_planes != nullptr;
        float gmax = 0.0f;
        bool gbad = false;
        auto request = [&](int g, Ops& o) {
            const int i = g >> 2, v4 = g & 3;
            const int c0 = mt * HB + 32 * i + 8 * v4 + 4 * lhi;      // first of this lane's four gated channels
            const size_t offa = ((size_t)b * R + c0) * T + tcol;      // saved tanh / sigmoid [B][R][T]
            const float* pg = d.aux1 + offa;
            if constexpr (FG == 2) {
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const char* pe = reinterpret_cast<const char*>(d.aux0) + ((size_t)(d.aux0_kc0 + c0 / 8) * a.NB + n0 + 64 * wv + 32 * j + l31) * 16 + lhi * 8;
                    o.h1[j] = *reinterpret_cast<const uint2*>(pe);
                    if constexpr (!BF) o.h2[j] = *reinterpret_cast<const uint2*>(pe + (size_t)AKC * a.NB * 16);
                }
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int j = 0; j < 2; ++j) o.sg[j][e] = pg[e * T + 32 * j];
            } else {
                const float* pt = d.aux0 + offa;
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int j = 0; j < 2; ++j) { o.th[j][e] = pt[e * T + 32 * j]; o.sg[j][e] = pg[e * T + 32 * j]; }
            }
        };
        auto finish = [&](int g, const Ops& o) {
            const int i = g >> 2, v4 = g & 3;
            const int c0 = mt * HB + 32 * i + 8 * v4 + 4 * lhi;
            const size_t offo = ((size_t)b * 2 * R + c0) * T + tcol;  // dpre [B][2R][T]: filter rows, then gate rows
            float* pf = d.net_out + offo;
            float* pq = pf + (size_t)R * T;
            float th[2][4], sg[2][4], qf[2][4], qg[2][4];
            if constexpr (FG == 2) {
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const uint2 h1 = o.h1[j];
                    // (no local arrays here: indexed ones kept the 256-row instantiation from unrolling and put the accumulators in scratch)
                    if constexpr (BF) {
                        th[j][0] = __uint_as_float(h1.x << 16); th[j][1] = __uint_as_float(h1.x & 0xffff0000u);
                        th[j][2] = __uint_as_float(h1.y << 16); th[j][3] = __uint_as_float(h1.y & 0xffff0000u);
                    } else {
                        const uint2 h2 = o.h2[j];
                        auto lo16 = [](unsigned w) { return (float)__builtin_bit_cast(_Float16, (u16)(w & 0xffffu)); };
                        auto hi16 = [](unsigned w) { return (float)__builtin_bit_cast(_Float16, (u16)(w >> 16)); };
                        th[j][0] = lo16(h1.x) + lo16(h2.x); th[j][1] = hi16(h1.x) + hi16(h2.x);
                        th[j][2] = lo16(h1.y) + lo16(h2.y); th[j][3] = hi16(h1.y) + hi16(h2.y);
                    }
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int j = 0; j < 2; ++j) th[j][e] = o.th[j][e];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int j = 0; j < 2; ++j) sg[j][e] = o.sg[j][e];
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const float dg = acc[i][j][v4 * 4 + e] * winv;
                    if constexpr (FG != 0) {
                        // th[][] holds g = tanh * sigmoid (the forward pass did not store tanh):
                        //   sg (1 - tanh^2) = sg - g^2 / sg  (0 where the sigmoid underflowed),   tanh sg (1 - sg) = g (1 - sg)
                        const float g_ = th[j][e], sv = sg[j][e];
                        // (a DENORMAL sigmoid -- gate pre-activations near -88 -- has an infinite v_rcp_f32 while g^2 underflows to
                        // zero: 0 * inf = NaN; below the smallest normal number the factor is taken as 0, like an underflowed sigmoid)
                        const float ff = sv >= 1.17549435e-38f ? sv - g_ * g_ * __builtin_amdgcn_rcpf(sv) : 0.0f;
                        qf[j][e] = dg * ff;
                        qg[j][e] = dg * g_ * (1.0f - sv);
                    } else {
                        qf[j][e] = dg * sg[j][e] * (1.0f - th[j][e] * th[j][e]);
                        qg[j][e] = dg * th[j][e] * sg[j][e] * (1.0f - sg[j][e]);
                    }
                    // (the fp32 values themselves go into the planes, also where no fp32 dpre is stored: unpinned, the planes-only body
                    // contracts these products into the fp16 conversions and the plane bits change)
                    if constexpr (STEP) asm volatile("" : "+v"(qf[j][e]), "+v"(qg[j][e]));
                    // (a NaN / inf in dg or in the saved activations shows in qf / qg: the check below sees it)
                    if (w32) {       // fp32 dpre only where somebody reads it (the batched weight gradients read the planes)
                        pf[e * T + 32 * j] = qf[j][e];
                        pq[e * T + 32 * j] = qg[j][e];
                    }
                }
            if (wpl) {
                // The max-abs / finiteness folds sit HERE, next to the plane stores and under the same condition, and are pinned by
                // an empty asm: written in the arithmetic loop above, the optimiser sank them into the conditional guard_report at the
                // end of the kernel and kept every qf / qg of the whole epilogue alive until then -- 150 (128-row blocks) to 290
                // (256-row) spilled registers, 600-1200 bytes of scratch per lane (round 2's "spill-ridden epilogue").
                float gm = 0.0f;
                bool bad = false;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        gm = fmaxf(gm, fmaxf(fabsf(qf[j][e]), fabsf(qg[j][e])));
                        bad |= !(fabsf(qf[j][e]) <= 3.0e38f) || !(fabsf(qg[j][e]) <= 3.0e38f);
                    }
                    store_plane_quad<BF>(d.net_out_planes, PKC, a.NB, d.planes_kc0 + c0 / 8, n0 + 64 * wv + 32 * j + l31, lhi, qf[j], ps);
                    store_plane_quad<BF>(d.net_out_planes, PKC, a.NB, d.planes_kc0 + (R + c0) / 8, n0 + 64 * wv + 32 * j + l31, lhi, qg[j], ps);
                }
                gmax = fmaxf(gmax, gm);
                int gb_i = (int)gbad | (int)bad;
                asm volatile("" : "+v"(gmax), "+v"(gb_i));
                gbad = gb_i != 0;
            }
        };
        x3_epilogue_pipeline<MR * 4, EPI_DEPTH, Ops>(request, finish);
        if (wpl) guard_report(gmax, gbad, ps, d.out_amax, d.flag);
    };
    // (the compile-time body where the training step runs: aux0 as planes.  Not FG 0 / 1 and not the 256-row fp16 instantiation, whose
    // planes-only bodies need more scratch than the run-time body -- 870 and 8 bytes per lane)
    constexpr bool HAS_STEP = FG == 2 && (MR == 4 || BF);
    if (HAS_STEP && !d.net_out && d.net_out_planes) epilogue(std::integral_constant<bool, HAS_STEP>{});
    else epilogue(std::false_type{});
}

}  // namespace

int x3_gate_bwd_launch(const vqw_f16x3_out_desc& d, hipStream_t st) {
    OutArgs a;
    a.d = d;
    a.NB = d.B * d.T;
    const bool bf = (d.mode & 1) != 0, half = (d.mode & VQW_X3_HALF_BLOCKS) != 0;
    typedef void (*kfn_t)(OutArgs);
    const kfn_t kbwds[4] = {gate_bwd_f16x3_kernel<false, 8>, gate_bwd_f16x3_kernel<true, 8>, gate_bwd_f16x3_kernel<false, 4>, gate_bwd_f16x3_kernel<true, 4>};
    kfn_t kfn = kbwds[(bf ? 1 : 0) + (half ? 2 : 0)];
    if (d.flags & 6) {
        const bool pl = (d.flags & 4) != 0;      // bit 2: aux0 = the gated planes (bit 1: tanh * sigmoid as fp32)
        const kfn_t kg[8] = {gate_bwd_f16x3_kernel<false, 8, 1>, gate_bwd_f16x3_kernel<false, 4, 1>, gate_bwd_f16x3_kernel<false, 8, 2>,
                             gate_bwd_f16x3_kernel<false, 4, 2>, gate_bwd_f16x3_kernel<true, 8, 2>, gate_bwd_f16x3_kernel<true, 4, 2>,
                             gate_bwd_f16x3_kernel<true, 8, 1>, gate_bwd_f16x3_kernel<true, 4, 1>};
        kfn = kg[(pl ? (bf ? 4 : 2) : (bf ? 6 : 0)) + (half ? 1 : 0)];
    }
    const int lds = half ? X3Shape<4>::LDS_BYTES : X3Shape<8>::LDS_BYTES, hb = half ? 128 : 256;
    return x3_launch(kfn, (d.R / hb) * (a.NB / 256), lds, st, a, "vqw_f16x3_out_conv");
}
