// Dynamic time warping between two cepstral sequences for gfx950 (mel-cepstral distortion, scoring.mcd): the accumulated
// cost and the length of the optimal path, one workgroup per pair.  The contract is in include/vqwave.h; every floating-point
// operation below is one correctly rounded fp32 operation in a fixed order, so tests/dtw_ref.py restates it bit for bit.
#include "vqw_common.h"

// c(i, j) is a sum of separately rounded squares: a fused multiply-add would round once where the contract rounds twice
#pragma clang fp contract(off)

namespace {

constexpr int DTW_THREADS = 256;
constexpr int DTW_MAX_T = 4096;        // 3 diagonals x 4096 cells x 8 bytes = 96 KiB of the CU's 160 KiB LDS

struct __attribute__((aligned(8))) DtwCell {
    float cost;      // Dp(i, j)
    int steps;       // n(i, j): cells on the path chosen up to and including (i, j)
};

// Anti-diagonal k = i + j holds the cells max(0, k - (nb - 1)) <= i <= min(na - 1, k); cell (i, j) lives at index i of buffer
// k % 3.  Its predecessors: (i-1, j-1) at index i-1 of diagonal k-2; (i-1, j) and (i, j-1) at indices i-1 and i of diagonal
// k-1.  Diagonal k overwrites the buffer of diagonal k-3, which nobody reads any more once the barrier after diagonal k-1 is
// passed: ONE barrier per diagonal.  The three LDS reads are unconditional (index i-1 clamped to 0, so they stay inside the
// buffer) and a predecessor that does not exist is masked out afterwards: what an unwritten entry holds never matters, and
// the LDS needs no initialisation.  Lanes run along i: a[d][i] is read ascending, b[d][k - i] descending, both contiguous.
// DS > 0: D is the compile-time DS and the 2 * DS loads of a cell are in flight together; DS == 0: any D, four terms at a time.
// The arithmetic is written with plain operators under the pragma above (the __f*_rn device functions are inlined from a
// header compiled with contraction on, and a multiply and an add from there DO fuse; __fsqrt_rn there is the hardware's
// 1-ulp square root, sqrtf the correctly rounded one).
template <int DS>
__global__ __launch_bounds__(DTW_THREADS) void cepstral_dtw_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                   const int32_t* __restrict__ na_p, const int32_t* __restrict__ nb_p,
                                                                   float* __restrict__ cost, int32_t* __restrict__ steps, int C, int d0,
                                                                   int D, int Ta, int Tb) {
    extern __shared__ __attribute__((aligned(8))) char dtw_smem[];
    DtwCell* diag = reinterpret_cast<DtwCell*>(dtw_smem);       // [3][Ta]
    const int p = blockIdx.x;
    const int na = na_p ? min(max(na_p[p], 1), Ta) : Ta;
    const int nb = nb_p ? min(max(nb_p[p], 1), Tb) : Tb;
    const float* ap = a + ((size_t)p * C + d0) * Ta;
    const float* bp = b + ((size_t)p * C + d0) * Tb;
    DtwCell* cur = diag;                     // diagonal k
    DtwCell* prev1 = diag + 2 * (size_t)Ta;  // diagonal k - 1
    DtwCell* prev2 = diag + (size_t)Ta;      // diagonal k - 2
    const int nk = na + nb - 1;
    for (int k = 0; k < nk; ++k) {
        const int ilo = max(0, k - (nb - 1)), ihi = min(na - 1, k);
        for (int i = ilo + (int)threadIdx.x; i <= ihi; i += DTW_THREADS) {
            const int j = k - i;
            const float* ai = ap + i;
            const float* bj = bp + j;
            float sum = 0.0f;
            if (DS > 0) {
                float va[DS > 0 ? DS : 1], vb[DS > 0 ? DS : 1];
#pragma unroll
                for (int d = 0; d < DS; ++d) {
                    va[d] = ai[(size_t)d * Ta];
                    vb[d] = bj[(size_t)d * Tb];
                }
#pragma unroll
                for (int d = 0; d < DS; ++d) {
                    const float x = va[d] - vb[d];
                    const float sq = x * x;
                    sum = sum + sq;
                }
            } else {
                int d = 0;
                for (; d + 4 <= D; d += 4) {
                    float va[4], vb[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        va[e] = ai[(size_t)(d + e) * Ta];
                        vb[e] = bj[(size_t)(d + e) * Tb];
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float x = va[e] - vb[e];
                        const float sq = x * x;
                        sum = sum + sq;
                    }
                }
                for (; d < D; ++d) {
                    const float x = ai[(size_t)d * Ta] - bj[(size_t)d * Tb];
                    const float sq = x * x;
                    sum = sum + sq;
                }
            }
            const float c = sqrtf(sum);      // correctly rounded (hipcc's default for fp32 sqrt); __fsqrt_rn is the native one
            const int im = max(i - 1, 0);
            const DtwCell vd = prev2[im], vu = prev1[im], vl = prev1[i];      // (i-1, j-1), (i-1, j), (i, j-1)
            DtwCell best = vd;
            bool have = i > 0 && j > 0;
            if (i > 0 && (!have || vu.cost < best.cost)) best = vu;
            have = have || i > 0;
            if (j > 0 && (!have || vl.cost < best.cost)) best = vl;
            have = have || j > 0;
            DtwCell out;
            out.cost = have ? c + best.cost : c;
            out.steps = have ? best.steps + 1 : 1;
            cur[i] = out;
            if (k == nk - 1) {      // the one cell (na - 1, nb - 1)
                cost[p] = out.cost;
                steps[p] = out.steps;
            }
        }
        __syncthreads();
        DtwCell* const t = prev2;
        prev2 = prev1;
        prev1 = cur;
        cur = t;
    }
}

}  // namespace

// ============================================================================ C ABI
extern "C" int vqw_cepstral_dtw(const float* a, const float* b, const int32_t* na, const int32_t* nb, float* cost, int32_t* steps,
                                int P, int C, int d0, int D, int Ta, int Tb, vqw_stream_t s) {
    VQW_CHECK(a && b && cost && steps, "vqw_cepstral_dtw: null pointer (a=%p b=%p cost=%p steps=%p)", (const void*)a, (const void*)b,
              (void*)cost, (void*)steps);
    VQW_CHECK(P >= 1, "vqw_cepstral_dtw: P=%d must be at least 1", P);
    VQW_CHECK(D >= 1, "vqw_cepstral_dtw: D=%d must be at least 1", D);
    VQW_CHECK(d0 >= 0, "vqw_cepstral_dtw: d0=%d must not be negative", d0);
    VQW_CHECK((int64_t)d0 + D <= C, "vqw_cepstral_dtw: channels d0=%d .. d0+D=%lld exceed C=%d", d0, (long long)d0 + D, C);
    VQW_CHECK(Ta >= 1 && Ta <= DTW_MAX_T, "vqw_cepstral_dtw: Ta=%d must be in 1..%d", Ta, DTW_MAX_T);
    VQW_CHECK(Tb >= 1 && Tb <= DTW_MAX_T, "vqw_cepstral_dtw: Tb=%d must be in 1..%d", Tb, DTW_MAX_T);
    const size_t lds = (size_t)3 * Ta * sizeof(DtwCell);
    // the 12 coefficients of the MCD (and all 13) get a kernel with D known at compile time; any other D the general one
    auto kfn = D == 12 ? cepstral_dtw_kernel<12> : D == 13 ? cepstral_dtw_kernel<13> : cepstral_dtw_kernel<0>;
    // per call: the attribute belongs to the current device's copy of the kernel (no process-wide "done" flag)
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize,
                            3 * DTW_MAX_T * (int)sizeof(DtwCell)) != hipSuccess)
        return vqw_set_error("vqw_cepstral_dtw: hipFuncSetAttribute failed");
    hipLaunchKernelGGL(kfn, dim3(P), dim3(DTW_THREADS), lds, (hipStream_t)s, a, b, na, nb, cost, steps, C, d0, D, Ta, Tb);
    VQW_LAUNCH_CHECK("vqw_cepstral_dtw");
    return 0;
}
