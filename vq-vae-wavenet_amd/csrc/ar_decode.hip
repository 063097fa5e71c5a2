// Fast autoregressive WaveNet generation for gfx950 -- replaces the per-sample
// sess.run([predictions, push_ops]) of generate.py:103-113 and the graph built by
// wavenet.py:103-172 / wavenet_ops.py:147-267 (216 tf.matmul + 91 FIFOQueue ops per sample)
// and the host-side numpy sampling of utils.py:13-46.
//
// Design (round 1): every FIFOQueue becomes a device ring buffer indexed by a DEVICE-resident
// step counter, so one sample step is a fixed sequence of kernels with no per-step host
// arguments; that sequence is captured once into a hipGraph and replayed per sample.  The
// local-condition 1x1s (fast_condition, wavenet_ops.py:198-209) only change every `ratio`
// samples and are pre-computed for the whole utterance with the MFMA conv engine.
// Matrix-vector products stream the fp32 weights (L2 / Infinity-Cache resident after the
// first step) with 16-byte loads, 16 output columns per workgroup.
#include <string.h>

#include "ar_host.h"
#include "ar_persist.h"

namespace {

constexpr int MAXB = 8;

struct ArState {  // device resident
    int step;     // samples generated since reset
    int run_base; // value of step when the current run started
    int Tz, ratio, mode, n_steps;
    const float* uniforms;
    float* audio;
    int* indices;
    float* probs_last;
    ArSampleRow samp[MAXB];   // per-row temperature / top-k / top-p (ar_sampling.h); .on = 0: the default path
};

struct GemvSeg {
    const float* w;  // [K][ldw]
    const float* x;  // [B][K] (plain) or ring base [depth][B][K]
    int K, ldw;
    int depth;       // 0 = plain vector
    int phase;       // ring slot = (step + phase) % depth
};

enum { MODE_PLAIN = 0, MODE_GATE = 1, MODE_OUT = 2 };

struct GemvArgs {
    GemvSeg seg[VQW_MAX_TAPS];
    int nseg, B, N, H, S;      // N total columns; H gate half; S skip width (MODE_OUT)
    int in_relu;
    const float* bias;
    const float* cond;         // [B][N][Tz] or null
    float* out;                // PLAIN: [B][N]; GATE: gated [B][H]; OUT: skip [B][S]
    float* cur;                // OUT: [B][N-S] residual state (in place)
    float* ring_w;             // OUT: ring of this layer [depth][B][N-S]
    int ring_depth;
    const ArState* st;
};

// wavenet.py:113-124: x = mu_law_encode(input_t); fast_conv1d(k=pre_k, dilation 1, Cin=1).
__global__ void ar_pre_kernel(const ArState* st, const float* prev, float* xring, const float* pre_w,
                              const float* pre_b, float* cur, int pre_k, int R, const VqwMu mu) {
    __shared__ float taps[64];
    const int b = blockIdx.x;
    const int step = st->step;
    float* ring = xring + (size_t)b * pre_k;
    const float x_new = vqw_mu_encode_m(prev[b], mu);
    if (threadIdx.x < pre_k) {
        const int j = threadIdx.x;                      // tap j multiplies x(t - (pre_k-1-j))
        const int tau = step - (pre_k - 1 - j);
        const int slot = ((tau % pre_k) + pre_k) % pre_k;
        taps[j] = (j == pre_k - 1) ? x_new : ring[slot];
        if (j == pre_k - 1) ring[slot] = x_new;         // push (the slot of t - pre_k, no longer needed)
    }
    __syncthreads();
    for (int o = threadIdx.x; o < R; o += blockDim.x) {
        float acc = pre_b[o];
#pragma unroll 8
        for (int j = 0; j < pre_k; ++j) acc = fmaf(pre_w[(size_t)j * R + o], taps[j], acc);
        cur[(size_t)b * R + o] = acc;
    }
}

// out[b][n] = sum_seg sum_k w[k][n] x[b][k]  (+bias +cond), 16 columns per block.
template <int MODE>
__global__ __launch_bounds__(256) void ar_gemv_kernel(const GemvArgs a) {
    extern __shared__ float sm[];
    const int tid = threadIdx.x;
    const int kl = tid >> 2, cq = tid & 3;
    const int step = a.st->step;
    const int B = a.B;
    // column base of this thread's 4 columns
    int col;
    if (MODE == MODE_GATE) {
        const int g0 = blockIdx.x * 8;
        col = (cq < 2) ? g0 + 4 * cq : a.H + g0 + 4 * (cq - 2);
    } else {
        col = blockIdx.x * 16 + 4 * cq;
    }
    const bool colok = (MODE == MODE_GATE) ? (blockIdx.x * 8 + 4 * (cq & 1) < a.H) : (col < a.N);

    float acc[MAXB][4];
#pragma unroll
    for (int b = 0; b < MAXB; ++b)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[b][e] = 0.0f;

    // The per-sample chain is latency-bound: stage the input vectors of ALL segments behind one
    // barrier, then issue every weight load of a segment before the first one is consumed
    // (K <= 256 per segment in the default model: 4 loads in flight per thread and segment).
    float* xs = sm;  // [seg][B][K]
    {
        int off = 0;
        for (int sgi = 0; sgi < a.nseg; ++sgi) {
            const GemvSeg& sg = a.seg[sgi];
            const float* xp = sg.x;
            if (sg.depth > 0) xp += (size_t)((step + sg.phase) % sg.depth) * B * sg.K;
            for (int i = tid; i < B * sg.K; i += 256) {
                const float v = xp[i];
                xs[off + i] = a.in_relu ? fmaxf(v, 0.0f) : v;
            }
            off += B * sg.K;
        }
    }
    __syncthreads();
    if (colok) {
        int off = 0;
        for (int sgi = 0; sgi < a.nseg; ++sgi) {
            const GemvSeg& sg = a.seg[sgi];
            const float* wc = sg.w + col;
            for (int k0 = 0; k0 < sg.K; k0 += 256) {
                f32x4 w4[4];
                int kc[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int kk = k0 + kl + 64 * u;
                    kc[u] = min(kk, sg.K - 1);
                    w4[u] = *reinterpret_cast<const f32x4*>(wc + (size_t)kc[u] * sg.ldw);
                    if (kk >= sg.K) w4[u] = f32x4{0, 0, 0, 0};
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
#pragma unroll
                    for (int b = 0; b < MAXB; ++b) {
                        if (b < B) {
                            const float xv = xs[off + b * sg.K + kc[u]];
#pragma unroll
                            for (int e = 0; e < 4; ++e) acc[b][e] = fmaf(w4[u][e], xv, acc[b][e]);
                        }
                    }
                }
            }
            off += B * sg.K;
        }
    }
    // reduce over the 64 k-lanes: lanes of one wave hold kl = 16w..16w+15 (4 lanes each)
#pragma unroll
    for (int b = 0; b < MAXB; ++b) {
        if (b < B) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float v = acc[b][e];
                v += __shfl_xor(v, 4);
                v += __shfl_xor(v, 8);
                v += __shfl_xor(v, 16);
                v += __shfl_xor(v, 32);
                acc[b][e] = v;
            }
        }
    }
    __syncthreads();
    float* red = sm;  // [4 waves][B][16]
    const int lane = tid & 63, wv = tid >> 6;
    if (lane < 4) {
#pragma unroll
        for (int b = 0; b < MAXB; ++b)
            if (b < B)
#pragma unroll
                for (int e = 0; e < 4; ++e) red[(wv * B + b) * 16 + 4 * lane + e] = acc[b][e];
    }
    __syncthreads();
    const bool worker = tid < 16 * B;  // one thread per (batch row, result column)
    const int b = worker ? tid / 16 : 0, c = tid % 16;
    float v = 0.0f;
    if (worker)
        v = red[(0 * B + b) * 16 + c] + red[(1 * B + b) * 16 + c] + red[(2 * B + b) * 16 + c] +
            red[(3 * B + b) * 16 + c];
    // global column of result slot c
    int n;
    if (MODE == MODE_GATE) n = (c < 8) ? blockIdx.x * 8 + c : a.H + blockIdx.x * 8 + (c - 8);
    else n = blockIdx.x * 16 + c;
    const bool ok = worker && ((MODE == MODE_GATE) ? (blockIdx.x * 8 + (c & 7) < a.H) : (n < a.N));
    if (ok) {
        if (a.bias) v += a.bias[n];
        if (a.cond) {
            int frame = step / a.st->ratio;
            if (frame >= a.st->Tz) frame = a.st->Tz - 1;
            v += a.cond[((size_t)b * a.N + n) * a.st->Tz + frame];
        }
    }
    if (MODE == MODE_GATE) {
        __syncthreads();  // every thread of the block reaches both barriers
        if (worker) red[b * 16 + c] = v;
        __syncthreads();
        if (c < 8 && ok) {
            const float vf = red[b * 16 + c], vg = red[b * 16 + c + 8];
            const float th = 1.0f - 2.0f / (__expf(2.0f * vf) + 1.0f);
            const float sg = 1.0f / (1.0f + __expf(-vg));
            a.out[(size_t)b * a.H + n] = th * sg;
        }
    } else if (MODE == MODE_OUT) {
        if (ok) {
            if (n < a.S) {
                a.out[(size_t)b * a.S + n] += v;  // skip += skip_out   (wavenet.py:142)
            } else {
                const int R = a.N - a.S, r = n - a.S;
                const float old = a.cur[(size_t)b * R + r];
                if (a.ring_w) a.ring_w[((size_t)(step % a.ring_depth) * B + b) * R + r] = old;  // push
                a.cur[(size_t)b * R + r] = old + v;  // current += res_out (wavenet.py:143)
            }
        }
    } else {
        if (ok) a.out[(size_t)b * a.N + n] = v;
    }
}

// softmax (wavenet.py:171) + utils.decode (utils.py:30-46) + mu_law_decode_np; advances the step.
__global__ __launch_bounds__(256) void ar_sample_kernel(ArState* st, const float* logits, float* probs,
                                                        float* prev, int B, int Q, const VqwMu mu) {
    __shared__ float sp[1024];
    __shared__ float redv[4];
    __shared__ int redi[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int step = st->step;
    const int i_out = step - st->run_base;
    for (int b = 0; b < B; ++b) {
        const float* lg = logits + (size_t)b * Q;
        if (st->samp[b].on) {              // block-uniform; wave 0 samples the row (ar_sampling.h), the others wait
            if (wv == 0) {                 // (sp is this wave's alone: thread 0, the last reader of the row before, is in it)
                for (int q = lane; q < Q; q += 64) sp[q] = lg[q];
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // lanes read each other's LDS writes (same wave)
                const int idx = ar_sample_truncated(sp, Q, st->samp[b], st->uniforms[(size_t)b * st->n_steps + i_out],
                                                    st->probs_last ? st->probs_last + (size_t)b * Q : probs + (size_t)b * Q);
                if (lane == 0) {
                    const float dec = vqw_mu_decode_m((float)idx, mu);
                    if (st->audio) st->audio[(size_t)b * st->n_steps + i_out] = dec;
                    if (st->indices) st->indices[(size_t)b * st->n_steps + i_out] = idx;
                    prev[b] = dec;
                }
            }
            __syncthreads();
            continue;
        }
        // a default row (ar_sample_default); p goes to probs every step, and to probs_last whenever that is set
        const int mode = st->mode;
        const int idx = ar_sample_default(lg, 1, sp, redv, redi, Q, mode, mode ? st->uniforms + (size_t)b * st->n_steps + i_out : nullptr,
                                          probs + (size_t)b * Q, st->probs_last ? st->probs_last + (size_t)b * Q : nullptr);
        if (tid == 0) {
            const float dec = vqw_mu_decode_m((float)idx, mu);
            if (st->audio) st->audio[(size_t)b * st->n_steps + i_out] = dec;
            if (st->indices) st->indices[(size_t)b * st->n_steps + i_out] = idx;
            prev[b] = dec;
        }
    }
    if (tid == 0) st->step = step + 1;
}

}  // namespace

struct vqw_ar_decoder : ArTables {
    int B = 0;
    // device state
    ArState* st = nullptr;
    float *prev = nullptr, *xring = nullptr, *cur = nullptr, *gated = nullptr, *skip = nullptr,
          *h = nullptr, *logits = nullptr, *probs = nullptr;
    std::vector<float*> rings;   // per layer [depth][B][R]
    std::vector<float*> condenc; // per layer [B][2R][Tz]; last entry = postprocess1 [B][S][Tz]
    int cond_Tz_cap = 0;
    hipStream_t stream = nullptr;  // private stream (graph capture is illegal on the null stream)
    hipEvent_t ev_in = nullptr, ev_out = nullptr;
    ArGraph step;                  // launch_step, captured
    bool use_graph = true;
    ArPersist* persist = nullptr;  // persistent single-launch generator (default model shapes)
    bool pending = false;          // a run has been enqueued and not yet waited for
    hipStream_t run_stream = nullptr;   // the stream that run was enqueued on (a group run: the first handle's)
    int n_codes = 0;               // > 0: code-input mode of the latent prior (persistent kernel only, vqw_ar_prior_create)
    VqwMu mu = {256, 255.0f, 5.5451774444795623f};   // the mu-law level of an audio handle (vqw_ar_decode_set_levels)
};

namespace {

int launch_step(vqw_ar_decoder* h, hipStream_t st) {
    const vqw_ar_weights& w = h->w;
    const int B = h->B, R = w.R, S = w.S, Q = w.Q, ks = w.kernel_size;
    hipLaunchKernelGGL(ar_pre_kernel, dim3(B), dim3(256), 0, st, h->st, h->prev, h->xring, w.pre_w, w.pre_b,
                       h->cur, w.pre_k, R, h->mu);
    GemvArgs a;
    // skip = linear(current)  (wavenet.py:127-128)
    memset(&a, 0, sizeof(a));
    a.seg[0] = GemvSeg{w.skip0_w, h->cur, R, S, 0, 0};
    a.nseg = 1; a.B = B; a.N = S; a.bias = w.skip0_b; a.out = h->skip; a.st = h->st;
    hipLaunchKernelGGL((ar_gemv_kernel<MODE_PLAIN>), dim3(vqw_cdiv(S, 16)), dim3(256), B * R * sizeof(float) + 4 * MAXB * 16 * sizeof(float), st, a);
    for (int l = 0; l < w.n_layers; ++l) {
        const int d = h->dil[l];
        const int depth = (ks - 1) * d;
        // fast_gated_cnn (wavenet_ops.py:212-237)
        memset(&a, 0, sizeof(a));
        for (int j = 0; j < ks; ++j) {
            const float* wt = h->gated_w[l] + (size_t)j * R * 2 * R;
            if (j == ks - 1) a.seg[j] = GemvSeg{wt, h->cur, R, 2 * R, 0, 0};
            else a.seg[j] = GemvSeg{wt, h->rings[l], R, 2 * R, depth, j * d};  // x(t-(ks-1-j)d)
        }
        a.nseg = ks; a.B = B; a.N = 2 * R; a.H = R; a.bias = h->gated_b[l];
        a.cond = h->condenc[l]; a.out = h->gated; a.st = h->st;
        hipLaunchKernelGGL((ar_gemv_kernel<MODE_GATE>), dim3(vqw_cdiv(R, 8)), dim3(256), (size_t)ks * B * R * sizeof(float) + 4 * MAXB * 16 * sizeof(float), st, a);
        // skip / residual linears + accumulation + queue push (wavenet_ops.py:261-265, wavenet.py:142-143)
        memset(&a, 0, sizeof(a));
        a.seg[0] = GemvSeg{h->out_w[l], h->gated, R, w.out_ld, 0, 0};
        a.nseg = 1; a.B = B; a.N = S + R; a.S = S; a.bias = h->out_b[l];
        a.out = h->skip; a.cur = h->cur; a.ring_w = h->rings[l]; a.ring_depth = depth; a.st = h->st;
        hipLaunchKernelGGL((ar_gemv_kernel<MODE_OUT>), dim3(vqw_cdiv(S + R, 16)), dim3(256), B * R * sizeof(float) + 4 * MAXB * 16 * sizeof(float), st, a);
    }
    // postprocess1 (wavenet.py:152-162)
    memset(&a, 0, sizeof(a));
    a.seg[0] = GemvSeg{w.post1_w, h->skip, S, S, 0, 0};
    a.nseg = 1; a.B = B; a.N = S; a.in_relu = 1; a.bias = w.post1_b; a.cond = h->condenc[w.n_layers];
    a.out = h->h; a.st = h->st;
    hipLaunchKernelGGL((ar_gemv_kernel<MODE_PLAIN>), dim3(vqw_cdiv(S, 16)), dim3(256), B * S * sizeof(float) + 4 * MAXB * 16 * sizeof(float), st, a);
    // postprocess2 (wavenet.py:165-167)
    memset(&a, 0, sizeof(a));
    a.seg[0] = GemvSeg{w.post2_w, h->h, S, Q, 0, 0};
    a.nseg = 1; a.B = B; a.N = Q; a.in_relu = 1; a.bias = w.post2_b; a.out = h->logits; a.st = h->st;
    hipLaunchKernelGGL((ar_gemv_kernel<MODE_PLAIN>), dim3(vqw_cdiv(Q, 16)), dim3(256), B * S * sizeof(float) + 4 * MAXB * 16 * sizeof(float), st, a);
    hipLaunchKernelGGL(ar_sample_kernel, dim3(1), dim3(256), 0, st, h->st, h->logits, h->probs, h->prev, B, Q, h->mu);
    VQW_LAUNCH_CHECK("vqw_ar_decode_run(step)");
    return 0;
}

void free_all(vqw_ar_decoder* h) {
    if (!h) return;
    if (h->persist) arp_destroy(h->persist);
    h->step.drop();
    for (float* p : h->rings) (void)hipFree(p);
    for (float* p : h->condenc) (void)hipFree(p);
    float* bufs[] = {reinterpret_cast<float*>(h->st), h->prev, h->xring, h->cur, h->gated, h->skip, h->h, h->logits, h->probs};
    for (float* p : bufs) (void)hipFree(p);
    if (h->ev_in) (void)hipEventDestroy(h->ev_in);
    if (h->ev_out) (void)hipEventDestroy(h->ev_out);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

}  // namespace

static int ar_create(vqw_ar_decoder** out, const vqw_ar_weights* w, int batch, int channels_per_workgroup, int n_codes);

extern "C" int vqw_ar_decode_create(vqw_ar_decoder** out, const vqw_ar_weights* w, int batch) {
    return vqw_ar_decode_create_ex(out, w, batch, 0);
}

static int ar_create(vqw_ar_decoder** out, const vqw_ar_weights* w, int batch, int channels_per_workgroup, int n_codes) {
    VQW_CHECK(out && w, "vqw_ar_decode_create: null pointer");
    VQW_CHECK(channels_per_workgroup == 0 || channels_per_workgroup == 4 || channels_per_workgroup == 8,
              "vqw_ar_decode_create_ex: channels_per_workgroup is 0 (auto), 4 or 8 (got %d)", channels_per_workgroup);
    VQW_CHECK(batch >= 1 && batch <= MAXB, "vqw_ar_decode_create: batch=%d must be in 1..%d", batch, MAXB);
    VQW_CHECK(w->n_layers >= 1 && w->kernel_size >= 2 && w->kernel_size <= VQW_MAX_TAPS, "vqw_ar_decode_create: bad layer config");
    VQW_CHECK(w->R % 16 == 0 && w->S % 16 == 0 && w->Q % 4 == 0 && w->Cc % 16 == 0, "vqw_ar_decode_create: R,S,Cc must be multiples of 16, Q of 4");
    VQW_CHECK(w->Q <= 1024 && w->pre_k <= 64, "vqw_ar_decode_create: Q must be <= 1024 and pre_k <= 64");
    VQW_CHECK(w->pre_k >= 1 && w->dilations && w->gated_w && w->gated_b && w->cond_w && w->out_w && w->out_b, "vqw_ar_decode_create: null weight table");
    vqw_ar_decoder* h = new vqw_ar_decoder();
    h->assign(w);
    h->B = batch;
    const int L = w->n_layers;
    const char* env = getenv("VQW_AR_GRAPH");
    h->use_graph = !(env && env[0] == '0');
#define AR_ALLOC(ptr, n)                                                               \
    do {                                                                               \
        hipError_t e_ = hipMalloc((void**)&(ptr), (n) * sizeof(float));                \
        if (e_ != hipSuccess) { free_all(h); return vqw_set_error("vqw_ar_decode_create: hipMalloc failed: %s", hipGetErrorString(e_)); } \
    } while (0)
    const size_t B = batch;
    if (hipMalloc((void**)&h->st, sizeof(ArState)) != hipSuccess) { free_all(h); return vqw_set_error("vqw_ar_decode_create: hipMalloc failed"); }
    AR_ALLOC(h->prev, B);
    AR_ALLOC(h->xring, B * w->pre_k);
    AR_ALLOC(h->cur, B * w->R);
    AR_ALLOC(h->gated, B * w->R);
    AR_ALLOC(h->skip, B * w->S);
    AR_ALLOC(h->h, B * w->S);
    AR_ALLOC(h->logits, B * w->Q);
    AR_ALLOC(h->probs, B * w->Q);
    h->rings.assign(L, nullptr);
    for (int l = 0; l < L; ++l) AR_ALLOC(h->rings[l], h->ring_floats(l, batch));
    h->condenc.assign(L + 1, nullptr);
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_in, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_out, hipEventDisableTiming) != hipSuccess) {
        free_all(h);
        return vqw_set_error("vqw_ar_decode_create: stream/event creation failed");
    }
    h->n_codes = n_codes;
    if (arp_supported(w, batch)) {
        const int rc = arp_create(&h->persist, w, h->dil.data(), h->gated_w.data(), h->gated_b.data(), h->out_w.data(),
                                  h->out_b.data(), batch, channels_per_workgroup, n_codes);
        if (rc) { free_all(h); return rc; }
    } else if (n_codes > 0) {
        free_all(h);
        return vqw_set_error("vqw_ar_prior_create: code-input mode needs the persistent generator, which does not run here "
                             "(VQW_AR_PERSISTENT=0, or a shape / batch it does not support); the launch-per-phase path has no code input");
    }
    *out = h;
    return vqw_ar_decode_reset(h, nullptr);
}

extern "C" int vqw_ar_decode_create_ex(vqw_ar_decoder** out, const vqw_ar_weights* w, int batch, int channels_per_workgroup) {
    return ar_create(out, w, batch, channels_per_workgroup, 0);
}

extern "C" int vqw_ar_prior_create(vqw_ar_decoder** out, const vqw_ar_weights* w, int batch, int channels_per_workgroup, int n_codes) {
    VQW_CHECK(w && n_codes > 0 && n_codes == w->Q, "vqw_ar_prior_create: n_codes=%d must be > 0 and equal w->Q", n_codes);
    return ar_create(out, w, batch, channels_per_workgroup, n_codes);
}

// The mu-law level of an audio handle: 256 after every create call, whatever w->Q is.  Every check comes before any device call.
extern "C" int vqw_ar_decode_set_levels(vqw_ar_decoder* h, int levels) {
    VqwMu m;
    const int rc = ar_levels_check("vqw_ar_decode", h, levels, &m);
    if (rc) return rc;
    if (m.levels == h->mu.levels) return 0;
    h->mu = m;
    if (h->persist) arp_set_levels(h->persist, m);
    h->step.drop();   // the captured step carries the level as a kernel argument
    return 0;
}

extern "C" int vqw_ar_decode_reset(vqw_ar_decoder* h, vqw_stream_t s) {
    VQW_CHECK(h, "vqw_ar_decode_reset: null handle");
    if (h->pending) {
        const int rcw = vqw_ar_decode_wait(h);
        if (rcw) return rcw;
    }
    hipStream_t st = (hipStream_t)s;
    const size_t B = h->B;
    if (h->persist) {
        const int rc = arp_reset(h->persist, st);
        if (rc) return rc;
    }
    HIPC(hipMemsetAsync(h->st, 0, sizeof(ArState), st));
    HIPC(hipMemsetAsync(h->prev, 0, B * sizeof(float), st));       // audio = zeros (generate.py:103)
    HIPC(hipMemsetAsync(h->xring, 0, B * h->w.pre_k * sizeof(float), st));
    for (int l = 0; l < h->w.n_layers; ++l)
        HIPC(hipMemsetAsync(h->rings[l], 0, h->ring_floats(l, h->B) * sizeof(float), st));
    return 0;
}

namespace {

// Prefill of the launch-per-phase rings: layer l's inputs at steps t_lo .. t_lo+nt-1, slot tau % depth (depth = (ks-1) d:
// the slot the gate kernel reads as tap x(t - (ks-1) d) and MODE_OUT pushes).  x [B][R][ld], column tau - t_first.
__global__ void ar_prefill_ring_kernel(float* ring, int depth, int BR, const float* __restrict__ x, int ld, int t_first, int t_lo,
                                       int nt) {
    const size_t n = (size_t)BR * nt;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t bc = i / nt;                          // b * R + c
        const int tau = t_lo + (int)(i - bc * nt);
        ring[(size_t)(tau % depth) * BR + bc] = x[bc * ld + (tau - t_first)];
    }
}

// The preprocess queue (slot tau % pre_k = x_in(tau) = mu_law_encode(a[tau - 1]) for tau in (t_end - pre_k, t_end]), the
// last sample and the step counter.  tail[b][j] is a[t_end - pre_k + j]; entries before step 0 keep the reset's zeros.
// audio_tail NULL (a code-mode handle, whose history lives in the persistent kernel): only the step counter.
__global__ void ar_prefill_finish_kernel(ArState* st, float* prev, float* xring, int B, int pre_k, int t_end,
                                         const float* audio_tail, const VqwMu mu) {
    if (audio_tail) {
        for (int i = threadIdx.x; i < B * pre_k; i += blockDim.x) {
            const int b = i / pre_k, s = t_end - pre_k + i % pre_k;
            if (s >= 0) xring[b * pre_k + (s + 1) % pre_k] = vqw_mu_encode_m(audio_tail[i], mu);
        }
        if (t_end > 0)
            for (int b = threadIdx.x; b < B; b += blockDim.x) prev[b] = audio_tail[b * pre_k + pre_k - 1];
    }
    if (threadIdx.x == 0) st->step = t_end;
}

}  // namespace

extern "C" int vqw_ar_decode_prefill_layer(vqw_ar_decoder* h, int l, const float* x, int ld, int t_first, int t_end,
                                           vqw_stream_t s) {
    VQW_CHECK(h, "vqw_ar_decode_prefill_layer: null handle");
    VQW_CHECK(l >= 0 && l < h->w.n_layers, "vqw_ar_decode_prefill_layer: layer %d outside 0..%d", l, h->w.n_layers - 1);
    VQW_CHECK(t_end >= 0, "vqw_ar_decode_prefill_layer: t_end=%d < 0", t_end);
    const int span = (h->w.kernel_size - 1) * h->dil[l];
    const int t_lo = t_end > span ? t_end - span : 0;
    VQW_CHECK(t_first >= 0 && t_first <= t_lo && ld >= t_end - t_first,
              "vqw_ar_decode_prefill_layer: columns [%d, %d) do not cover layer %d's steps [%d, %d)", t_first, t_first + ld, l,
              t_lo, t_end);
    if (t_end == t_lo) return 0;
    VQW_CHECK(x, "vqw_ar_decode_prefill_layer: null x");
    if (h->pending) {
        const int rcw = vqw_ar_decode_wait(h);
        if (rcw) return rcw;
    }
    hipStream_t st = (hipStream_t)s;
    if (h->persist) return arp_prefill_layer(h->persist, l, x, ld, t_first, t_lo, t_end, st);
    const int BR = h->B * h->w.R, nt = t_end - t_lo;
    const int blocks = (int)(((size_t)BR * nt + 255) / 256 < 2048 ? ((size_t)BR * nt + 255) / 256 : 2048);
    hipLaunchKernelGGL(ar_prefill_ring_kernel, dim3(blocks), dim3(256), 0, st, h->rings[l], span, BR, x, ld, t_first, t_lo, nt);
    VQW_LAUNCH_CHECK("vqw_ar_decode_prefill_layer");
    return 0;
}

extern "C" int vqw_ar_decode_prefill_finish(vqw_ar_decoder* h, int t_end, const float* audio_tail, const int32_t* code_tail,
                                            vqw_stream_t s) {
    VQW_CHECK(h, "vqw_ar_decode_prefill_finish: null handle");
    VQW_CHECK(t_end >= 0, "vqw_ar_decode_prefill_finish: t_end=%d < 0", t_end);
    VQW_CHECK((audio_tail == nullptr) != (code_tail == nullptr),
              "vqw_ar_decode_prefill_finish: exactly one of audio_tail / code_tail must be given");
    VQW_CHECK(h->n_codes > 0 ? code_tail != nullptr : audio_tail != nullptr,
              "vqw_ar_decode_prefill_finish: a %s handle takes %s", h->n_codes > 0 ? "code-input" : "audio",
              h->n_codes > 0 ? "code_tail" : "audio_tail");
    if (h->pending) {
        const int rcw = vqw_ar_decode_wait(h);
        if (rcw) return rcw;
    }
    hipStream_t st = (hipStream_t)s;
    if (h->persist) {
        const int rc = arp_prefill_finish(h->persist, t_end, audio_tail, code_tail, st);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(ar_prefill_finish_kernel, dim3(1), dim3(256), 0, st, h->st, h->prev, h->xring, h->B, h->w.pre_k, t_end,
                       audio_tail, h->mu);
    VQW_LAUNCH_CHECK("vqw_ar_decode_prefill_finish");
    return 0;
}

extern "C" int vqw_ar_decode_wait(vqw_ar_decoder* h) {
    VQW_CHECK(h, "vqw_ar_decode_wait: null handle");
    if (!h->pending) return 0;
    h->pending = false;
    hipStream_t st = h->run_stream ? h->run_stream : h->stream;
    if (h->persist) {
        const int rc = arp_error(h->persist, st);
        if (rc) return vqw_set_error("vqw_ar_decode_run: persistent kernel %s", rc > 0 ? "timed out waiting for a workgroup" : "failed");
        return 0;
    }
    HIPC(hipStreamSynchronize(st));
    return 0;
}

extern "C" int vqw_ar_decode_run(vqw_ar_decoder* h, const float* encoding, int Tz, int ratio, int n_steps,
                                 int mode, const float* uniforms, float* audio, int32_t* indices,
                                 float* probs_last, vqw_stream_t s) {
    const int rc = vqw_ar_decode_run_async(h, encoding, Tz, ratio, n_steps, mode, uniforms, audio, indices, probs_last, s);
    if (rc) return rc;
    return vqw_ar_decode_wait(h);
}

extern "C" int vqw_ar_decode_workgroups(const vqw_ar_decoder* h) {
    return (h && h->persist) ? arp_workgroups(h->persist) : 0;
}

namespace {

// (re)allocate + compute the per-frame condition projections of one handle for this utterance, on `st`
int project_condition(vqw_ar_decoder* h, const float* encoding, int Tz, hipStream_t st) {
    const vqw_ar_weights& w = h->w;
    const int L = w.n_layers, B = h->B;
    if (Tz > h->cond_Tz_cap) {
        HIPC(hipStreamSynchronize(st));
        if (h->run_stream && h->run_stream != st) HIPC(hipStreamSynchronize(h->run_stream));
        for (int l = 0; l <= L; ++l) {
            if (h->condenc[l]) (void)hipFree(h->condenc[l]);
            const size_t n = (size_t)B * (l < L ? 2 * w.R : w.S) * Tz;
            HIPC(hipMalloc((void**)&h->condenc[l], n * sizeof(float)));
        }
        h->cond_Tz_cap = Tz;
        h->step.drop();   // the captured step carries the condition buffers as kernel arguments
    }
    for (int l = 0; l <= L; ++l) {
        vqw_conv_desc d;
        memset(&d, 0, sizeof(d));
        d.B = B; d.T_in = Tz; d.T_out = Tz; d.C0 = w.Cc; d.ntaps = 1; d.in_stride = 1;
        d.M = (l < L) ? 2 * w.R : w.S;
        d.ldw = (l < L) ? w.cond_ld : w.post1_cond_ld;
        d.epilogue = VQW_EPI_STORE;
        d.x0 = encoding; d.w = (l < L) ? h->cond_w[l] : w.post1_cond_w; d.out0 = h->condenc[l];
        const int rc = vqw_conv_gemm(&d, st);
        if (rc) return rc;
    }
    return 0;
}

}  // namespace

static int run_group(vqw_ar_decoder* const* hs, int n, const float* const* encoding, int Tz, int ratio, int n_steps, int mode,
                     const float* const* uniforms, const vqw_ar_sampling* const* sampling, float* const* audio,
                     int32_t* const* indices, float* const* probs_last, vqw_stream_t s);

// one handle; sampling: NULL (every row at its defaults) or h->B host entries
static int run_single(vqw_ar_decoder* h, const float* encoding, int Tz, int ratio, int n_steps, int mode,
                      const float* uniforms, const vqw_ar_sampling* sampling, float* audio, int32_t* indices,
                      float* probs_last, vqw_stream_t s) {
    if (h && h->persist)
        return run_group(&h, 1, &encoding, Tz, ratio, n_steps, mode, uniforms ? &uniforms : nullptr,
                         sampling ? &sampling : nullptr, &audio, indices ? &indices : nullptr,
                         probs_last ? &probs_last : nullptr, s);
    VQW_CHECK(h && encoding, "vqw_ar_decode_run: null pointer");
    if (h->pending) {
        const int rcw = vqw_ar_decode_wait(h);
        if (rcw) return rcw;
    }
    VQW_CHECK(Tz > 0 && ratio > 0 && n_steps > 0, "vqw_ar_decode_run: bad Tz/ratio/n_steps");
    VQW_CHECK(mode == 0 || (mode == 1 && uniforms), "vqw_ar_decode_run: mode must be 0 (greedy) or 1 (sample, needs uniforms)");
    ArSampleRow rows[MAXB];
    int any = 0;
    {
        const int rc = ar_sampling_rows(sampling, h->B, h->w.Q, mode, rows, &any);
        if (rc) return rc;
    }
    hipStream_t user = (hipStream_t)s;
    hipStream_t st = h->stream;
    h->run_stream = st;
    HIPC(hipEventRecord(h->ev_in, user));
    HIPC(hipStreamWaitEvent(st, h->ev_in, 0));
    {
        const int rc = project_condition(h, encoding, Tz, st);
        if (rc) return rc;
    }
    // run parameters -> device state (step / run_base live on the device)
    ArState hs;
    memset(&hs, 0, sizeof(hs));
    hs.Tz = Tz; hs.ratio = ratio; hs.mode = mode; hs.n_steps = n_steps;
    hs.uniforms = uniforms; hs.audio = audio; hs.indices = indices; hs.probs_last = probs_last;
    for (int b = 0; b < MAXB; ++b) hs.samp[b] = (b < h->B) ? rows[b] : ArSampleRow{1.0f, 0, 1.0f, 0};
    // copy everything except `step`; run_base := step is done by a tiny device-side copy
    HIPC(hipMemcpyAsync(reinterpret_cast<char*>(h->st) + offsetof(ArState, Tz), reinterpret_cast<char*>(&hs) + offsetof(ArState, Tz),
                        sizeof(ArState) - offsetof(ArState, Tz), hipMemcpyHostToDevice, st));
    HIPC(hipMemcpyAsync(&h->st->run_base, &h->st->step, sizeof(int), hipMemcpyDeviceToDevice, st));
    HIPC(hipStreamSynchronize(st));  // `hs` is a stack object; also orders the capture below

    if (h->use_graph && !h->step.exec) {
        const int rc = h->step.capture(st, [&] { return launch_step(h, st); }, "vqw_ar_decode_run");
        if (rc) return rc;
    }
    for (int i = 0; i < n_steps; ++i) {
        if (h->step.exec) {
            HIPC(hipGraphLaunch(h->step.exec, st));
        } else {
            const int rc = launch_step(h, st);
            if (rc) return rc;
        }
    }
    h->pending = true;
    return 0;
}

extern "C" int vqw_ar_decode_run_async(vqw_ar_decoder* h, const float* encoding, int Tz, int ratio, int n_steps,
                                       int mode, const float* uniforms, float* audio, int32_t* indices,
                                       float* probs_last, vqw_stream_t s) {
    return run_single(h, encoding, Tz, ratio, n_steps, mode, uniforms, nullptr, audio, indices, probs_last, s);
}

extern "C" int vqw_ar_decode_run_sampled_async(vqw_ar_decoder* h, const float* encoding, int Tz, int ratio, int n_steps,
                                               int mode, const float* uniforms, const vqw_ar_sampling* sampling, float* audio,
                                               int32_t* indices, float* probs_last, vqw_stream_t s) {
    return run_single(h, encoding, Tz, ratio, n_steps, mode, uniforms, sampling, audio, indices, probs_last, s);
}

extern "C" int vqw_ar_decode_run_group_async(vqw_ar_decoder* const* hs, int n, const float* const* encoding, int Tz,
                                             int ratio, int n_steps, int mode, const float* const* uniforms,
                                             float* const* audio, int32_t* const* indices,
                                             float* const* probs_last, vqw_stream_t s) {
    return run_group(hs, n, encoding, Tz, ratio, n_steps, mode, uniforms, nullptr, audio, indices, probs_last, s);
}

extern "C" int vqw_ar_decode_run_group_sampled_async(vqw_ar_decoder* const* hs, int n, const float* const* encoding, int Tz,
                                                     int ratio, int n_steps, int mode, const float* const* uniforms,
                                                     const vqw_ar_sampling* const* sampling, float* const* audio,
                                                     int32_t* const* indices, float* const* probs_last, vqw_stream_t s) {
    return run_group(hs, n, encoding, Tz, ratio, n_steps, mode, uniforms, sampling, audio, indices, probs_last, s);
}

static int run_group(vqw_ar_decoder* const* hs, int n, const float* const* encoding, int Tz, int ratio, int n_steps, int mode,
                     const float* const* uniforms, const vqw_ar_sampling* const* sampling, float* const* audio,
                     int32_t* const* indices, float* const* probs_last, vqw_stream_t s) {
    VQW_CHECK(hs && encoding && (audio || (hs[0] && hs[0]->n_codes > 0)) && n >= 1 && n <= 8,
              "vqw_ar_decode_run_group: null pointer or n=%d outside 1..8", n);
    VQW_CHECK(Tz > 0 && ratio > 0 && n_steps > 0, "vqw_ar_decode_run: bad Tz/ratio/n_steps");
    VQW_CHECK(mode == 0 || (mode == 1 && uniforms), "vqw_ar_decode_run: mode must be 0 (greedy) or 1 (sample, needs uniforms)");
    for (int i = 0; i < n; ++i) {
        VQW_CHECK(hs[i] && encoding[i] && (hs[i]->n_codes > 0 || audio[i]) && (mode == 0 || uniforms[i]),
                  "vqw_ar_decode_run_group: null pointer (handle %d)", i);
        VQW_CHECK(hs[i]->n_codes == hs[0]->n_codes, "vqw_ar_decode_run_group: handles of one launch must share the input mode");
        VQW_CHECK(hs[i]->persist && arp_same_launch(hs[0]->persist, hs[i]->persist),
                  "vqw_ar_decode_run_group: every handle must run the same persistent kernel (start the others one by one)");
        for (int j = 0; j < i; ++j) VQW_CHECK(hs[j] != hs[i], "vqw_ar_decode_run_group: handle %d given twice", i);
    }
    ArSampleRow rows[8][MAXB];
    const ArSampleRow* rowp[8] = {nullptr};
    for (int i = 0; i < n; ++i) {
        int any = 0;
        const int rc = ar_sampling_rows(sampling ? sampling[i] : nullptr, hs[i]->B, hs[i]->w.Q, mode, rows[i], &any);
        if (rc) return rc;
        if (any) rowp[i] = rows[i];
    }
    for (int i = 0; i < n; ++i) {
        if (hs[i]->pending) {
            const int rcw = vqw_ar_decode_wait(hs[i]);
            if (rcw) return rcw;
        }
    }
    // everything is enqueued on the FIRST handle's stream, ordered after the work already in `s`; the caller's stream is
    // not made to wait (vqw_ar_decode_wait blocks the host instead and reports spin-wait timeouts)
    hipStream_t st = hs[0]->stream;
    HIPC(hipEventRecord(hs[0]->ev_in, (hipStream_t)s));
    HIPC(hipStreamWaitEvent(st, hs[0]->ev_in, 0));
    ArPersist* ps[8];
    const float* const* conds[8];
    for (int i = 0; i < n; ++i) {
        const int rc = project_condition(hs[i], encoding[i], Tz, st);
        if (rc) return rc;
        ps[i] = hs[i]->persist;
        conds[i] = hs[i]->condenc.data();
    }
    const int rc = arp_run(ps, n, conds, Tz, ratio, n_steps, mode, uniforms, audio, indices, probs_last, rowp, st);
    if (rc) return rc;
    for (int i = 0; i < n; ++i) {
        hs[i]->pending = true;
        hs[i]->run_stream = st;
    }
    return 0;
}

extern "C" int vqw_ar_decode_destroy(vqw_ar_decoder* h) {
    if (!h) return 0;
    if (h->pending) (void)vqw_ar_decode_wait(h);   // a group run lives on another handle's stream
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    free_all(h);
    return 0;
}
