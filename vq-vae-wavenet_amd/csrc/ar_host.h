// Host code the handles of the launch-per-phase generator (ar_decode.hip) and of the wide generator (ar_wide.hip) share:
// the copy of the caller's weight tables, the captured step graph, the checks of *_set_levels.  Plain host C++, no kernels.
#pragma once
#include <vector>

#include "mu_law.h"
#include "vqw_common.h"

#define HIPC(x)                                                                       \
    do {                                                                              \
        hipError_t e_ = (x);                                                          \
        if (e_ != hipSuccess) return vqw_set_error("%s failed: %s", #x, hipGetErrorString(e_)); \
    } while (0)

// A handle's own copy of vqw_ar_weights: the caller's per-layer tables need not outlive the create call.
struct ArTables {
    vqw_ar_weights w;               // its six table pointers are null: read the vectors
    std::vector<int> dil;
    std::vector<const float*> gated_w, gated_b, cond_w, out_w, out_b;

    void assign(const vqw_ar_weights* src) {
        w = *src;
        const int L = w.n_layers;
        dil.assign(w.dilations, w.dilations + L);
        gated_w.assign(w.gated_w, w.gated_w + L);
        gated_b.assign(w.gated_b, w.gated_b + L);
        cond_w.assign(w.cond_w, w.cond_w + L);
        out_w.assign(w.out_w, w.out_w + L);
        out_b.assign(w.out_b, w.out_b + L);
        w.dilations = nullptr; w.gated_w = nullptr; w.gated_b = nullptr; w.cond_w = nullptr;
        w.out_w = nullptr; w.out_b = nullptr;
    }
    // floats of layer l's ring for B rows: (ks-1) d slots of [B][R]
    size_t ring_floats(int l, int B) const { return (size_t)(w.kernel_size - 1) * dil[l] * B * w.R; }
};

// One step of a handle, captured once and replayed per sample.
struct ArGraph {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;

    void drop() {                   // the next run captures again
        if (exec) { (void)hipGraphExecDestroy(exec); exec = nullptr; }
        if (graph) { (void)hipGraphDestroy(graph); graph = nullptr; }
    }
    // capture what step_fn() enqueues on st (a private stream: capture is illegal on the null stream) and instantiate it
    template <class F>
    int capture(hipStream_t st, F step_fn, const char* what) {
        HIPC(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
        const int rc = step_fn();
        hipGraph_t g = nullptr;
        hipError_t e = hipStreamEndCapture(st, &g);
        if (rc) return rc;
        if (e != hipSuccess) return vqw_set_error("%s: graph capture failed: %s", what, hipGetErrorString(e));
        graph = g;
        HIPC(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
        return 0;
    }
};

// The refusals of <family>_set_levels (family: vqw_ar_decode / vqw_ar_wide), in their order and before any device call;
// *m is the level's constants.  H: a handle with n_codes, w.Q and pending.
template <class H>
int ar_levels_check(const char* family, const H* h, int levels, VqwMu* m) {
    VQW_CHECK(vqw_mu_level(levels, m), "%s_set_levels: levels=%d must be 256, 512 or 1024", family, levels);
    VQW_CHECK(h, "%s_set_levels: null handle", family);
    VQW_CHECK(h->n_codes == 0, "%s_set_levels: a code-input handle (n_codes=%d) has no mu-law", family, h->n_codes);
    VQW_CHECK(levels == h->w.Q, "%s_set_levels: levels=%d is not the handle's Q=%d", family, levels, (int)h->w.Q);
    VQW_CHECK(!h->pending, "%s_set_levels: levels=%d refused while a run is pending (%s_wait first)", family, levels, family);
    return 0;
}
