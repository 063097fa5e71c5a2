// Internal interface of the persistent fast-generation kernel (csrc/ar_persist.hip).
#pragma once
#include "ar_sampling.h"
#include "mu_law.h"
#include "vqw_common.h"

struct ArPersist;
bool arp_supported(const vqw_ar_weights* w, int batch);
int arp_create(ArPersist** out, const vqw_ar_weights* w, const int* dil, const float* const* gated_w,
               const float* const* gated_b, const float* const* out_w, const float* const* out_b, int batch,
               int channels_per_workgroup,    // 0 = auto (4 where the chip has R/4 CUs), 4 or 8
               int n_codes);                  // > 0: code-input mode (w->pre_w is [pre_k][n_codes][R]); 0: audio
int arp_reset(ArPersist* h, hipStream_t st);
void arp_set_levels(ArPersist* h, const VqwMu& m);   // audio handles: the mu-law level of the decode / re-encode table (256 after create)
// ONE launch for n handles (1..8, the same kernel instantiation, n * workgroups <= CUs) generating side by side.
// condenc[i]: L+1 device pointers of handle i ([B][2R][Tz] per layer, then [B][S][Tz] of postprocess1)
int arp_run(ArPersist* const* hs, int n, const float* const* const* condenc, int Tz, int ratio, int n_steps, int mode,
            const float* const* uniforms, float* const* audio /* may be NULL */, int32_t* const* indices, float* const* probs_last,
            const ArSampleRow* const* samp /* NULL, or per handle B rows (ar_sampling_rows) */, hipStream_t st);
// prefill after arp_reset (vqw_ar_decode_prefill_layer / _finish): layer l's ring slots t_lo .. t_end-1 from x [B][R][ld]
// (column tau - t_first); then the input history, the last sample and the step counter
int arp_prefill_layer(ArPersist* h, int l, const float* x, int ld, int t_first, int t_lo, int t_end, hipStream_t st);
int arp_prefill_finish(ArPersist* h, int t_end, const float* audio_tail, const int32_t* code_tail, hipStream_t st);
int arp_workgroups(const ArPersist* h);
bool arp_same_launch(const ArPersist* x, const ArPersist* y);
int arp_error(ArPersist* h, hipStream_t st);   // 0 ok, 1 a spin-wait timed out, -1 HIP error
void arp_destroy(ArPersist* h);
