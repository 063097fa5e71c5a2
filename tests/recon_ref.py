"""float64 restatement of teacher-forced sampling over a whole logits tensor (include/vqwave.h, vqw_softmax_sample), built on
sampling_ref.restate / fp32_edge; shared by test_recon_cpu.py and test_recon_gpu.py.

    sample_ref(z [B][Q][T], u [B][T], settings, t_begin, t_end, mode) -> dict
        idx    int64   [B][T]      the class of every position in the range, -1 outside
        probs  float64 [B][T][Q]   the distribution drawn from (softmax(z) in greedy mode), 0 outside
        edge   bool    [B][T]      the restated decision sits on an fp32 edge (sampling_ref.fp32_edge); False outside / greedy
        last   int64   [B][T]      the largest kept index, -1 outside
        mask   bool    [B][T]      the position is in its row's range

settings: None (every row at its defaults) or one (temperature, top_k, top_p) per row.  Greedy is np.argmax: the lowest index
among the maxima."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampling_ref as SR  # noqa: E402

DEFAULTS = (1.0, 0, 1.0)


def range_mask(B, T, t_begin=None, t_end=None):
    t = np.arange(T)[None, :]
    lo = np.zeros(B, np.int64) if t_begin is None else np.maximum(np.asarray(t_begin, np.int64), 0)
    hi = np.full(B, T, np.int64) if t_end is None else np.minimum(np.asarray(t_end, np.int64), T)
    return (t >= lo[:, None]) & (t < hi[:, None])


def sample_ref(z, u=None, settings=None, t_begin=None, t_end=None, mode='sample'):
    z = np.asarray(z)
    B, Q, T = z.shape
    mask = range_mask(B, T, t_begin, t_end)
    idx = np.full((B, T), -1, np.int64)
    last = np.full((B, T), -1, np.int64)
    probs = np.zeros((B, T, Q), np.float64)
    edge = np.zeros((B, T), bool)
    for b in range(B):
        temperature, top_k, top_p = DEFAULTS if settings is None else settings[b]
        for t in np.nonzero(mask[b])[0]:
            col = z[b, :, t].astype(np.float64)
            if mode == 'greedy':
                idx[b, t] = int(np.argmax(z[b, :, t]))
                probs[b, t] = SR.softmax_t(col, 1.0)
                continue
            p, keep, q, i = SR.restate(col, temperature, top_k, top_p, float(u[b, t]))
            idx[b, t], probs[b, t], last[b, t] = i, q, int(np.nonzero(keep)[0][-1])
            edge[b, t] = SR.fp32_edge(p, keep, q, top_k, top_p, float(u[b, t]))
    return {'idx': idx, 'probs': probs, 'edge': edge, 'last': last, 'mask': mask}
