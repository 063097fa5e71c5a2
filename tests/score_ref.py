"""numpy restatement of the held-out scores (include/vqwave.h: vqw_softmax_score, vqw_code_histogram), float64 by default.

    nll[b][t]     = logsumexp_q z[b][q][t] - z[b][label][t]                    nats
    entropy[b][t] = logsumexp_q z - sum_q softmax(z)_q z_q                     nats
    position (b, t) is scored iff t_begin[b] <= t < t_end[b]; unscored positions read 0
    per row: sums of nll and entropy, the number of scored positions, hits
    hit: the label is the LOWEST index among the maxima of the position's logits

`dtype=np.float32` evaluates the same formulas in single precision (every intermediate is float32): the model of what a
float32 implementation may lose, which the GPU tests measure against the float64 evaluation.
"""
import numpy as np


def score_ref(logits, labels, t_begin=None, t_end=None, dtype=np.float64):
    z = np.asarray(logits).astype(dtype)
    B, Q, T = z.shape
    labels = np.asarray(labels).astype(np.int64).reshape(B, T)
    tb = np.zeros(B, np.int64) if t_begin is None else np.asarray(t_begin, np.int64)
    te = np.full(B, T, np.int64) if t_end is None else np.asarray(t_end, np.int64)
    t = np.arange(T)[None, :]
    mask = (t >= tb[:, None]) & (t < te[:, None])
    m = z.max(axis=1)                                       # [B][T]
    d = z - m[:, None, :]
    e = np.exp(d)
    s = e.sum(axis=1)
    log_s = np.log(s)
    zl = np.take_along_axis(z, labels[:, None, :], axis=1)[:, 0, :]
    nll = (log_s + m) - zl
    # sum_q p_q z_q = m + sum_q e_q d_q / s  (e_q d_q -> 0 where e_q underflows)
    ed = np.where(e > 0, e * np.where(e > 0, d, 0), 0).astype(dtype)
    entropy = log_s - ed.sum(axis=1) / s
    arg = z.argmax(axis=1)                                  # numpy: the first (lowest) index among the maxima
    hit = (arg == labels) & mask
    nll = np.where(mask, nll, 0).astype(dtype)
    entropy = np.where(mask, entropy, 0).astype(dtype)
    return {'nll': nll, 'entropy': entropy, 'mask': mask,
            'nll_sum': nll.astype(np.float64).sum(axis=1), 'entropy_sum': entropy.astype(np.float64).sum(axis=1),
            'count': mask.sum(axis=1).astype(np.int64), 'hits': hit.sum(axis=1).astype(np.int64)}


def histogram_ref(idx, K, f_end=None):
    """counts[c] = occurrences of c in idx [B][Tz] over frames f < f_end[b]; indices outside [0, K) are counted nowhere.
    Returns (counts int64 [K], whether any index was outside)."""
    idx = np.asarray(idx, np.int64)
    B, Tz = idx.shape
    fe = np.full(B, Tz, np.int64) if f_end is None else np.asarray(f_end, np.int64)
    valid = np.arange(Tz)[None, :] < fe[:, None]
    v = idx[valid]
    inside = (v >= 0) & (v < K)
    return np.bincount(v[inside], minlength=K).astype(np.int64), bool((~inside).any())
