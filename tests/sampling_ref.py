"""float64 restatement of tempered / truncated sampling (include/vqwave.h, vqw_ar_sampling), shared by
test_sampling_cpu.py and test_sampling_gpu.py."""
import numpy as np


def softmax_t(z, temperature):
    z = np.asarray(z, np.float64)
    e = np.exp((z - z.max()) / temperature)
    return e / e.sum()


def order_of(p):
    """Classes by (p descending, index ascending)."""
    return np.lexsort((np.arange(len(p)), -np.asarray(p)))


def kept_set(p, top_k=0, top_p=1.0):
    """Boolean mask of the classes kept by top-k, then top-p over the renormalised kept set (steps 2-3)."""
    p = np.asarray(p, np.float64)
    Q = len(p)
    sel = order_of(p)
    if 0 < top_k < Q:
        sel = sel[:top_k]
    if top_p < 1.0:
        c = np.cumsum(p[sel] / p[sel].sum())
        n = int(np.searchsorted(c, top_p, 'left')) + 1      # the shortest prefix whose mass is >= top_p
        sel = sel[:min(n, len(sel))]
    keep = np.zeros(Q, bool)
    keep[sel] = True
    return keep


def draw(q, keep, u):
    """Step 4: the first kept index whose ascending cdf of q reaches u, else the largest kept index."""
    c = np.cumsum(q)
    hit = np.nonzero(keep & (c >= u))[0]
    return int(hit[0]) if len(hit) else int(np.nonzero(keep)[0][-1])


def restate(z, temperature=1.0, top_k=0, top_p=1.0, u=0.5):
    """Steps 1-4 on logits z: (p, keep, q, index)."""
    p = softmax_t(z, temperature)
    keep = kept_set(p, top_k, top_p)
    q = np.where(keep, p, 0.0)
    q = q / q.sum()
    return p, keep, q, draw(q, keep, u)


def fp32_edge(p, keep, q, top_k, top_p, u, tol_u=2e-6, tol_p=1e-5, tol_tie=1e-7):
    """True when the restated decision sits on an fp32 edge: u within tol_u of a cdf value, the top-p mass of a prefix
    within tol_p of P, or a p-tie within tol_tie at the top-k / top-p cut."""
    if np.abs(np.cumsum(q) - u).min() < tol_u:
        return True
    srt = order_of(p)
    ps = p[srt]
    n_k = len(p) if not 0 < top_k < len(p) else top_k
    if n_k < len(p) and abs(ps[n_k - 1] - ps[n_k]) < tol_tie:
        return True
    if top_p < 1.0:
        c = np.cumsum(ps[:n_k] / ps[:n_k].sum())
        if np.abs(c - top_p).min() < tol_p:
            return True
        n = int(keep.sum())
        if n < n_k and abs(ps[n - 1] - ps[n]) < tol_tie:
            return True
    return False
