"""float64 restatement of tempered / truncated sampling (include/vqwave.h, vqw_ar_sampling), shared by
test_sampling_cpu.py and test_sampling_gpu.py.

For the planted logits of sampling_cases.py (exact ties, no near-ties) there is also a float32 restatement of the KERNEL'S OWN
rule (csrc/ar_sampling.h: value thresholds, ties filled in index order, `above + rank * cut < target` at the nucleus cut):
kept_set_fp32 / restate_fp32, with deliberately wrong evaluations (`wrong=`, WRONG) that test_sampling_planted_cpu.py tells
apart from the right one, and the predicate planted_clean, which takes the place of fp32_edge there: a planted case is
never excused, it has to be clean."""
import numpy as np

WRONG = ('ties_high_index_first', 'topk_keeps_all_ties', 'topk_drops_all_ties', 'topp_keeps_all_ties', 'topp_of_total_mass',
         'topp_before_topk', 'draw_ignores_keep', 'last_is_Q_minus_1', 'lane_tail_dropped')


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


def draws(q, keep, us):
    """draw() for many uniforms at once: the kept classes' cdf values ascend, so the first that reaches u is a searchsorted."""
    ki = np.nonzero(keep)[0]
    pos = np.searchsorted(np.cumsum(q)[ki], np.asarray(us, q.dtype), 'left')
    return ki[np.minimum(pos, len(ki) - 1)]


# ------------------------------------------------------------------ the kernel's rule in float32, and wrong evaluations of it
def _fill(eq, short, high_first):
    """Of the tied classes eq, those whose rank (in index order; from the high end when high_first) passes short(rank)."""
    rank = np.cumsum(eq) - 1
    if high_first:
        rank = int(eq.sum()) - 1 - rank
    return eq & short(rank)


def _top_k32(p, keep, top_k, wrong):
    if not 0 < top_k < int(keep.sum()):
        return keep
    kth = np.sort(p[keep])[::-1][top_k - 1]                  # the K-th largest value: what the bisection over bit patterns finds
    gt, eq = keep & (p > kth), keep & (p == kth)
    if wrong == 'topk_keeps_all_ties':
        return gt | eq
    if wrong == 'topk_drops_all_ties':
        return gt
    need = top_k - int(gt.sum())
    return gt | _fill(eq, lambda rank: rank < need, wrong == 'ties_high_index_first')


def _top_p32(p, keep, top_p, wrong, before):
    f = np.float32
    if not top_p < 1.0:
        return keep
    of = before if wrong == 'topp_of_total_mass' else keep
    target = max(f(top_p) * p[of].sum(dtype=f), f(1.17549435e-38))
    cut = f(0)                                              # the largest value x with M(x) = sum of kept p >= x reaching the target
    for x in np.unique(p[keep])[::-1]:
        if p[keep & (p >= x)].sum(dtype=f) >= target:
            cut = x
            break
    gt, eq = keep & (p > cut), keep & (p == cut)
    if wrong == 'topp_keeps_all_ties':
        return gt | eq
    above = p[gt].sum(dtype=f)
    return gt | _fill(eq, lambda rank: above + rank.astype(f) * cut < target, wrong == 'ties_high_index_first')


def restate_fp32(z, temperature=1.0, top_k=0, top_p=1.0, us=(0.5,), wrong=None):
    """Steps 1-4 as ar_sample_truncated does them, in float32, for every u of us: (p, keep, q, indices).  Sums are numpy's, not
    the kernel's lane order: the planted cases sit 5e-5 from every edge, rounding is 1e-7.  wrong: one of WRONG.  A wrong
    evaluation that keeps nothing returns indices of -1."""
    f = np.float32
    z = np.asarray(z, f)
    Q = len(z)
    valid = np.ones(Q, bool)
    if wrong == 'lane_tail_dropped' and Q % 64:
        valid[64 * (Q // 64):] = False
    us = np.asarray(us, f)
    if not valid.any():
        return np.zeros(Q, f), valid, np.zeros(Q, f), np.full(len(us), -1)
    e = np.where(valid, np.exp((z - z[valid].max()) * (f(1) / f(temperature))), f(0)).astype(f)
    p = e * (f(1) / e.sum(dtype=f))
    k = valid if top_k >= Q else _top_k32(p, valid, top_k, wrong)       # (K >= Q is stored as off)
    if wrong == 'topp_before_topk':
        keep = _top_k32(p, _top_p32(p, valid, top_p, wrong, valid), top_k, wrong)
    else:
        keep = _top_p32(p, k, top_p, wrong, valid)
    if not keep.any():
        return p, keep, np.zeros(Q, f), np.full(len(us), -1)
    q = np.where(keep, p * (f(1) / p[keep].sum(dtype=f)), f(0)).astype(f)
    c = np.cumsum(q, dtype=f)
    hit = c[None, :] >= us[:, None]
    if wrong != 'draw_ignores_keep':
        hit &= keep[None, :]
    last = Q - 1 if wrong == 'last_is_Q_minus_1' else int(np.nonzero(keep)[0][-1])
    return p, keep, q, np.where(hit.any(1), hit.argmax(1), last)


def kept_set_fp32(z, temperature=1.0, top_k=0, top_p=1.0, wrong=None):
    return restate_fp32(z, temperature, top_k, top_p, (), wrong)[1]


# ------------------------------------------------------------------ planted cases: clean, never excused
def planted_faults(z, temperature, top_k, top_p, us, restated=None):
    """Why the float64 restatement of this planted case could differ from an fp32 evaluation of the same rule ([] = clean).
    z are fp32 logits, top_p and us the fp32 values the kernel is given.
      - the levels of z / temperature: equal logits are one level (bit-equal, so equal p in any precision); different levels are
        at least 0.75 apart and at least -40 below the maximum, except at most ONE level at <= -120, whose p is exactly 0 in fp32
        and which is still one tied level in float64.  (This covers every pair of classes around the two cuts.)
      - the renormalised prefix masses of the top-k set stay 5e-5 away from top_p;
      - every u other than 0, 1 and 2 stays 5e-5 away from every cdf value and draws a class with q >= 1e-4.
    u = 0 and u = 2 are decided by the kept mask alone (cdf >= 0 at the first kept class; no cdf value reaches 2).  u = 1 asks
    for the largest kept index, which an fp32 cdf gives only if it cannot reach 1 before that class: its q must be >= 1e-4."""
    z = np.asarray(z)
    why = []
    if z.dtype != np.float32 or not np.isfinite(z).all():
        return ['logits are not finite fp32']
    lv = np.unique(z.astype(np.float64))[::-1] / temperature
    gaps = lv[:-1] - lv[1:]
    if (gaps < 0.75).any():
        why.append('levels closer than 0.75 in z / T')
    low = lv - lv[0] < -40
    if low.sum() > 1 or (lv[low] - lv[0] > -120).any():
        why.append('a level between -40 and -120, or two underflowed levels')
    p, keep, q, _ = restated or restate(z, temperature, top_k, top_p, 0.5)      # (restated: the same, already computed)
    Q = len(z)
    if top_p < 1.0:
        ps = p[order_of(p)][:top_k if 0 < top_k < Q else Q]
        if np.abs(np.cumsum(ps / ps.sum()) - top_p).min() < 5e-5:
            why.append('a prefix mass within 5e-5 of top_p')
    c = np.cumsum(q)
    last = int(np.nonzero(keep)[0][-1])
    for u, i in zip(us, draws(q, keep, us)):
        if u in (0.0, 2.0):
            continue
        if u == 1.0:
            if q[last] < 1e-4:
                why.append('u = 1 with q < 1e-4 at the largest kept index')
        elif np.abs(c - u).min() < 5e-5 or q[i] < 1e-4:
            why.append('u = %r within 5e-5 of a cdf value, or its class has q < 1e-4' % float(u))
    return why


def planted_clean(z, temperature, top_k, top_p, us):
    return not planted_faults(z, temperature, top_k, top_p, us)
