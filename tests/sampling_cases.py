"""Planted logits for truncated sampling (csrc/ar_sampling.h): staircases whose every top-k / top-p / draw decision is exact, so
that the tie fill, the `above + rank * cut < target` arithmetic, the ballot prefix counts and the empty / partial lanes are
held to the float64 restatement of sampling_ref.py with NO excuse.  Shared by test_sampling_planted_cpu.py (which proves
the cases clean and able to tell wrong evaluations apart) and test_sampling_planted_gpu.py.

A Staircase is Q classes on 2 to 5 levels of logits; the classes of one level are exact ties.  Its canonical order is level
by level; `logits(st, shuffle)` scatters the levels over the classes (and so over the lanes) by a seeded permutation.
  - the levels are LEVELS + an offset: multiples of 0.25, exact in fp32; neighbours at least 1.5 apart and the lowest 7.5
    below the top, so that at every temperature of TEMPERATURES they are >= 0.75 apart and >= -15 in z / T;
  - at most one more level at UNDER = -256 below the top: z / T <= -128, p exactly 0 in fp32 (exp(-128) = 2.6e-56 is below
    the smallest denormal), still one tied level of tiny positive p in float64.  Top-k above the count of non-zero classes then
    runs the kernel's `ans == 0` path.
Three staircases per Q: 0 has a single top class and no underflowed level, 1 and 2 have a plateau on top and an underflowed
level; Q = 4 has its own three.

settings(st): the rows (temperature, top_k, top_p) of a staircase.  They depend on the level counts alone, not on the shuffle:
  top_k   0, 1, cuts in the middle of a plateau and one short of its end, the cut at that plateau's end, and (underflowed
          level) a cut inside that level;
  top_p   1, or the fp32 midpoint between the renormalised prefix masses of n - 1 and n classes of the top-k set, for n = 1,
          n inside a plateau (the highest and the lowest eligible one) and n = the last class of renormalised mass >= 1e-4.
draw_list(...): u = 0, u = 2, u = 1 where it is decidable (sampling_ref.planted_faults) and the midpoint of the cdf
interval of every kept class with q >= 1e-4.

plant(st, rows, T): a logits tensor [B][Q][T] for the all-positions kernel, row b under rows[b], position t with its own
shuffle and its own u from that position's draw list, and the float64 restatement of every position."""
import collections
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampling_ref as S  # noqa: E402

QS = (4, 60, 64, 68, 100, 256, 512, 1020, 1024)      # of the all-positions kernel
CODE_QS = (32, 96)                                     # code counts of the prior generators (the audio ones: 256, 1024)
TEMPERATURES = (0.5, 1.0, 2.0)
LEVELS = (0.0, -1.5, -3.0, -5.0, -7.5)
UNDER = -256.0
OFFSETS = (2.5, -1.25, 0.0)
N_STAIRCASES = 3
Q4 = (((1, 3), False), ((2, 2), True), ((1, 2, 1), False))       # (counts, the last level underflows)

Staircase = collections.namedtuple('Staircase', 'Q index counts values under')


@functools.lru_cache(maxsize=None)
def staircase(Q, index):
    """Staircase `index` (0 .. N_STAIRCASES - 1) of Q classes."""
    if Q == 4:
        counts, under = Q4[index]
    else:
        n_levels, under = ((3, False), (3, True), (5, True))[index]
        g = np.random.RandomState(1000 * Q + index)
        while True:
            cuts = np.sort(g.choice(np.arange(1, Q), n_levels - 1, replace=False))
            if index == 0:
                cuts[0] = 1                                  # a single class on top
            counts = tuple(int(c) for c in np.diff(np.concatenate([[0], cuts, [Q]])))
            body = counts[:-1]
            # a plateau of >= 3 classes that is not the last level; >= 2 on top (but for staircase 0) and on an underflowed level
            if min(counts) >= 1 and max(body) >= 3 and (index == 0 or counts[0] >= 2) and (not under or counts[-1] >= 2):
                break
    values = [LEVELS[i] + OFFSETS[index] for i in range(len(counts) - under)] + ([UNDER + OFFSETS[index]] if under else [])
    return Staircase(Q, index, counts, tuple(values), under)


def canonical(st):
    """The logits level by level, fp32 [Q]."""
    return np.repeat(np.asarray(st.values, np.float32), st.counts)


def permutation(st, shuffle):
    return np.random.RandomState((st.Q * 8 + st.index) * 4096 + shuffle).permutation(st.Q)


def logits(st, shuffle=0):
    z = np.empty(st.Q, np.float32)
    z[permutation(st, shuffle)] = canonical(st)
    return z


def plateau(st):
    """(classes above it, its count) of the plateau the top-k cuts use: the largest level that is neither the last nor the
    underflowed one (Q = 4, counts (1, 3): the last after all; the cut at its end is then K = Q, which is top-k off)."""
    cand = [j for j in range(len(st.counts) - 1) if st.counts[j] >= 2] or [len(st.counts) - 1]
    j = max(cand, key=lambda j: (st.counts[j], j))
    return sum(st.counts[:j]), st.counts[j]


def top_ks(st):
    above, count = plateau(st)
    ks = [0, 1, above + max(1, count // 2), above + count - 1, above + count]     # two cuts inside the plateau, one at its end
    if st.under:
        ks.append(st.Q - st.counts[-1] + max(1, st.counts[-1] // 2))      # above the count of non-zero classes
    return sorted(set(ks))


def top_ps(st, temperature, top_k):
    p = S.softmax_t(canonical(st).astype(np.float64), temperature)     # descending; ties in index order
    nk = top_k if 0 < top_k < st.Q else st.Q
    ps = p[:nk] / p[:nk].sum()
    c = np.concatenate([[0.0], np.cumsum(ps)])
    level = np.repeat(np.arange(len(st.counts)), st.counts)[:nk]
    heavy = int((ps >= 1e-4).sum())
    ns = {1, heavy}
    inside = [n for n in range(1, min(heavy, nk - 1) + 1) if level[n - 1] == level[n]]       # classes n and n + 1 are tied
    for lv in {level[n] for n in inside[:1] + inside[-1:]}:
        of = [n for n in inside if level[n] == lv]
        ns.add(of[len(of) // 2])
    return [1.0] + sorted({float(np.float32((c[n - 1] + c[n]) / 2)) for n in ns})


@functools.lru_cache(maxsize=None)
def settings(st):
    return tuple((t, k, p) for t in TEMPERATURES for k in top_ks(st) for p in top_ps(st, t, k))


def draw_list(q, keep):
    """The uniforms of a restated (q, keep), fp32: 0, 2, 1 where the largest kept class has q >= 1e-4, then the midpoint of the
    cdf interval of every kept class with q >= 1e-4 in index order."""
    c = np.cumsum(q)
    target = np.nonzero(keep & (q >= 1e-4))[0]
    special = [0.0, 2.0] + ([1.0] if q[np.nonzero(keep)[0][-1]] >= 1e-4 else [])
    return np.concatenate([special, c[target] - q[target] / 2]).astype(np.float32)


def pick(us, t, T):
    """Position t of T takes the specials first, then the midpoints spread evenly over the list."""
    n_special = 3 if us[2] == 1.0 else 2
    if t < n_special:
        return us[t]
    mid = us[n_special:]
    return mid[(t - n_special) * len(mid) // (T - n_special)]


Planted = collections.namedtuple('Planted', 'z u rows idx keep q faults')


def plant(st, rows, T):
    """z fp32 [B][Q][T], u fp32 [B][T] and the float64 restatement idx [B][T], keep [B][T][Q], q [B][T][Q] of rows
    [(temperature, top_k, top_p)]; position t has shuffle t.  faults: what sampling_ref.planted_faults finds (must be [])."""
    B, Q = len(rows), st.Q
    z = np.empty((B, Q, T), np.float32)
    u = np.empty((B, T), np.float32)
    idx = np.empty((B, T), np.int64)
    keep = np.empty((B, T, Q), bool)
    q = np.empty((B, T, Q), np.float64)
    faults = []
    for t in range(T):
        zt = logits(st, t)
        z[:, :, t] = zt
        for b, (temperature, top_k, top_p) in enumerate(rows):
            r = S.restate(zt, temperature, top_k, top_p)
            _, keep[b, t], q[b, t], _ = r
            u[b, t] = pick(draw_list(q[b, t], keep[b, t]), t, T)
            idx[b, t] = S.draw(q[b, t], keep[b, t], float(u[b, t]))
            faults += ['Q %d staircase %d row %s position %d: %s' % (Q, st.index, rows[b], t, w)
                       for w in S.planted_faults(zt, temperature, top_k, top_p, u[b, t:t + 1], restated=r)]
    return Planted(z, u, list(rows), idx, keep, q, faults)


def steps(st, row, n, shuffle=0):
    """For the generators, whose logits are the same staircase at every step: n uniforms of the row's draw list (all of it, in
    order, when it is no longer than n; else the specials and an even spread of the midpoints) and the restated indices."""
    zt = logits(st, shuffle)
    p, keep, q, _ = S.restate(zt, *row)
    us = draw_list(q, keep)
    u = np.array([pick(us, t, n) for t in range(n)], np.float32) if len(us) > n else np.resize(us, n)
    return u, S.draws(q, keep, u.astype(np.float64)), keep, q
