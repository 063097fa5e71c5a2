"""Plane-exact float64 reference of the stride-1 weight gradients of the fp16x3 engine -- vqw_f16x3_wgrad / vqw_f16x3_wgrad_batch
with p_stride 1, in all four operand forms, fp16x3 and VQW_X3_BF16 --, their seeded case tables, the launcher's path and refusal
rules restated, and their bars, for tests/test_x3_wgrad_ref_cpu.py and tests/test_x3_wgrad_kernels_gpu.py.  (The stride-2 forms
are held by tests/sconv_ref.py.)

numpy only, float64, written from the sentences of include/vqwave.h ("Weight gradient of conv1d_v2") and not from the kernels'
index arithmetic.  The number format comes from tests/x3_ref.py: an operand is scaled by its power of two (scaled), split into
two fp16 planes (split) or rounded to its one bf16 plane (bf16_round), a product is a1 b1 + a1 b2 + a2 b1 (one product under bf16)
summed in float64 and divided by the scales, the host-side factors p_planes_scale / q_planes_scale included.  What is left to
the device is its fp32 accumulation, the descale of each partial tile, the adds of the reduce kernel and the add onto dw.

Bars, elementwise, U = 2^-24.  abs_sum is the sum of the absolute values of the addends of one dw element in the units of the
unscaled result, `terms` = 3 (fp16x3) or 1 (bf16) products per step of the contraction:

    e_acc       = terms * B * T * U * abs_sum      a recursive fp32 sum of n terms in ANY order errs by at most (n - 1) U sum|.|;
                                                   n, not n - 1, for the reason given in tests/pointwise_ref.py.  Steps that read
                                                   padding are counted: they add exact zeros.
    P           = |dw - dw0| + e_acc               the magnitude of a partial tile and of the update
    bar         = e_acc                            the accumulators
                + U * P                            the descale of every partial tile (one product each, by 1 / (scales); with
                                                   powers of two it is exact, and the term is kept for scales that are not)
                + nsplit * U * P                   the adds of the reduce kernel: one per partial tile, each partial sum at most P
                + 2 U * (P + |dw0|)                the add onto the value dw held
    q_total     : (B * T + 3) * U * (sum |q| + |total0|)         as sconv_ref.wgrad_s2: an any-order sum of B * T values that may
    q_seg       : (T / seg_T + 3) * U * sum |q|                  each have been formed by one fp32 add of two planes and one
                                                                 product with 1 / scale, atomics onto the value held before
                                                                 (q_seg is zeroed by the caller)

No constant was moved against the sequential fp32 emulations of tests/test_x3_wgrad_ref_cpu.py (time-major, and cut into nsplit
partial sums that are descaled and then added): the only term that a single rounding can fill, the add onto dw0, was taken as
2 U from the start, for the reason tests/sconv_ref.py gives where that constant did move (one rounding attains U |result| just
above a power of two, and a bar cannot leave a quarter of itself free for less than 4/3 roundings).  e_acc grows with
n * abs_sum ~ n^2 while the rounding error of n random terms grows with sqrt(n): measured errors are small fractions of these
bars at large B * T, and the shapes are kept small for that reason too -- at B * T = 32 a missing h2 h1 term is several bars.

Two kinds of operands per case (as tests/sconv_ref.py):
 'ints'    integers |v| <= 4 in p and q, integer dw0 / total0, power-of-two scales: every low plane is zero, the bf16 plane is
           exact and every partial sum in every order is exact in fp32 -- the device must equal the reference bit for bit, in
           dw, q_total and q_seg.
 'normal'  p standard normal under 2^9, q of order 1e-5 under 2^27 (q1: 3e-5 under 2^26), dw0 and total0 of order 1e-4.

Deliberately wrong evaluations (`wrong=` of wgrad(), WRONG below) are told apart from the right one by
tests/test_x3_wgrad_ref_cpu.py, and swapped in for it on the device once."""
import numpy as np

import sconv_ref as S
import x3_ref as X

U, EMU_FRACTION, GUARD, SENTINEL, F32 = S.U, S.EMU_FRACTION, S.GUARD, S.SENTINEL, S.F32
seed_of, ints = S.seed_of, S.ints
KINDS = ('ints', 'normal')
MAX_TAPS, MAX_BATCH, TILE = 8, 32, 256
TILE_FLOATS = TILE * TILE
SP, SQ0, SQ1 = 2.0 ** 9, 2.0 ** 27, 2.0 ** 26         # guard scales of the 'normal' kind (tests/wgrad_dma_cases.py)

WRONG = ('shift_plus_one', 'drop_last_tap', 'drop_last_pair', 'drop_last_split', 'leak_before_t0', 'ragged_tail_read',
         'window_not_moved', 'no_h2h1', 'dw_overwritten', 'q1_scale_from_q0', 'row_tile_reads_first', 'no_relu',
         'relu_after_split', 'total_all_cols', 'seg_from_rounded', 'p_kc0_ignored', 'p_tap_chunk_ignored', 'q_hscale_ignored')


# ---------------------------------------------------------------------------------------------------- the reference
def pieces(x, s, bf16):
    """The values the planes of s * x hold, as float64: (h1, h2), or (bf16(s x), 0)."""
    if bf16:
        r = X.bf16_round(X.scaled(x, s))
        return r, np.zeros_like(r)
    return X.planes_of(x, s)


def pairs(B, T):
    """(pairs per batch row, pairs in all): the contraction runs in pairs of 16-step stages, 32 steps of one batch row."""
    return -(-T // 32), B * -(-T // 32)


def split_range(B, T, nsplit, k):
    """The pairs [begin, end) of partial sum k of nsplit: contiguous, even cuts of the flat (batch row, pair) axis."""
    pt = pairs(B, T)[1]
    return k * pt // nsplit, (k + 1) * pt // nsplit


def step_mask(B, T, lo, hi):
    """[B][T] bool: the steps of the pairs [lo, hi)."""
    pr = pairs(B, T)[0]
    pair = np.arange(B)[:, None] * pr + np.arange(T)[None, :] // 32
    return (pair >= lo) & (pair < hi)


def _read(h, idx, leak):
    """h [B][C][T] read at idx of every batch row, zero outside [0, T).  leak: before t = 0 the flat (batch, time) rows are read
    instead -- the previous batch row's end (nothing lies before batch 0)."""
    if not leak:
        return X.gather(h, idx)
    B, C, T = h.shape
    flat = h.transpose(1, 0, 2).reshape(C, B * T)
    f = (np.arange(B) * T)[:, None] + idx[None, :]
    ok = (f >= 0) & (idx[None, :] < T)
    return (flat[:, np.clip(f, 0, B * T - 1)] * ok).transpose(1, 0, 2)


def wgrad(p, q0, q1, taps, sp=1.0, sq0=1.0, sq1=1.0, *, Cp=None, Q0=None, mode=0, p_planes=False, q_planes=False, p_hscale=1.0,
          q_hscale=1.0, p_kc0=0, p_tap_chunk=None, q_kc0=0, p_relu=False, dw0=None, total=False, total0=None, total_cols=None,
          seg_T=0, nsplit=1, csel=None, osel=None, wrong=None, full=False):
    """dw[j][c][o] = dw0 + sum_{b,t} p[b][c][t + taps[j]] q[b][o][t], zero outside [0, T) of the batch row; q = [q0; q1] along o, each
    with its own scale.  p [B][>= Cp][T]: with p_planes the channels of a wider planes tensor, tap j reading the Cp channels from chunk
    p_kc0 + p_tap_chunk[j] (8 channels per chunk); q0 likewise with q_planes, Q0 channels from chunk q_kc0.  p_hscale / q_hscale:
    the host-side factors of the planes' scales.  p_relu: max(p, 0) before the split.  q_total (with `total`) = total0 + sum_{b,t} q
    over the columns total_cols, q_seg[b][o][f] (with seg_T) = sum of q over frame f of T / seg_T steps: of q as it arrives -- the
    fp32 values, or what the planes hold over their scale.  csel / osel: only these rows / columns of dw (and sums) are evaluated.
    nsplit enters the bar, and the deliberately wrong evaluation that drops the last partial sum.
    Returns (dw, q_total, q_seg), with full (dw, q_total, q_seg, bar_dw, bar_total, bar_seg, abs_sum); sums not asked for are None."""
    p = np.asarray(p, F32)
    B, _, T = p.shape
    Cp = p.shape[1] if Cp is None else Cp
    Q0 = q0.shape[1] if Q0 is None else Q0
    Q1 = 0 if q1 is None else q1.shape[1]
    bf = bool(mode & X.X3_BF16)
    ntaps = len(taps)
    csel = np.arange(Cp) if csel is None else np.asarray(csel)
    osel = np.arange(Q0 + Q1) if osel is None else np.asarray(osel)
    chunk = list(p_tap_chunk) if p_tap_chunk is not None else [0] * ntaps
    if wrong == 'p_tap_chunk_ignored':
        chunk = [0] * ntaps
    kc0 = 0 if wrong == 'p_kc0_ignored' else p_kc0
    ph = float(F32(p_hscale)) if p_planes else 1.0
    qh = float(F32(q_hscale)) if q_planes else 1.0
    # ---- q: the pieces of each half at its own scale, and the scale each column is divided by
    qa = np.asarray(q0, F32)[:, 8 * q_kc0:8 * q_kc0 + Q0]
    h = [pieces(qa, sq0 * qh, bf)]
    col_scale = np.full(Q0 + Q1, float(F32(sq0)) * (1.0 if wrong == 'q_hscale_ignored' else qh))
    if Q1:
        h.append(pieces(q1, sq1, bf))
        col_scale[Q0:] = float(F32(sq0 if wrong == 'q1_scale_from_q0' else sq1))
    b1, b2 = (np.concatenate([x[i] for x in h], axis=1)[:, osel] for i in (0, 1))
    keep = np.ones((B, T), bool)
    pr = pairs(B, T)[0]
    if wrong == 'drop_last_pair':
        keep &= np.arange(T)[None, :] < 32 * (pr - 1)
    if wrong == 'drop_last_split' and nsplit > 1:
        keep &= ~step_mask(B, T, *split_range(B, T, nsplit, nsplit - 1))
    b1, b2 = b1 * keep[:, None, :], b2 * keep[:, None, :]
    qf = lambda x: x.transpose(1, 0, 2).reshape(len(osel), B * T)  # noqa: E731
    B1, B2 = qf(b1), qf(b2)
    # ---- p: relu, pieces, and per tap the rows it reads
    pin = np.maximum(p, F32(0)) if p_relu and wrong not in ('no_relu', 'relu_after_split') else p
    a_all = pieces(pin, sp * ph, bf)
    if p_relu and wrong == 'relu_after_split':
        a_all = tuple(np.maximum(x, 0.0) for x in a_all)
    t = np.arange(T)
    inv = 1.0 / (float(F32(sp)) * ph * col_scale[osel])[None, :]
    dw, ab = [], []
    for j, sh in enumerate(taps):
        sh = sh + (wrong == 'shift_plus_one')
        c0 = 8 * (kc0 + chunk[j])
        rows = c0 + (csel % TILE if wrong == 'row_tile_reads_first' else csel)
        idx = t + sh
        g = [_read(x[:, rows], idx, wrong == 'leak_before_t0') for x in a_all]
        if wrong == 'window_not_moved' and sh < 0 and (sh & 3):
            live = ~((idx >= 0) & (idx < 4 - ((-sh) & 3)))         # the window that straddles t = 0 read as zero throughout
            g = [x * live for x in g]
        a1, a2 = (x.transpose(1, 0, 2).reshape(len(csel), B * T) for x in g)
        v = a1 @ (B1 + B2).T
        s = np.abs(a1) @ (np.abs(B1) + np.abs(B2)).T
        if wrong != 'no_h2h1':
            v, s = v + a2 @ B1.T, s + np.abs(a2) @ np.abs(B1).T
        if wrong == 'ragged_tail_read' and T % 32:
            # the steps behind the row's end are the next batch row's first steps on the planes' flat (batch, time) row axis
            k = np.arange(32 * pr - T)
            for b in range(B - 1):
                f = (b + 1) * T + k + sh
                ok = (T + k + sh >= 0) & (f >= 0) & (f < B * T)
                fl = [x[:, rows].transpose(1, 0, 2).reshape(len(csel), B * T)[:, np.clip(f, 0, B * T - 1)] * ok for x in a_all]
                v = v + fl[0] @ (b1[b + 1][:, k] + b2[b + 1][:, k]).T + fl[1] @ b1[b + 1][:, k].T
        if wrong == 'drop_last_tap' and j == ntaps - 1 and ntaps > 1:
            v = v * 0.0
        dw.append(v * inv)
        ab.append(s * inv)
    dw, ab = np.stack(dw), np.stack(ab)
    e_acc = (1 if bf else 3) * B * T * U * ab
    P = np.abs(dw) + e_acc
    d0 = np.zeros_like(dw) if dw0 is None else np.asarray(dw0, np.float64)[:, csel][:, :, osel]
    bar = e_acc + U * P + nsplit * U * P + 2 * U * (P + np.abs(d0))
    if wrong != 'dw_overwritten':
        dw = dw + d0
    # ---- the sums of q as it arrives
    if q_planes:
        qv = ((h[0][0] + h[0][1]) / (float(F32(sq0)) * qh))[:, osel]
    else:
        qv = np.concatenate([qa] + ([np.asarray(q1, F32)] if Q1 else []), axis=1).astype(np.float64)[:, osel]
    q_total = bar_total = q_seg = bar_seg = None
    if total:
        tot, tab = qv.sum((0, 2)), np.abs(qv).sum((0, 2))
        t0 = np.zeros(len(osel)) if total0 is None else np.asarray(total0, np.float64)[osel]
        o0, o1 = total_cols if total_cols is not None and wrong != 'total_all_cols' else (0, Q0 + Q1)
        sel = (osel >= o0) & (osel < o1)
        q_total = np.where(sel, t0 + tot, t0)
        bar_total = np.where(sel, (B * T + 3) * U * (tab + np.abs(t0)), 0.0)
    if seg_T:
        qs = qv
        if wrong == 'seg_from_rounded' and bf and not q_planes:
            qs = (np.concatenate([x[0] for x in h], axis=1) / col_scale[None, :, None])[:, osel]
        q_seg = qs.reshape(B, len(osel), seg_T, T // seg_T).sum(-1)
        bar_seg = (T // seg_T + 3) * U * np.abs(qv).reshape(B, len(osel), seg_T, T // seg_T).sum(-1)
    return (dw, q_total, q_seg, bar, bar_total, bar_seg, ab) if full else (dw, q_total, q_seg)


# ---------------------------------------------------------------------------------------------------- the launcher's rules
FORMS = ('ff', 'fq', 'pf', 'pq')      # p then q: f = fp32, p / q = as planes


def _is_pp(c):
    return c['form'][0] == 'p'


def _is_qp(c):
    return c['form'][1] == 'q'


def all_taps(c):
    """The tap lists of a case's problems: c['taps'], or one list per problem of a batch."""
    if not c['taps']:
        return [[]]
    return [list(tp) for tp in c['taps']] if isinstance(c['taps'][0], (list, tuple)) else [list(c['taps'])]


def tiles(c):
    return c['n'] * len(all_taps(c)[0]) * (c['Cp'] // TILE) * ((c['Q0'] + c['Q1']) // TILE)


def path(c, cus):
    """The launcher's choice: dict(kernel, odd, bf, s2, qp, pp, nsplit, tiles).  kernel 'dma' where both operands come as planes, else
    'reg'; odd (any shift of any problem with shift & 3) selects the unaligned-window variant of the register kernel and means
    nothing where p comes as planes (a shift is a row offset there)."""
    pp, qp, bf, s2 = _is_pp(c), _is_qp(c), bool(c['mode'] & 1), c.get('p_stride', 1) == 2
    odd = any(sh & 3 for tp in all_taps(c) for sh in tp)
    tl = tiles(c)
    ns = c['nsplit'] if c['nsplit'] > 0 else cus // tl
    ns = min(max(ns, 1), pairs(c['B'], c['T'])[1])
    if s2:
        key = dict(kernel='reg', odd=False, bf=False, s2=True, qp=False, pp=False)
    elif pp and qp:
        key = dict(kernel='dma', odd=False, bf=bf, s2=False, qp=True, pp=True)
    elif pp:
        key = dict(kernel='reg', odd=False, bf=bf, s2=False, qp=False, pp=True)
    else:
        key = dict(kernel='reg', odd=odd, bf=bf, s2=False, qp=qp, pp=False)
    return dict(key, nsplit=ns, tiles=tl)


def instantiation(pth):
    return tuple(pth[k] for k in ('kernel', 'odd', 'bf', 's2', 'qp', 'pp'))


def stride1_instantiations():
    """The 12: the register kernel over (odd, bf, qp) and with p as planes over bf, the LDS-DMA kernel over bf."""
    out = [('reg', odd, bf, False, qp, False) for odd in (False, True) for bf in (False, True) for qp in (False, True)]
    out += [('reg', False, bf, False, False, True) for bf in (False, True)]
    return out + [('dma', False, bf, False, True, True) for bf in (False, True)]


def legality(c):
    """None where the launch is legal, else the refusal: the launcher's rules in the launcher's order (include/vqwave.h,
    vqw_f16x3_wgrad_desc).  slab_floats: None = exactly what the launch needs at 256 CUs."""
    pp, qp = _is_pp(c), _is_qp(c)
    n = c['n']
    if not 1 <= n <= MAX_BATCH:
        return '1..32 problems per launch'
    if c['B'] <= 0 or c['T'] <= 0 or not (c['T'] % 32 == 0 or (pp and qp and not c['seg_T'])):
        return 'T a multiple of 32; any T with both operands as planes and no q_seg'
    if c['Cp'] <= 0 or c['Cp'] % TILE or c['Q0'] <= 0 or c['Q0'] % TILE or c['Q1'] < 0 or c['Q1'] % TILE:
        return 'Cp, Q0, Q1 multiples of 256'
    tp = all_taps(c)
    if not 1 <= len(tp[0]) <= MAX_TAPS:
        return '1..8 taps'
    if c.get('p_stride', 1) not in (0, 1, 2):
        return 'p_stride is 1 or 2'
    Q = c['Q0'] + c['Q1']
    lddw = c['lddw'] or Q
    if lddw < Q or lddw % 4:
        return 'lddw a multiple of 4 and >= Q0 + Q1'
    if not 0 <= c['mode'] <= 3:
        return 'mode within VQW_X3_BF16 | VQW_X3_HALF_BLOCKS'
    if c.get('shape_differs') or c.get('planes_in_one_problem'):
        return 'the problems of a batch have one shape and one operand form'
    if pp:
        kc = c['p_KC'] or c['Cp'] // 8
        ch = c['p_tap_chunk'] or [0]
        if c['p_kc0'] < 0 or min(ch) < 0 or c['p_kc0'] + max(ch) + c['Cp'] // 8 > kc:
            return 'bad chunk range of the p planes'
    if qp:
        kc = c['q_KC'] or c['Q0'] // 8
        if c['q_kc0'] < 0 or c['q_kc0'] + c['Q0'] // 8 > kc:
            return 'bad chunk range of the q planes'
    if c.get('dw_misaligned'):
        return 'dw 16-byte aligned'
    if not pp and any(sh > 0 for t_ in tp for sh in t_):
        return 'tap shifts <= 0 unless p comes as planes'
    if c['seg_T'] and (c['T'] % c['seg_T'] or (c['T'] // c['seg_T']) % 32 or (c['seg_bstride'] or Q * c['seg_T']) < Q * c['seg_T']):
        return 'q_seg needs (T / seg_T) % 32 == 0 and seg_bstride >= (Q0 + Q1) * seg_T'
    if c.get('slab_short'):
        return 'slab too small'
    if qp and c['Q1']:
        return 'q as planes needs Q1 = 0'
    if pp and c['p_relu']:
        return 'p as planes takes no p_relu'
    return None


# ---------------------------------------------------------------------------------------------------- cases
def _case(name, **kw):
    c = dict(name=name, B=2, T=64, Cp=256, Q0=256, Q1=0, taps=(-2, -1, 0), mode=0, form='ff', nsplit=2, n=1, lddw=0, tap_gap=0, col0=0,
             total=False, total_cols=None, seg_T=0, seg_bstride=0, p_relu=False, p_neg=1.0, p_KC=0, p_kc0=0, p_tap_chunk=None, p_hscale=1.0,
             q_KC=0, q_kc0=0, q_hscale=1.0, family=name.split('/')[0])
    bad = set(kw) - set(c) - {'p_stride', 'shape_differs', 'planes_in_one_problem', 'dw_misaligned', 'slab_short'}
    assert not bad, bad
    c.update(kw)
    return c


ALIGNED, UNALIGNED = (-8, -4, 0), (-2, -1, 0)
MODES = ((0, 'f16x3'), (1, 'bf16'))


def form_cases():
    """All four operand forms x aligned / unaligned shifts x fp16x3 / bf16: the 12 stride-1 instantiations (p as planes ignores the
    alignment).  Two pairs per row, two K splits; the fp32-q forms carry a q1 half."""
    out = []
    for form in FORMS:
        for taps, al in ((ALIGNED, 'aligned'), (UNALIGNED, 'unaligned')):
            for mode, mn in MODES:
                out.append(_case('forms/%s-%s-%s' % (form, al, mn), form=form, taps=taps, mode=mode, Q1=0 if form[1] == 'q' else 256,
                                 total=True, B=1 if al == 'aligned' else 2, T=32 if al == 'aligned' else 64, nsplit=1 if al == 'aligned' else 2))
    return out


def tap_cases():
    """One tap of 0; -1, -2, -3, -5 in one launch; -4, -T/2, -(T-1); -T and -2T beside 0 (whole taps in the padding); eight taps;
    positive shifts with p as planes.  B >= 2 throughout: a read before t = 0 would land in the previous batch row or channel."""
    out = []
    for form in ('ff', 'pq'):
        out.append(_case('taps/%s-1x1' % form, form=form, taps=(0,)))
        out.append(_case('taps/%s-unaligned4' % form, form=form, taps=(-1, -2, -3, -5), B=3, T=32, nsplit=3))
        for T in (64, 96):
            out.append(_case('taps/%s-T%d-far' % (form, T), form=form, T=T, taps=(-4, -T // 2, -(T - 1))))
            out.append(_case('taps/%s-T%d-padding' % (form, T), form=form, T=T, taps=(-T, -2 * T, 0), nsplit=3))
        out.append(_case('taps/%s-eight' % form, form=form, taps=tuple(range(-7, 1)), nsplit=1))
    out.append(_case('taps/fq-unaligned4-bf16', form='fq', taps=(-1, -2, -3, -5), mode=1))
    out.append(_case('taps/fq-padding', form='fq', taps=(-64, -128, -3), B=3))
    for form in ('pf', 'pq'):
        out.append(_case('taps/%s-positive' % form, form=form, taps=(1, 64, 0, -1), B=3, nsplit=3))
        out.append(_case('taps/%s-positive-T96-bf16' % form, form=form, T=96, taps=(96, 95, 2), mode=1))
    out.append(_case('taps/pq-ragged-T40', form='pq', T=40, taps=(-8, -3, 0, 5), B=3))
    out.append(_case('taps/pq-ragged-T72', form='pq', T=72, taps=(-72, -36, 1), B=2, nsplit=3))
    out.append(_case('taps/pq-ragged-T40-bf16', form='pq', T=40, taps=(-2, -1, 0), B=2, mode=1, total=True))
    return out


def rowcol_cases():
    """Cp = 512; a second column tile that is q1 with its own scale; Q0 = 512 with Q1 = 256; lddw and dw_tap_stride wider than needed;
    the residual-half form (dw a column block from column 512 of a wider matrix)."""
    out = [_case('rowcol/Cp512-ff', Cp=512), _case('rowcol/Cp512-pq', Cp=512, form='pq', T=32, nsplit=1),
           _case('rowcol/Cp512-fq-bf16', Cp=512, form='fq', mode=1), _case('rowcol/Cp512-pf', Cp=512, form='pf', Q1=256, B=1),
           _case('rowcol/Q1-ff', Q1=256, T=32), _case('rowcol/Q1-pf-bf16', Q1=256, form='pf', mode=1),
           _case('rowcol/Q0-512-Q1-ff', Q0=512, Q1=256, taps=ALIGNED), _case('rowcol/Q0-512-pq', Q0=512, form='pq'),
           _case('rowcol/lddw-ff', Q1=256, lddw=520), _case('rowcol/lddw-pq', form='pq', lddw=264, T=96, nsplit=3),
           _case('rowcol/tap-gap-ff', Cp=512, lddw=264, tap_gap=64), _case('rowcol/tap-gap-pq', form='pq', tap_gap=64),
           _case('rowcol/block-ff', col0=512, taps=(0,), B=3), _case('rowcol/block-pq', col0=512, form='pq', Q0=512, taps=(0, -1)),
           _case('rowcol/block-fq-tap-gap', col0=512, form='fq', tap_gap=64, mode=1)]
    return out


SPLITS = (1, 2, 3, 4, 5, 8, 9, 12, 17)


def split_cases():
    """Explicit nsplit on B = 3, T = 192 (18 pairs: the reduce kernel's 8-unrolled loop runs 0, 1 and 2 times, its tail 0 .. 7
    times), cuts inside a batch row and exactly at one (B = 3, T = 64: 6 pairs in 3 and in 4), an nsplit above the pairs."""
    out = [_case('splits/%d-%s' % (ns, form), form=form, B=3, T=192, nsplit=ns, taps=(-3, 0) if i % 2 else (-4, 0))
           for i, ns in enumerate(SPLITS) for form in (('ff', 'pq') if ns in (1, 9, 17) else (('ff', 'pq', 'fq', 'pf')[i % 4],))]
    out.append(_case('splits/at-a-row-ff', B=3, T=64, nsplit=3))
    out.append(_case('splits/inside-a-row-pq', form='pq', B=3, T=64, nsplit=4))
    out.append(_case('splits/inside-a-row-ff', B=3, T=96, nsplit=2))
    out.append(_case('splits/clamped-ff', nsplit=40))
    out.append(_case('splits/clamped-pq-ragged', form='pq', T=72, B=1, nsplit=5))
    return out


def auto_cases():
    """nsplit = 0 where the automatic value is not clamped at 256 CUs: 48 tiles, 6 pairs."""
    return [_case('auto/48-tiles', taps=tuple(range(-7, 1)), Cp=512, Q0=512, Q1=256, B=2, T=96, nsplit=0, total=True),
            _case('auto/one-tile-clamped-pq', form='pq', taps=(0,), nsplit=0)]


def sums_cases():
    """q_total over all columns, inside one tile, astride Q0 | Q1 and over q1 only; q_seg with seg_T = 1 and T / 32 behind a wider
    seg_bstride; both, neither, each alone; fp32 q under bf16 (sums of the unrounded q) and q as planes (of the rounded q);
    Cp = 512 with three taps (each sum must arrive once)."""
    out = [_case('sums/total-all', Q1=256, total=True), _case('sums/total-inside-a-tile', Q1=256, total=True, total_cols=(64, 200)),
           _case('sums/total-astride', Q1=256, total=True, total_cols=(200, 300)), _case('sums/total-q1-only', Q1=256, total=True, total_cols=(256, 512)),
           _case('sums/total-second-tile-pq', form='pq', Q0=512, total=True, total_cols=(300, 500)),
           _case('sums/seg1', seg_T=1, seg_bstride=256 + 3), _case('sums/seg-T32', seg_T=2, seg_bstride=2 * 256 + 8, total=True),
           _case('sums/seg-T32-pq', form='pq', T=96, seg_T=3, seg_bstride=3 * 256 + 4, nsplit=3), _case('sums/seg1-pq-total', form='pq', seg_T=1, total=True, B=3),
           _case('sums/neither-pq', form='pq'),
           _case('sums/fp32-q-bf16', mode=1, Q1=256, total=True, seg_T=2, seg_bstride=2 * 512 + 4),
           _case('sums/fp32-q-bf16-pf', form='pf', mode=1, total=True, seg_T=1),
           _case('sums/q-planes-bf16', form='pq', mode=1, total=True, seg_T=2), _case('sums/q-planes-bf16-fq', form='fq', mode=1, total=True, seg_T=1, taps=ALIGNED),
           _case('sums/q-planes-fq', form='fq', total=True, total_cols=(8, 250), seg_T=2),
           _case('sums/once-Cp512-ff', Cp=512, Q1=256, total=True, seg_T=2, total_cols=(100, 400)),
           _case('sums/once-Cp512-pq', form='pq', Cp=512, total=True, seg_T=1, B=3, nsplit=5)]
    return out


def relu_cases():
    """p_relu on fp32 p, with and without q as planes, aligned and unaligned, bf16; the negative half of p is eight times the
    positive one: a skipped relu is many bars."""
    return [_case('relu/%s-%s-%s' % (form, al, mn), form=form, taps=taps, mode=mode, p_relu=True, p_neg=8.0, T=32 if form == 'ff' else 64)
            for form in ('ff', 'fq') for taps, al in ((ALIGNED, 'aligned'), (UNALIGNED, 'unaligned')) for mode, mn in MODES]


def wide_cases():
    """Planes inside wider tensors (three layers side by side: KC = 96 chunks at Cp = Q0 = 256), tap chunks on stride 1, host-side
    factors of the planes' scales.  The other chunks hold operands of the same kind: a read from them shows."""
    return [_case('wide/p-kc0-pq', form='pq', p_KC=96, p_kc0=32), _case('wide/p-kc0-pf-bf16', form='pf', p_KC=96, p_kc0=64, mode=1, Q1=256),
            _case('wide/q-kc0-pq', form='pq', q_KC=96, q_kc0=64, total=True), _case('wide/q-kc0-fq', form='fq', q_KC=96, q_kc0=32, seg_T=1),
            _case('wide/both-kc0-pq-bf16', form='pq', p_KC=96, p_kc0=32, q_KC=64, q_kc0=32, mode=1, T=40),
            _case('wide/tap-chunk-pq', form='pq', p_KC=96, p_tap_chunk=(64, 0, 32)), _case('wide/tap-chunk-kc0-pf', form='pf', p_KC=96, p_kc0=32, p_tap_chunk=(32, 0, 32)),
            _case('wide/hscale-pq', form='pq', p_hscale=4.0, q_hscale=0.5, total=True, seg_T=1), _case('wide/q-hscale-fq-bf16', form='fq', q_hscale=2.0, mode=1, total=True),
            _case('wide/p-hscale-pf', form='pf', p_hscale=0.25)]


BATCH_TAPS = ((-2, -1, 0), (-8, -4, 0), (-32, -16, 0), (-64, -5, 0), (-3, -2, -1))


def batch_cases():
    """n = 1, 2, 5 and 32 problems of the smallest shape, each with its own taps, scales, operands and sums."""
    out = []
    for n, form, mode in ((1, 'ff', 0), (2, 'pq', 0), (2, 'fq', 1), (5, 'ff', 1), (5, 'pq', 0), (5, 'pf', 0), (32, 'pq', 0), (32, 'ff', 0)):
        taps = tuple(BATCH_TAPS[i % 5] for i in range(n))
        if form == 'ff' and n == 32:
            taps = tuple(BATCH_TAPS[1 + i % 2] for i in range(n))        # aligned shifts only: the aligned register kernel in a batch
        out.append(_case('batch/%d-%s-%s' % (n, form, MODES[mode][1]), form=form, mode=mode, n=n, taps=taps if n > 1 else taps[0], B=2, T=32,
                         nsplit=2 if n < 32 else 1, total=True, seg_T=1, seg_bstride=256 + 4))
    return out


def all_cases():
    return form_cases() + tap_cases() + rowcol_cases() + split_cases() + auto_cases() + sums_cases() + relu_cases() + wide_cases() + batch_cases()


def refusal_cases():
    """(name, case, the launcher's message) for every rule of the launcher a caller reaches through kernels.py (nine taps do not
    reach it: the descriptor has eight slots)."""
    r = lambda name, msg, **kw: (name, _case('refusals/' + name, **kw), msg)  # noqa: E731
    return [r('T40-fp32', 'T must be a positive multiple of 32', T=40),
            r('T40-planes-q_seg', 'T must be a positive multiple of 32', T=40, form='pq', seg_T=1),
            r('Cp128', 'Cp, Q0, Q1 must be multiples of 256', Cp=128), r('Q0-384', 'Cp, Q0, Q1 must be multiples of 256', Q0=384),
            r('Q1-128', 'Cp, Q0, Q1 must be multiples of 256', Q1=128), r('no-taps', '1..8 taps', taps=()),
            r('p_stride3', 'p_stride is 1 or 2', p_stride=3), r('lddw-short', 'lddw must be a multiple of 4', Q1=256, lddw=508),
            r('lddw-odd', 'lddw must be a multiple of 4', lddw=258), r('mode4', 'mode is a bit set', mode=4),
            r('positive-shift-fp32-p', 'tap shifts must be <= 0', taps=(-1, 0, 1)), r('positive-shift-fq', 'tap shifts must be <= 0', taps=(4, 0), form='fq'),
            r('p-chunks', 'bad chunk range of the p planes', form='pq', p_KC=96, p_kc0=65),
            r('p-tap-chunk', 'bad chunk range of the p planes', form='pf', p_KC=96, p_kc0=32, p_tap_chunk=(0, 33, 0)),
            r('q-chunks', 'bad chunk range of the q planes', form='fq', q_KC=48, q_kc0=17),
            r('dw-misaligned', 'dw must be 16-byte aligned', dw_misaligned=True),
            r('seg-ratio', 'q_seg needs T / seg_T to be a multiple of 32', seg_T=4), r('seg-bstride', 'q_seg needs T / seg_T to be a multiple of 32', seg_T=2, seg_bstride=511),
            r('slab-short', 'slab too small', slab_short=True), r('q-planes-Q1', 'q as planes needs p_stride 1, Q1 = 0', form='fq', Q1=256),
            r('p-planes-relu', 'p as planes needs p_stride 1, no p_relu', form='pf', p_relu=True),
            r('batch-shape', 'differs from problem 0 in shape or layout', n=2, taps=(UNALIGNED, UNALIGNED), shape_differs=True),
            r('batch-planes-in-one', 'an operand as planes in every problem or in none', n=2, taps=(UNALIGNED, UNALIGNED), form='fq', planes_in_one_problem=True),
            r('batch-33', '1..32 problems per launch', n=33, taps=tuple(UNALIGNED for _ in range(33)), B=1, T=32, nsplit=1)]


# ---------------------------------------------------------------------------------------------------- operands
def wide_channels(c):
    """(channels of the p tensor, channels of the q0 tensor): the wider planes tensors where the case has them."""
    return (8 * c['p_KC'] if _is_pp(c) and c['p_KC'] else c['Cp']), (8 * c['q_KC'] if _is_qp(c) and c['q_KC'] else c['Q0'])


def inputs(c, kind, i=0):
    """Operands of problem i of a case: p [B][Cw][T], q0 [B][Qw][T], q1 [B][Q1][T] or None, dw0 [ntaps][Cp][Q0 + Q1], total0 [Q0 + Q1],
    the power-of-two guard scales sp, sq0, sq1 (every problem of a batch has its own)."""
    rng = np.random.default_rng(seed_of('x3_wgrad', c['name'], kind, i))
    B, T, Q = c['B'], c['T'], c['Q0'] + c['Q1']
    Cw, Qw = wide_channels(c)
    nt = len(all_taps(c)[i]) if c['taps'] else 1
    e = i % 3 - 1
    if kind == 'ints':
        p = ints(rng, (B, Cw, T), 4)
        out = dict(p=p, q0=ints(rng, (B, Qw, T), 4), q1=ints(rng, (B, c['Q1'], T), 4) if c['Q1'] else None, dw0=ints(rng, (nt, c['Cp'], Q), 8),
                   total0=ints(rng, Q, 8), sp=4.0 * 2.0 ** e, sq0=8.0 * 2.0 ** -e, sq1=2.0)
    else:
        g = lambda *s: rng.standard_normal(s).astype(F32)  # noqa: E731
        p = g(B, Cw, T)
        out = dict(p=p, q0=(g(B, Qw, T) * F32(1e-5)).astype(F32), q1=(g(B, c['Q1'], T) * F32(3e-5)).astype(F32) if c['Q1'] else None,
                   dw0=(g(nt, c['Cp'], Q) * F32(1e-4)).astype(F32), total0=(g(Q) * F32(1e-4)).astype(F32), sp=SP * 2.0 ** e, sq0=SQ0 * 2.0 ** -e, sq1=SQ1)
    if c['p_neg'] != 1.0:
        out['p'] = np.where(p < 0, p * F32(c['p_neg']), p).astype(F32)
    return out


def reference(c, ins, i=0, nsplit=None, wrong=None, csel=None, osel=None):
    """wgrad(full=True) of problem i of a case over its operands `ins`; nsplit: what path() named (default: the case's own, for
    cases whose count does not depend on the device)."""
    ns = nsplit if nsplit is not None else path(c, 256)['nsplit']
    return wgrad(ins['p'], ins['q0'], ins['q1'], all_taps(c)[i], ins['sp'], ins['sq0'], ins['sq1'], Cp=c['Cp'], Q0=c['Q0'], mode=c['mode'],
                 p_planes=_is_pp(c), q_planes=_is_qp(c), p_hscale=c['p_hscale'], q_hscale=c['q_hscale'], p_kc0=c['p_kc0'], p_tap_chunk=c['p_tap_chunk'],
                 q_kc0=c['q_kc0'], p_relu=c['p_relu'], dw0=ins['dw0'], total=c['total'], total0=ins['total0'], total_cols=c['total_cols'],
                 seg_T=c['seg_T'], nsplit=ns, csel=csel, osel=osel, wrong=wrong, full=True)


def plane_images(c, ins):
    """The uint16 images [planes][KC][B * T][8] of the operands that come as planes (None for an fp32 operand), made at
    guard scale * host factor, all chunks of a wider tensor included (they hold the other layers' operands)."""
    pp = X.act_planes(ins['p'], c['p_hscale'], ins['sp'], mode=c['mode'] & 1) if _is_pp(c) else None
    qp = X.act_planes(ins['q0'], c['q_hscale'], ins['sq0'], mode=c['mode'] & 1) if _is_qp(c) else None
    return pp, qp


def sample_rows(c):
    """Rows and columns of dw for the CPU tests: the edges of every 256-tile and a few inside."""
    edge = lambda n: np.array(sorted({k * TILE + d for k in range(n // TILE) for d in (0, 1, 97, 254, 255)}))  # noqa: E731
    return edge(c['Cp']), edge(c['Q0'] + c['Q1'])


# ---------------------------------------------------------------------------------------------------- fp32 emulations
def emulate(c, ins, csel, osel, order, nsplit, i=0):
    """The same sums step by step in fp32 for the rows csel x columns osel: products of plane values (exact in fp32) added one at a
    time, (b, t) ascending, the terms of a step in the order a1 b2, a2 b1, a1 b1.  order 'time': one accumulator, descaled once.
    order 'split': nsplit accumulators over the K ranges of split_range, each descaled, then added in ascending order.  The result
    is added onto dw0.  Returns (dw, q_total, q_seg) as float32 (sums None where the case has none)."""
    B, T, Q0, bf = c['B'], c['T'], c['Q0'], bool(c['mode'] & 1)
    taps = all_taps(c)[i]
    pp, qp = _is_pp(c), _is_qp(c)
    ph, qh = (c['p_hscale'] if pp else 1.0), (c['q_hscale'] if qp else 1.0)
    pin = np.maximum(ins['p'], F32(0)) if c['p_relu'] else ins['p']
    a_all = pieces(pin, ins['sp'] * ph, bf)
    chunk = c['p_tap_chunk'] or [0] * len(taps)
    qa = ins['q0'][:, 8 * c['q_kc0']:8 * c['q_kc0'] + Q0]
    hq = [pieces(qa, ins['sq0'] * qh, bf)] + ([pieces(ins['q1'], ins['sq1'], bf)] if c['Q1'] else [])
    b1, b2 = (np.concatenate([x[k] for x in hq], axis=1)[:, osel].astype(F32) for k in (0, 1))
    col_scale = np.concatenate([np.full(Q0, ins['sq0'] * qh), np.full(c['Q1'], ins['sq1'])])[osel]
    inv = (1.0 / (ins['sp'] * ph * col_scale)).astype(F32)[None, None, :]
    t = np.arange(T)
    g = [tuple(X.gather(x[:, 8 * (c['p_kc0'] + chunk[j]) + csel], t + sh).astype(F32) for x in a_all) for j, sh in enumerate(taps)]
    parts = [(0, pairs(B, T)[1])] if order == 'time' else [split_range(B, T, nsplit, k) for k in range(nsplit)]
    total = np.zeros((len(taps), len(csel), len(osel)), F32)
    for lo, hi in parts:
        acc = np.zeros_like(total)
        on = step_mask(B, T, lo, hi)
        for b in range(B):
            for tt in np.flatnonzero(on[b]):
                a1 = np.stack([gj[0][b, :, tt] for gj in g])[:, :, None]
                a2 = np.stack([gj[1][b, :, tt] for gj in g])[:, :, None]
                q1_, q2_ = b1[b, :, tt][None, None, :], b2[b, :, tt][None, None, :]
                acc = S._seq(acc, (a1 * q1_,) if bf else (a1 * q2_, a2 * q1_, a1 * q1_))
        total = (total + (acc * inv).astype(F32)).astype(F32)
    dw = (ins['dw0'][:, csel][:, :, osel] + total).astype(F32)
    if qp:
        qv = ((hq[0][0].astype(F32) + hq[0][1].astype(F32)).astype(F32) * F32(1.0 / (ins['sq0'] * qh))).astype(F32)[:, osel]
    else:
        qv = np.concatenate([qa] + ([ins['q1']] if c['Q1'] else []), axis=1)[:, osel].astype(F32)
    q_total = q_seg = None
    if c['total']:
        o0, o1 = c['total_cols'] or (0, Q0 + c['Q1'])
        acc = ins['total0'][osel].astype(F32)
        for b in range(B):
            for tt in range(T):
                acc = (acc + qv[b, :, tt]).astype(F32)
        q_total = np.where((osel >= o0) & (osel < o1), acc, ins['total0'][osel]).astype(F32)
    if c['seg_T']:
        q_seg = np.zeros((B, len(osel), c['seg_T']), F32)
        r = T // c['seg_T']
        for tt in range(T):
            q_seg[:, :, tt // r] = (q_seg[:, :, tt // r] + qv[:, :, tt]).astype(F32)
    return dw, q_total, q_seg
