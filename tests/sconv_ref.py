"""Plane-exact float64 reference of the encoder's stride-2 convs on the fp16x3 engine -- vqw_f16x3_strided_conv (forward, input
gradient, split-K) and the stride-2 forms of vqw_f16x3_wgrad --, their seeded case tables and their bars, for
tests/test_sconv_ref_cpu.py and tests/test_sconv_kernels_gpu.py.

numpy only, float64, written from the sentences of include/vqwave.h ("The encoder's stride-2 convs on the fp16x3 engine",
"Weight gradient of conv1d_v2") and not from the kernels' index arithmetic.  The number format comes from tests/x3_ref.py:
every operand is scaled by its power of two (scaled), split into two fp16 planes h1, h2 (split), and a product is
a1 b1 + a1 b2 + a2 b1 summed in float64 and divided by the scales -- plane-exact, like x3_ref.contract.  What is left to the
device is its fp32 accumulation and its fp32 epilogue, and the bars bound exactly that.

Bars, elementwise, U = 2^-24.  abs_sum is the sum of the absolute values of the addends of the same contraction (returned by
every reference function, in the units of the unscaled result), n the number of products summed:

    e_acc       = n * U * abs_sum           n = 3 * taps * channels (forward; input gradient: the taps of the element's parity),
                                            n = 3 * B * T for a weight gradient.  The bound of a recursive fp32 sum of n terms
                                            in ANY order, so split-K launches and the split weight gradient have no other bar.
    P           = |pre| + e_acc             the magnitude the epilogue sees
    input grad.   bar = e_acc + U * P                                   (* winv)
    save_r      : e_r = e_acc + U * P + [bias] U * (P + |bias|)         (* winv, + bias; the relu adds no rounding and is
                                                                         1-Lipschitz)
    out         : R = |r| + e_r;  bar = e_r  without bn_scale, else
                  |bn_scale| * e_r + U * |bn_scale| * R + U * (|bn_scale| * R + |bn_shift|)      (the product, the sum)
    dw          : e_acc + U * P + 2U * (P + |dw0|)                      (* 1 / (sp sq), the add onto the pre-filled value)
    q_total     : (B * T + 3) * U * (sum |q| + |total0|)                (any-order sum of B * T values that may each have been
                                                                         formed by one fp32 add of two planes, atomics onto
                                                                         the pre-filled value)

One constant was moved, because the sequential fp32 emulation of tests/test_sconv_ref_cpu.py did not fit and before any kernel
had run against it: the add onto the pre-filled dw from U to 2U * (P + |dw0|).  One rounding to nearest attains U * |result|
just above a power of two, so a term of exactly one rounding is the whole bar wherever the update is small against dw0 -- at
B * T = 4, where a tap behind Tp sums two products, the emulation reached 0.88 of the first form over the 8 x 256 x 256
elements; a bar cannot leave a quarter of itself free for less than 4/3 roundings.  (The epilogues of the convs keep one U
per rounding: there e_acc, of n >= 192 products, is never small against them.  e_acc has n, not n - 1, for the reason given in
tests/pointwise_ref.py: n - 1 is attained at n = 2.)  The emulation then stays under EMU_FRACTION of every bar.  e_acc grows
with n * abs_sum ~ n^2 while the rounding error of a sum of n random terms grows with sqrt(n): measured errors are small
fractions of these bars, and the sharp test for a misplaced tap, chunk, parity or column is the exact-integer kind below.

Two kinds of operands per case (as tests/pointwise_ref.py):
 'ints'    integers |x| <= 4, |w| <= 2, integer bias / shift, bn_scale in {+-1, +-2, +-0.5}, power-of-two scales: every low
           plane is zero and every partial sum in every order is exact in fp32 -- the device must equal the reference bit for bit.
 'normal'  standard-normal activations, weights scaled by (ks * Cin)^-1/2, gradients scaled by 1e-4 and lifted by 2^22.

Deliberately wrong evaluations (`wrong=` of the reference functions, WRONG below) are told apart from the right one by
tests/test_sconv_ref_cpu.py."""
import zlib

import numpy as np

import x3_ref as X

U = 2.0 ** -24
EMU_FRACTION = 0.75
F32 = np.float32
GUARD = 64                  # floats on either side of an output (256 bytes: views keep 16-byte alignment)
SENTINEL = F32(-1234.5)
MAX_COLS, MAX_CIN, MAX_M = 800, 256, 768
SPLIT_MAX = 8               # at most 8 partial tiles per fix-up

WRONG = ('pad_plus_one', 'parity_swap', 'leak', 'drop_last_tap', 'drop_last_chunk', 'drop_last_col', 'drop_split',
         'bias_after_relu', 'bn_on_save_r', 'relu_forced', 'wgrad_no_zero_behind_tp', 'dw_overwritten', 'no_h2h1')


def seed_of(*parts):
    return zlib.crc32(repr(parts).encode()) & 0x7fffffff


def unsplit(x32):
    """In place of x3_ref.split: the operand itself as the first plane, no second plane (float64 of the fp32 value)."""
    x = np.asarray(x32, F32).astype(np.float64)
    return x, np.zeros_like(x)


# the planes of an operand, the three products and a read with zero outside the batch row: shared with tests/x3_conv_ref.py
_planes, _three, _gather = X.planes_of, X.three_terms, X.gather


def _inv(sa, sb):
    return 1.0 / (float(F32(sa)) * float(F32(sb)))


# ---------------------------------------------------------------------------------------------------- forward
def fwd_operands(x1, x2, ks, pad_left, T, leak=False):
    """The two planes of x [B][C][2T] as the operand of ONE contraction over (tap, channel): [B][ks * C][T], tap j reading
    sample 2t + j - pad_left (zero outside [0, 2T): the padding behind is implicit in ks and pad_left)."""
    t = np.arange(T)
    return tuple(np.concatenate([_gather(h, 2 * t + j - pad_left, leak) for j in range(ks)], axis=1) for h in (x1, x2))


def fwd_operands_s2d(planes, B, C, T, ks, pad_left):
    """The same operands decoded from the VQW_X3_S2D image x3_ref.act_planes(x [B][C][2T]) returns: tap j with e = j - pad_left
    is chunk block e & 1 at row offset e >> 1 (a stride-1 read of the space-to-depth planes)."""
    img = planes.view(np.float16).astype(np.float64)                    # [2][2 C/8][B T][8]
    out = []
    for p in (0, 1):
        taps = []
        for j in range(ks):
            e = j - pad_left
            blk = img[p, (e & 1) * (C // 8):((e & 1) + 1) * (C // 8)]       # [C/8][B T][8]
            rows = blk.transpose(1, 0, 2).reshape(B, T, C).transpose(0, 2, 1)   # [B][C][T]
            taps.append(_gather(rows, np.arange(T) + (e >> 1)))
        out.append(np.concatenate(taps, axis=1))
    return tuple(out)


def kmask_all(ks, C):
    return np.ones((ks, C), dtype=bool)


def fwd_pre(x, w, pad_left, sx, sw, split=X.split, kmask=None, wrong=None, operands=None):
    """(pre, abs_sum) [B][M][T] of sum_j sum_c w[j][c][m] x[b][c][2t + j - pad_left]; kmask [ks][C]: the (tap, channel) pairs summed."""
    ks, C, M = w.shape
    B, _, L = x.shape
    T = L // 2
    w1, w2 = _planes(w, sw, split)
    if kmask is not None:
        w1, w2 = w1 * kmask[:, :, None], w2 * kmask[:, :, None]
    if operands is None:
        x1, x2 = _planes(x, sx, split)
        operands = fwd_operands(x1, x2, ks, pad_left + (wrong == 'pad_plus_one'), T, leak=(wrong == 'leak'))
    val, ab = _three(operands[0], operands[1], w1.reshape(ks * C, M), w2.reshape(ks * C, M), wrong == 'no_h2h1')
    inv = _inv(sx, sw)
    return val * inv, ab * inv


def fwd_epilogue(pre, abs_sum, n, bias, bn_scale, bn_shift, relu, wrong=None):
    """(out, save_r, bar_out, bar_r) of the header's bias -> relu -> BatchNorm affine over a pre-activation [B][M][T]."""
    col = lambda v: np.asarray(v, np.float64)[None, :, None]  # noqa: E731
    e_acc = n * U * abs_sum
    P = np.abs(pre) + e_acc
    e_r = e_acc + U * P
    r = pre
    if bias is not None and wrong != 'bias_after_relu':
        r = r + col(bias)
        e_r = e_r + U * (P + np.abs(col(bias)))
    if relu or wrong == 'relu_forced':
        r = np.maximum(r, 0.0)
    if bias is not None and wrong == 'bias_after_relu':
        r = r + col(bias)
    out, bar = r, e_r
    if bn_scale is not None:
        s, h = col(bn_scale), col(bn_shift)
        R = np.abs(r) + e_r
        out = s * r + h
        bar = np.abs(s) * e_r + U * np.abs(s) * R + U * (np.abs(s) * R + np.abs(h))
    save_r = out if wrong == 'bn_on_save_r' else r
    return out, save_r, bar, e_r


def sconv_fwd(x, w, bias, bn_scale, bn_shift, relu, pad_left, sx=1.0, sw=1.0, split=X.split, kmask=None, wrong=None,
              operands=None, full=False):
    """out[b][m][t] = bn_scale[m] * relu(pre + bias[m]) + bn_shift[m], save_r = the value the affine is applied to; bias,
    bn_scale / bn_shift and the relu are optional.  Returns (out, save_r), or with full (out, save_r, bar_out, bar_r, abs_sum)."""
    ks, C, M = w.shape
    pre, ab = fwd_pre(x, w, pad_left, sx, sw, split, kmask, wrong, operands)
    out, r, bar, bar_r = fwd_epilogue(pre, ab, 3 * ks * C, bias, bn_scale, bn_shift, relu, wrong)
    if wrong == 'drop_last_col':
        out, r = out.copy(), r.copy()
        out[-1, :, -1] = 0.0
        r[-1, :, -1] = 0.0
    return (out, r, bar, bar_r, ab) if full else (out, r)


# ---------------------------------------------------------------------------------------------------- input gradient
def dgrad_taps(ks, pad_left, r):
    """The taps j that reach output parity r: 2t + j - pad_left = u with u = r (mod 2)."""
    return [j for j in range(ks) if (j - pad_left - r) % 2 == 0]


def sconv_dgrad(dy, wt, pad_left, sx=1.0, sw=1.0, split=X.split, kmask=None, wrong=None, full=False):
    """dx[b][m][u] (u < 2T) = sum_{j, t: 2t + j - pad_left = u} sum_o wt[j][o][m] dy[b][o][t]; dy [B][O][T], wt [ks][O][M].
    Returns dx, or with full (dx, bar, abs_sum)."""
    ks, O, M = wt.shape
    B, _, T = dy.shape
    pl = pad_left + (wrong == 'pad_plus_one')
    w1, w2 = _planes(wt, sw, split)
    if kmask is not None:
        w1, w2 = w1 * kmask[:, :, None], w2 * kmask[:, :, None]
    y1, y2 = _planes(dy, sx, split)
    u = np.arange(2 * T)
    ops = ([], [])
    for j in range(ks):
        num = u + pl - j                                                # = 2t
        idx = np.where(num % 2 == 0, num // 2, -(10 ** 9))             # the other parity: no t
        for h, o in zip((y1, y2), ops):
            g = _gather(h, idx, leak=(wrong == 'leak'))
            o.append(g * (num % 2 == 0) if wrong == 'leak' else g)
    a1, a2 = (np.concatenate(o, axis=1) for o in ops)
    val, ab = _three(a1, a2, w1.reshape(ks * O, M), w2.reshape(ks * O, M), wrong == 'no_h2h1')
    inv = _inv(sx, sw)
    dx, ab = val * inv, ab * inv
    ntap = np.array([len(dgrad_taps(ks, pad_left, r)) for r in (0, 1)])[u % 2]
    e_acc = (3 * O * ntap)[None, None, :] * U * ab
    bar = e_acc + U * (np.abs(dx) + e_acc)
    if wrong == 'parity_swap':
        dx = dx.reshape(B, M, T, 2)[..., ::-1].reshape(B, M, 2 * T)
    if wrong == 'drop_last_col':
        dx = dx.copy()
        dx[-1, :, -2:] = 0.0
    return (dx, bar, ab) if full else dx


# ---------------------------------------------------------------------------------------------------- weight gradient
def wgrad_s2(p, q, taps, Tp, sp=1.0, sq=1.0, split=X.split, dw0=None, total0=None, total_cols=None, q_from_planes=False,
             wrong=None, full=False):
    """dw[j][c][o] = sum_{b,t} p[b][c][2t + taps[j]] q[b][o][t], zero outside [0, Tp); p [B][C][Tp], q [B][O][T].  With dw0 the
    value accumulated onto it.  q_total[o] = sum_{b,t} q[b][o][t] (of q as it arrives: the fp32 values, or h1 + h2 over sq where
    q comes as planes), added onto total0 over the columns total_cols.  Returns (dw, q_total), with full
    (dw, q_total, bar_dw, bar_total, abs_sum)."""
    B, C, _ = p.shape
    O, T = q.shape[1:]
    assert p.shape[2] == Tp
    p1, p2 = _planes(p, sp, split)
    q1, q2 = _planes(q, sq, split)
    t = np.arange(T)
    inv = _inv(sp, sq)
    qf = lambda h: h.transpose(1, 0, 2).reshape(O, B * T)  # noqa: E731
    dw, ab = [], []
    for sh in taps:
        idx = 2 * t + sh
        if wrong == 'wgrad_no_zero_behind_tp':
            # the rows of p are one flat array: behind a row lies the next channel's first sample
            g = []
            for h in (p1, p2):
                flat = np.concatenate([h.reshape(-1), np.zeros(2 * T + 16)])
                base = (np.arange(B * C) * Tp).reshape(B, C, 1)
                g.append(np.where(idx >= 0, flat[np.clip(base + idx, 0, flat.size - 1)], 0.0))
        else:
            g = [_gather(h, idx) for h in (p1, p2)]
        a1, a2 = (h.transpose(1, 0, 2).reshape(C, B * T) for h in g)
        v = a1 @ (qf(q1) + qf(q2)).T
        s = np.abs(a1) @ (np.abs(qf(q1)) + np.abs(qf(q2))).T
        if wrong != 'no_h2h1':
            v, s = v + a2 @ qf(q1).T, s + np.abs(a2) @ np.abs(qf(q1)).T
        dw.append(v * inv)
        ab.append(s * inv)
    dw, ab = np.stack(dw), np.stack(ab)
    e_acc = 3 * B * T * U * ab
    P = np.abs(dw) + e_acc
    bar = e_acc + U * P
    if dw0 is not None:
        d0 = np.asarray(dw0, np.float64)
        bar = bar + 2 * U * (P + np.abs(d0))
        if wrong != 'dw_overwritten':
            dw = dw + d0
    qv = (q1 + q2) / float(F32(sq)) if q_from_planes else np.asarray(q, F32).astype(np.float64)
    tot, tab = qv.sum((0, 2)), np.abs(qv).sum((0, 2))
    t0 = np.zeros(O) if total0 is None else np.asarray(total0, np.float64)
    o0, o1 = total_cols if total_cols is not None else (0, O)
    sel = (np.arange(O) >= o0) & (np.arange(O) < o1)
    q_total = np.where(sel, t0 + tot, t0)
    bar_total = np.where(sel, (B * T + 3) * U * (tab + np.abs(t0)), 0.0)
    return (dw, q_total, bar, bar_total, ab) if full else (dw, q_total)


# ---------------------------------------------------------------------------------------------------- the entry point's rules
def steps(c):
    """K steps of 16 channels: (forward) or (parity 0, parity 1) of an input gradient."""
    spt = c['Cin'] // 16
    if not c['dgrad']:
        return (c['ks'] * spt,)
    return tuple(len(dgrad_taps(c['ks'], c['pad_left'], r)) * spt for r in (0, 1))


def fits(c, S):
    """The K steps of every parity divide into S even parts of at least 8 steps."""
    return S >= 1 and all(st % (2 * S) == 0 and st // S >= 8 for st in steps(c))


def col_tiles(c):
    return -(-c['B'] * c['T'] // 256)


def split_tiles(c):
    """128-row tiles of a split launch: one per 128 rows, column tile and (input gradient) output parity."""
    return (c['M'] // 128) * col_tiles(c) * (2 if c['dgrad'] else 1)


def slab_floats(c, S):
    return split_tiles(c) * S * 128 * 256


def legality(c):
    """None where the header declares the launch legal, else the refusal (include/vqwave.h, vqw_f16x3_sconv_desc)."""
    if c['B'] <= 0 or c['T'] <= 0:
        return 'B, T > 0'
    if c['Cin'] < 64 or c['Cin'] % 32 or c['M'] <= 0 or c['M'] % 128:
        return 'Cin a multiple of 32 from 64, M a multiple of 128'
    if not (2 <= c['ks'] <= 8 and 0 <= c['pad_left'] < c['ks']):
        return '2..8 taps, 0 <= pad_left < ks'
    if c.get('bn_scale') and not c.get('bn_shift', c.get('bn_scale')):
        return 'bn_scale needs bn_shift'
    if not c.get('w_scale_inv', 1.0) > 0:
        return 'w_scale_inv must be positive'
    sh = c.get('shape', 0)
    if sh not in (0, 1, 2, 3, 4, 5) or (sh == 3 and c['M'] % 256) or (sh == 4 and c['M'] % 192):
        return 'shape 0..5; 3 needs M % 256 == 0, 4 needs M % 192 == 0'
    if c.get('slab') and c.get('ksplit', 0) != 1 and sh in (0, 2):
        if not c.get('counters', True):
            return 'split_slab needs split_counters'
        S = c.get('ksplit', 0)
        if S > 1:
            if not fits(c, S):
                return 'the K steps do not divide into %d even parts of >= 8' % S
            if c.get('slab_floats', slab_floats(c, S)) < slab_floats(c, S) or c.get('counters_n', split_tiles(c)) < split_tiles(c):
                return 'split scratch too small'
    return None


def path(c, cus):
    """The launcher's choice: dict(shape = block shape 1..5, S = blocks per tile (1: unsplit), rounds = 0 (unsplit), 1 or 2)."""
    nt, M = col_tiles(c), c['M']
    forced = c.get('shape', 0)
    if c.get('slab') and c.get('ksplit', 0) != 1 and forced in (0, 2):          # 128-row blocks only
        S, tiles = c.get('ksplit', 0), split_tiles(c)
        if S == 0:
            for n in range(2, SPLIT_MAX + 1):                                  # as many as fill the chip once
                if fits(c, n) and tiles * n <= cus:
                    S = n
            if S == 0 and (M // 128) * nt * 3 <= cus:                          # two thirds of the chip idle: up to two rounds
                for n in range(2, SPLIT_MAX + 1):
                    if fits(c, n) and tiles * n <= 2 * cus:
                        S = n
        if S > 1:
            return dict(shape=2, S=S, rounds=1 if tiles * S <= cus else 2)
    shape = forced
    if shape == 0:
        shape = 3 if M % 256 == 0 and (M // 256) * nt * 2 > cus else 2         # 256-row blocks fill more than half of the chip
        if shape == 3 and M % 192 == 0 and (M // 192) * nt <= cus:
            shape = 4                                                          # 192-row blocks fill more CUs in one round
        if shape == 2 and (M // 128) * nt * 4 <= cus:
            shape = 5                                                          # three quarters of the chip idle: 64-row blocks
    return dict(shape=shape, S=1, rounds=0)


def split_kmask(c, S, part):
    """[ks][Cin] bool: the (tap, channel) pairs of split `part` of S -- K steps run tap by tap, 16 channels per step, each parity of
    an input gradient on its own."""
    ks, C = c['ks'], c['Cin']
    spt = C // 16
    mask = np.zeros((ks, C), dtype=bool)
    groups = [list(range(ks))] if not c['dgrad'] else [dgrad_taps(ks, c['pad_left'], r) for r in (0, 1)]
    for taps in groups:
        n = len(taps) * spt // S
        for s in range(part * n, (part + 1) * n):
            mask[taps[s // spt], (s % spt) * 16:(s % spt + 1) * 16] = True
    return mask


# ---------------------------------------------------------------------------------------------------- cases
GEOMETRIES = (        # (B, T_out, Cin, M, ks, pad_left)
    (1, 1, 64, 128, 2, 0), (5, 3, 64, 128, 3, 1), (2, 128, 64, 128, 5, 1), (1, 257, 96, 128, 5, 2), (3, 104, 128, 256, 5, 1),
    (7, 37, 64, 384, 4, 1), (8, 96, 128, 768, 5, 1), (2, 40, 64, 128, 8, 0), (2, 40, 64, 128, 8, 7), (2, 40, 64, 128, 8, 3),
    (2, 40, 64, 128, 2, 1))
OPTION_SETS = (       # (name, bias, bn, relu, save_r)
    ('all', True, True, True, True), ('none', False, False, False, False), ('bias', True, False, False, False),
    ('bn_relu', False, True, True, False), ('save_r', True, False, True, True))
SCALE_MODES = ('dev', 'host')     # device scalars x_scale / w_scale with w_scale_inv = 1; NULL slots and a host-side w_scale_inv
KINDS = ('ints', 'normal')


def shapes_for(M):
    return [0, 1, 2] + ([3] if M % 256 == 0 else []) + ([4] if M % 192 == 0 else []) + [5]


def _case(B, T, Cin, M, ks, pad_left, dgrad, **kw):
    c = dict(B=B, T=T, Cin=Cin, M=M, ks=ks, pad_left=pad_left, dgrad=bool(dgrad), shape=0, slab=False, ksplit=0, expect=None)
    c.update(kw)
    c['name'] = '%s-B%d-T%d-C%d-M%d-k%d-p%d%s%s' % ('dgrad' if dgrad else 'fwd', B, T, Cin, M, ks, pad_left,
                                                   '-ksplit%d' % c['ksplit'] if c['slab'] else '', kw.get('tag', ''))
    return c


def dgrad_channels(Cin, M):
    """The input gradient contracts the forward pass's output channels: (Cin, M) swapped where the swapped pair is itself legal and
    inside the size limits, otherwise as they stand."""
    return (M, Cin) if Cin % 128 == 0 and M <= MAX_CIN else (Cin, M)


def table_cases():
    """The geometry table, forward and input gradient (every block shape and option set is run inside the test)."""
    out = []
    for (B, T, Cin, M, ks, pl) in GEOMETRIES:
        out.append(_case(B, T, Cin, M, ks, pl, False))
        Cd, Md = dgrad_channels(Cin, M)
        out.append(_case(B, T, Cd, Md, ks, pl, True))
    return out


def split_cases():
    """Explicit ksplit through split_slab / split_counters (shape 0 and forced shape 2)."""
    out = []
    for Cin, ks, splits in ((128, 5, (2, 4, 5)), (192, 4, (3, 6)), (256, 5, (8,))):
        for S in splits:
            out.append(_case(3, 104, Cin, 256, ks, 1, False, slab=True, ksplit=S, shape=(0, 2)[S % 2]))
    for pl in (1, 2):
        out.append(_case(3, 104, 128, 128, 5, pl, True, slab=True, ksplit=2, shape=(0, 2)[pl % 2]))
    for S in (2, 4):
        out.append(_case(7, 37, 256, 256, 5, 1, True, slab=True, ksplit=S))
    return out


def ignored_split_cases():
    """An explicit ksplit > 1 with a forced shape 1, 3, 4 or 5 runs unsplit (128-row blocks only)."""
    return [_case(3, 104, 128, 768, 5, 1, dg, slab=True, ksplit=2, shape=sh, tag='-shape%d' % sh) for sh in (1, 3, 4, 5) for dg in (False, True)]


def auto_cases(cus):
    """shape = 0 (and ksplit = 0 with scratch) on geometries sized from the CU count so that every outcome of the automatic rules is
    reached: `expect` is what path(case, cus) must say.  Shapes 3 and 4 and the cus-bound split outcomes need more than MAX_COLS
    columns at any real CU count; they keep the smallest K (Cin = 64, two taps) instead.  Shape 1 is never chosen automatically."""
    out = []
    # block shapes, no scratch: 5 (a quarter of the chip), 2, 4 (192-row blocks fit in one round), 3
    out.append(_case(2, 40, 64, 128, 2, 1, False, expect=dict(shape=5, S=1, rounds=0), tag='-auto5'))
    out.append(_case(2, 40, 64, 128, 2, 1, True, expect=dict(shape=5, S=1, rounds=0), tag='-auto5'))
    nt = cus // 4 + 1                                  # 128 rows: nt * 4 > cus, M % 256 != 0
    out.append(_case(nt, 256, 64, 128, 2, 0, False, expect=dict(shape=2, S=1, rounds=0), tag='-auto2'))
    nt = cus // 6 + 1                                  # 768 rows: 3 * nt * 2 > cus and 4 * nt <= cus
    if 4 * nt <= cus:
        out.append(_case(nt, 256, 64, 768, 2, 0, False, expect=dict(shape=4, S=1, rounds=0), tag='-auto4'))
        out.append(_case(nt - 1, 256 + 7, 64, 768, 2, 1, True, expect=dict(shape=4, S=1, rounds=0), tag='-auto4'))
    nt = cus // 2 + 1                                  # 256 rows (no multiple of 192): nt * 2 > cus
    out.append(_case(nt, 256, 64, 256, 2, 0, False, expect=dict(shape=3, S=1, rounds=0), tag='-auto3'))
    # split outcomes with scratch and ksplit = 0
    out.append(_case(3, 104, 128, 128, 5, 1, False, slab=True, expect=dict(shape=2, S=5 if 10 <= cus else 4 if 8 <= cus else 2, rounds=1), tag='-one-round'))
    out.append(_case(3, 104, 128, 128, 5, 1, True, slab=True, expect=dict(shape=2, S=2, rounds=1), tag='-one-round'))
    t0 = cus // 3                                      # input gradient (two taps of 8 steps per parity), cus / 4 < tiles <= cus / 3:
                                                       # two blocks per tile in two rounds
    if 4 * t0 > cus:
        out.append(_case(t0, 256 - 3, 128, 128, 4, 1, True, slab=True, expect=dict(shape=2, S=2, rounds=2), tag='-two-rounds'))
    t0 = cus // 2 + 1                                  # 16 steps would split in two, but two blocks per tile overfill the chip: unsplit
    out.append(_case(t0, 256, 128, 128, 2, 0, False, slab=True, expect=dict(shape=2, S=1, rounds=0), tag='-no-split-cus'))
    out.append(_case(5, 3, 64, 128, 3, 1, False, slab=True, expect=dict(shape=5, S=1, rounds=0), tag='-no-split-fits'))
    return out


def all_sconv_cases(cus=256):
    return table_cases() + split_cases() + ignored_split_cases() + auto_cases(cus)


def refusal_cases():
    """(name, case) pairs the entry point must refuse; the geometry otherwise that of a legal case."""
    base = dict(B=2, T=40, Cin=64, M=128, ks=5, pad_left=1, dgrad=False, shape=0, slab=False, ksplit=0)
    sp = dict(base, B=3, T=104, Cin=128, M=256, slab=True)
    mk = lambda d, **kw: dict(d, **kw)  # noqa: E731
    return [('Cin32', mk(base, Cin=32)), ('Cin80', mk(base, Cin=80)), ('M192', mk(base, M=192)), ('ks1', mk(base, ks=1, pad_left=0)),
            ('ks9', mk(base, ks=9)), ('pad_left=ks', mk(base, pad_left=5)), ('bn_scale without bn_shift', mk(base, bn_scale=True, bn_shift=False)),
            ('w_scale_inv=0', mk(base, w_scale_inv=0.0)), ('shape3 at M384', mk(base, M=384, shape=3)),
            ('shape4 at M256', mk(base, M=256, shape=4)), ('shape6', mk(base, shape=6)),
            ('ksplit3 at 40 steps', mk(sp, ksplit=3)), ('ksplit8 at 40 steps', mk(sp, ksplit=8)),
            ('slab one float short', mk(sp, ksplit=2, slab_floats=slab_floats(sp, 2) - 1)),
            ('counters one short', mk(sp, ksplit=2, counters_n=split_tiles(sp) - 1)),
            ('slab without counters', mk(sp, ksplit=2, counters=False))]


def ints(rng, shape, lim):
    return rng.integers(-lim, lim + 1, shape).astype(F32)


def sconv_inputs(c, kind):
    """Operands of a case: x (forward: [B][Cin][2T]; input gradient: dy [B][Cin][T]), w [ks][Cin][M], bias, bn_scale, bn_shift [M],
    the power-of-two scales sx, sw."""
    rng = np.random.default_rng(seed_of(c['B'], c['T'], c['Cin'], c['M'], c['ks'], c['pad_left'], c['dgrad'], kind))
    B, T, Cin, M, ks = c['B'], c['T'], c['Cin'], c['M'], c['ks']
    L = T if c['dgrad'] else 2 * T
    if kind == 'ints':
        return dict(x=ints(rng, (B, Cin, L), 4), w=ints(rng, (ks, Cin, M), 2), bias=ints(rng, M, 8),
                    bn_scale=rng.choice(F32([1, -1, 2, -2, 0.5, -0.5]), M).astype(F32), bn_shift=ints(rng, M, 8), sx=4.0, sw=8.0)
    g = lambda *s: rng.standard_normal(s).astype(F32)  # noqa: E731
    x = g(B, Cin, L) * F32(1e-4) if c['dgrad'] else g(B, Cin, L)
    return dict(x=x.astype(F32), w=(g(ks, Cin, M) * F32((ks * Cin) ** -0.5)).astype(F32), bias=g(M) * F32(0.5), bn_scale=g(M),
                bn_shift=g(M) * F32(0.3), sx=2.0 ** 22 if c['dgrad'] else 8.0, sw=256.0)


def options(name):
    n, bias, bn, relu, save_r = next(o for o in OPTION_SETS if o[0] == name)
    return dict(name=n, bias=bias, bn=bn, relu=relu, save_r=save_r)


def sliced(c, ins, msel):
    """The case and its operands with only the output channels msel (every output channel is a contraction of its own)."""
    out = dict(ins, w=np.ascontiguousarray(ins['w'][:, :, msel]))
    for k in ('bias', 'bn_scale', 'bn_shift'):
        out[k] = ins[k][msel]
    return dict(c, M=len(msel)), out


def reference(c, ins, opts=None, split=X.split, kmask=None, wrong=None):
    """forward: (out, save_r, bar_out, bar_r, abs_sum); input gradient: (dx, bar, abs_sum)."""
    if c['dgrad']:
        return sconv_dgrad(ins['x'], ins['w'], c['pad_left'], ins['sx'], ins['sw'], split, kmask, wrong, full=True)
    return sconv_fwd(ins['x'], ins['w'], ins['bias'] if opts['bias'] else None, ins['bn_scale'] if opts['bn'] else None,
                     ins['bn_shift'] if opts['bn'] else None, opts['relu'], c['pad_left'], ins['sx'], ins['sw'], split, kmask, wrong, full=True)


# weight gradient
WG_C = 256
WG_TAPS = ((5, 1), (5, 2), (2, 0), (3, 1), (4, 1), (8, 3))
WG_BT = ((1, 4), (3, 36), (3, 104), (2, 128))
WG_LDDW = WG_C + 8
WG_TOTAL_COLS = (64, 200)


def wgrad_cases():
    """(ks, pad_left) x (B, T) x Tp in (2T, 2T - 1); form (b) (both operands as planes) exists where Tp = 2T."""
    return [dict(name='wgrad-k%d-p%d-B%d-T%d-Tp%d' % (ks, pl, B, T, Tp), ks=ks, pad_left=pl, B=B, T=T, Tp=Tp)
            for (ks, pl) in WG_TAPS for (B, T) in WG_BT for Tp in (2 * T, 2 * T - 1)]


def wgrad_inputs(c, kind):
    rng = np.random.default_rng(seed_of('wgrad', c['ks'], c['pad_left'], c['B'], c['T'], c['Tp'], kind))
    B, T, Tp, ks, C = c['B'], c['T'], c['Tp'], c['ks'], WG_C
    if kind == 'ints':
        return dict(p=ints(rng, (B, C, Tp), 4), q=ints(rng, (B, C, T), 2), dw0=ints(rng, (ks, C, C), 8), total0=ints(rng, C, 8), sp=4.0, sq=8.0)
    g = lambda *s: rng.standard_normal(s).astype(F32)  # noqa: E731
    return dict(p=g(B, C, Tp), q=(g(B, C, T) * F32(1e-4)).astype(F32), dw0=(g(ks, C, C) * F32(1e-4)).astype(F32),
                total0=(g(C) * F32(1e-3)).astype(F32), sp=4.0, sq=2.0 ** 22)


def wgrad_taps(c):
    return [j - c['pad_left'] for j in range(c['ks'])]


# ---------------------------------------------------------------------------------------------------- fp32 emulations
def _seq(acc, terms):
    for t in terms:
        acc = (acc + t).astype(F32)
    return acc


def emulate_sconv(c, ins, opts, S=1, msel=None):
    """The same sums as sconv_fwd / sconv_dgrad step by step in fp32: products of fp16 planes (exact in fp32) added one at a time in
    (tap, channel, term) order -- per split first, the partial sums then added in split order --, then the epilogue in fp32.
    Only the output channels msel are evaluated.  Returns (out, save_r) / dx as float32."""
    ks, C, T, B = c['ks'], c['Cin'], c['T'], c['B']
    msel = np.arange(c['M']) if msel is None else msel
    sx, sw = ins['sx'], ins['sw']
    w1, w2 = (h.astype(F32)[:, :, msel] for h in X.split(X.scaled(ins['w'], sw)))
    x1, x2 = (h.astype(np.float64) for h in X.split(X.scaled(ins['x'], sx)))
    if c['dgrad']:
        u = np.arange(2 * T)
        num = [u + c['pad_left'] - j for j in range(ks)]
        ops = [tuple(_gather(h, np.where(n % 2 == 0, n // 2, -(10 ** 9))).astype(F32) for h in (x1, x2)) for n in num]
        N = 2 * T
    else:
        a1, a2 = fwd_operands(x1, x2, ks, c['pad_left'], T)
        ops = [(a1[:, j * C:(j + 1) * C].astype(F32), a2[:, j * C:(j + 1) * C].astype(F32)) for j in range(ks)]
        N = T
    total = np.zeros((B, len(msel), N), F32)
    for part in range(S):
        mask = split_kmask(c, S, part) if S > 1 else kmask_all(ks, C)
        acc = np.zeros((B, len(msel), N), F32)
        for j in range(ks):
            for ch in np.flatnonzero(mask[j]):
                xa, xb = ops[j][0][:, ch, None, :], ops[j][1][:, ch, None, :]
                wa, wb = w1[j, ch][None, :, None], w2[j, ch][None, :, None]
                acc = _seq(acc, (xa * wb, xb * wa, xa * wa))
        total = acc if S == 1 else (total + acc).astype(F32)
    y = (total * F32(_inv(sx, sw))).astype(F32)
    return y if c['dgrad'] or opts is None else emulate_epilogue(y, ins, opts, msel)


def emulate_epilogue(y, ins, opts, msel):
    """bias -> relu -> BatchNorm affine in fp32, every product and sum rounded on its own; returns (out, save_r)."""
    col = lambda v: np.asarray(v, F32)[msel][None, :, None]  # noqa: E731
    if opts['bias']:
        y = (y + col(ins['bias'])).astype(F32)
    if opts['relu']:
        y = np.maximum(y, F32(0))
    out = y
    if opts['bn']:
        out = ((col(ins['bn_scale']) * y).astype(F32) + col(ins['bn_shift'])).astype(F32)
    return out, y


def emulate_wgrad(c, ins, csel, osel):
    """dw0 + the weight gradient summed one (b, t) at a time in fp32, for the channels csel x osel."""
    B, T, Tp = c['B'], c['T'], c['Tp']
    p1, p2 = (h.astype(np.float64) for h in X.split(X.scaled(ins['p'], ins['sp'])))
    q1, q2 = (h.astype(F32)[:, osel] for h in X.split(X.scaled(ins['q'], ins['sq'])))
    t = np.arange(T)
    acc = np.zeros((c['ks'], len(csel), len(osel)), F32)
    g = [tuple(_gather(h[:, csel], 2 * t + sh).astype(F32) for h in (p1, p2)) for sh in wgrad_taps(c)]
    for b in range(B):
        for tt in range(T):
            a1 = np.stack([gj[0][b, :, tt] for gj in g])[:, :, None]
            a2 = np.stack([gj[1][b, :, tt] for gj in g])[:, :, None]
            acc = _seq(acc, (a1 * q2[b, :, tt][None, None, :], a2 * q1[b, :, tt][None, None, :], a1 * q1[b, :, tt][None, None, :]))
    upd = (acc * F32(_inv(ins['sp'], ins['sq']))).astype(F32)
    return (ins['dw0'][:, csel][:, :, osel] + upd).astype(F32)
