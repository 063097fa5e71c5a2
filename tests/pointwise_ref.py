"""Float64 references of the HBM-bound kernels (csrc/pointwise.hip), their seeded case tables and their bars, for
tests/test_pointwise_ref_cpu.py and tests/test_pointwise_kernels_gpu.py.

Everything here is numpy on the CPU, written from the formulas of include/vqwave.h and not from the kernels.  Every output and
every in-place operand of a GPU case is a view into a sentinel-filled buffer (conv_ref.Buf); compare() holds the written
region to the case's bar and everything else -- guard bands, what lies beyond an output's extent -- to bit-equality.

Three kinds of expectation:

 (a) 'bits': bit-exact by construction: transpose, the dz of bn_relu_bwd (one fp32 multiply and a mask), the r of relu_bn_fwd,
     the labels of wavenet_inputs, whatever a device skip != 0 must leave alone.
 (b) 'ints': exact-integer inputs for every kernel that sums.  Operands are integers of |value| <= 4 held in fp32; alpha,
     scale, shift and the accumulators' initial contents are integers or halves.  Every partial sum in every order is then a
     multiple of 1/2 below 2^23: fp32 addition, FMA and atomics are exact, and the device must equal the reference BIT FOR BIT
     whatever its reduction order.  (The CPU test asserts 2 * sum |terms| < 2^24 for every case.)
 (c) 'normal': standard-normal inputs and elementwise bars that are formulas in U = 2^-24, not fractions of the tensor maximum:
       a sum of n terms                      n * U * sum |terms|            (any order; + U * sum |terms| per fp32 rounding
                                                                             of a term before it is summed: a product, alpha)
       relu_bn_fwd x                         3U * (|scale * r| + |shift|)   (the product may or may not be contracted)
       softmax p                             U * (16 + 2 sqrt(Q) + 4 |v - M|) * p + 2^-126   (|v - M|: the rounding of the
                                                                             fast exponential's argument scaling; sqrt(Q): the
                                                                             random walk of a fp32 sum of Q terms)
       dlogits                               |grad_scale| * (bar(p) + 2U * |p - onehot|)
       per-position loss                     2U * (4 + |M| + |x_label| + |loss|)
       loss_sum                              the sum of the positions' bars + the any-order bound over the positions
       Adam                                  atol = rtol = 1e-6 against clip_ref.adam_ema_step (tests/test_clip_gpu.py)
     The bars are set against the reference, never against the kernel: the CPU test evaluates each with a step-by-step fp32
     numpy emulation of the formula and asserts that it stays at or under EMU_FRACTION of the bar on every case.
     Four constants were moved because the EMULATION did not fit, none because a kernel failed.  Sums: the any-order bound
     (n - 1) * U * sum |terms| is attained at n = 2 (one addition of two terms of one sign, a tie), so it cannot leave the
     emulation a quarter of the bar; n * U * sum |terms| does.  Softmax p: with the constant 16 alone the sequential fp32 sum of
     Q = 256 and 512 terms put the emulation at up to 1.39 bars (22 U relative on one of 1e5 probabilities); 2 sqrt(Q) is the
     growth of that sum's rounding error.  relu_bn_fwd x: the uncontracted form rounds twice, 2U |scale * r| + U |shift| at
     worst, which is the whole of a 2U bar where shift is small (0.84 of it over 528 000 elements); 3U.  The dlogits bar
     carries 2U * |p - onehot| beside the probability bar: at the label the fp32 subtraction p - 1 rounds to 2^-25 whatever p
     is, which |grad_scale| * bar(p) alone cannot hold once p < 1/32 (the emulation exceeds it there by orders of magnitude);
     the two extra roundings are the subtraction and the product with grad_scale.

A written zero is compared by value: a sum that comes to zero has no promised sign (0 + -0 and -0 + -0 differ)."""
import zlib

import numpy as np

import clip_ref
from conv_ref import GUARD, SENTINEL, Buf, randn, same_pads, with_zeros  # noqa: F401  (re-exported to the two test files)

U = 2.0 ** -24
TINY = 2.0 ** -126
EMU_FRACTION = 0.75
F32 = np.float32


def seed_of(*parts):
    return zlib.crc32(repr(parts).encode()) & 0x7fffffff


def ints(seed, *shape, lim=4):
    """Integers of |value| <= lim held in fp32."""
    return np.random.RandomState(seed).randint(-lim, lim + 1, shape).astype(F32)


def halves(seed, *shape, lim=4):
    """Multiples of 1/2 of |value| <= lim held in fp32."""
    return (np.random.RandomState(seed).randint(-2 * lim, 2 * lim + 1, shape) / 2.0).astype(F32)


def operand(kind, seed, *shape):
    return ints(seed, *shape) if kind == 'ints' else randn(seed, *shape)


def coeff(kind, seed, *shape):
    """scale / shift / bias / initial accumulator contents."""
    return halves(seed, *shape) if kind == 'ints' else randn(seed, *shape)


def _f64(a):
    return np.asarray(a, dtype=np.float64)


# ---------------------------------------------------------------------------------------------------- comparison
def compare(got, buf, vals, bar, mask=None, what=''):
    """got: the WHOLE fp32 buffer read back; buf: the conv_ref.Buf as it was before the launch; vals: float64 reference of the
    view; mask: the view's written positions (default: all); bar: None = the written region equals fp32(vals) bit for bit, else
    a scalar or an array over the view of elementwise bounds.  Everything not written must be bit-equal to buf.  Returns the
    worst err / bar (0.0 for a bit-exact comparison)."""
    vals = _f64(vals).reshape(-1)
    mask = np.ones(buf.n, dtype=bool) if mask is None else np.asarray(mask, dtype=bool).reshape(-1)
    full = buf.view.astype(np.float64)
    full[mask] = vals[mask]
    ref, keep = buf.expected(full, mask)
    g = np.asarray(got).reshape(-1)
    assert g.dtype == np.float32 and g.size == ref.size, '%s: buffer sizes differ' % what
    same = g[keep].view(np.uint32) == ref[keep].astype(F32).view(np.uint32)
    assert same.all(), '%s: %d of %d positions the kernel must not touch changed (first: element %d, %r -> %r)' % (
        what, int((~same).sum()), int(keep.sum()), int(np.flatnonzero(keep)[np.argmin(same)]) - buf.lo,
        float(ref[keep][np.argmin(same)]), float(g[keep][np.argmin(same)]))
    gw, rw = g[~keep], ref[~keep]
    if bar is None:
        eq = (gw.view(np.uint32) == rw.astype(F32).view(np.uint32)) | ((gw == 0) & (rw == 0))      # a zero sum has no promised sign
        assert eq.all(), '%s: %d of %d written elements are not bit-equal to the reference (first: element %d, got %r, want %r)' % (
            what, int((~eq).sum()), eq.size, int(np.flatnonzero(mask)[np.argmin(eq)]), float(gw[np.argmin(eq)]), float(rw[np.argmin(eq)]))
        return 0.0
    b = np.broadcast_to(_f64(bar).reshape(-1) if np.ndim(bar) else _f64(bar), (buf.n,))[mask]
    return ratio_of(gw, rw, b, what, np.flatnonzero(mask))


def ratio_of(got, ref, bar, what='', index=None):
    """max |got - ref| / bar, asserted <= 1 (an exact element passes a zero bar)."""
    got, ref, bar = _f64(got).reshape(-1), _f64(ref).reshape(-1), np.broadcast_to(_f64(bar), np.shape(ref)).reshape(-1)
    d = np.abs(got - ref)
    d = np.where(np.isfinite(d), d, np.inf)
    with np.errstate(divide='ignore', invalid='ignore'):
        q = np.where(d == 0.0, 0.0, d / bar)
    if q.size == 0:
        return 0.0
    i = int(np.argmax(q))
    assert q[i] <= 1.0, '%s: err %.3e > bar %.3e (%.2f bars) at element %d: got %r, want %r' % (
        what, d[i], bar[i], q[i], i if index is None else int(index[i]), float(got[i]), float(ref[i]))
    return float(q[i])


# ---------------------------------------------------------------------------------------------------- softmax cross-entropy
SOFTMAX_Q = (4, 8, 64, 68, 100, 256, 512)            # channels per wave 1, 2, 16, 17, 25, 64, 128: tail, chunks, chunks + tail
SOFTMAX_T = (1, 63, 64, 65, 200)
SOFTMAX_SETS = ('normal', 'equal', 'shift', 'wide0', 'wide1', 'wide2', 'wide3')
SOFTMAX_LOSS0 = 3.25                                  # loss_sum starts from it


def softmax_cases():
    out = []
    for i, Q in enumerate(SOFTMAX_Q):
        for j, T in enumerate(SOFTMAX_T):
            out.append(dict(Q=Q, T=T, B=(1, 3)[(i + j) & 1], logits='normal', gs=('quarter', 'mean')[j & 1]))
        for s, kind in enumerate(SOFTMAX_SETS[1:]):
            out.append(dict(Q=Q, T=SOFTMAX_T[(i + s) % 5], B=(3, 1)[(i + s) & 1], logits=kind, gs=('mean', 'quarter')[s & 1]))
    for c in out:
        c['name'] = '%s_q%d_t%d_b%d_%s' % (c['logits'], c['Q'], c['T'], c['B'], c['gs'])
        c['grad_scale'] = float(F32(0.25 if c['gs'] == 'quarter' else 1.0 / (c['B'] * c['T'])))
    return out


def softmax_legal(c):
    return c['B'] > 0 and c['T'] > 0 and c['Q'] >= 4 and c['Q'] % 4 == 0


def softmax_paths(c):
    """The kernel's channel loops a case runs: 16-channel chunks and / or the per-channel tail, and a partial 64-step tile."""
    qn = c['Q'] // 4
    return {'chunks': qn >= 16, 'tail': qn % 16 != 0, 'partial_tile': c['T'] % 64 != 0, 'full_tile': c['T'] >= 64}


def boundary_labels(Q):
    """Each wave's first and last channel and both sides of every 16-channel chunk boundary inside a wave."""
    qn, out = Q // 4, []
    for w in range(4):
        out += [w * qn, (w + 1) * qn - 1]
        for e in range(16, qn, 16):
            out += [w * qn + e - 1, w * qn + e]
    return sorted(set(out))


def softmax_inputs(c):
    B, Q, T, kind = c['B'], c['Q'], c['T'], c['logits']
    sd = seed_of('softmax', c['name'])
    if kind == 'equal':
        x = np.full((B, Q, T), 1.5, dtype=F32)
    else:
        x = randn(sd, B, Q, T) * F32(3.0)
        if kind == 'shift':
            x = x + F32(1e4)
        elif kind.startswith('wide'):                  # wave w's channels sit 150 above the rest: the others' sums underflow in the merge
            w, qn = int(kind[4:]), Q // 4
            x = x - F32(75.0)
            x[:, w * qn:(w + 1) * qn, :] += F32(150.0)
    lab = np.random.RandomState(sd + 1).randint(0, Q, (B, T)).astype(np.int32)
    bl = boundary_labels(Q)
    flat = lab.reshape(-1)
    n = min(flat.size, len(bl))
    rot = sd % len(bl)
    flat[:n] = [bl[(rot + i) % len(bl)] for i in range(n)]
    return np.ascontiguousarray(x, dtype=F32), lab


def softmax_ref(logits, labels):
    """float64: p [B][Q][T], per-position M, x_label and loss [B][T]."""
    x = _f64(logits)
    M = x.max(1)
    e = np.exp(x - M[:, None, :])
    S = e.sum(1)
    xl = np.take_along_axis(x, labels[:, None, :].astype(np.int64), 1)[:, 0, :]
    return dict(p=e / S[:, None, :], M=M, xl=xl, loss=np.log(S) + M - xl)


def onehot(labels, Q):
    return (np.arange(Q)[None, :, None] == labels[:, None, :]).astype(np.float64)


def softmax_bars(logits, labels, ref, grad_scale):
    x = _f64(logits)
    bp = U * (16.0 + 2.0 * np.sqrt(x.shape[1]) + 4.0 * np.abs(x - ref['M'][:, None, :])) * ref['p'] + TINY
    bd = abs(grad_scale) * (bp + 2.0 * U * np.abs(ref['p'] - onehot(labels, x.shape[1])))
    bl = 2.0 * U * (4.0 + np.abs(ref['M']) + np.abs(ref['xl']) + np.abs(ref['loss']))
    bsum = bl.sum() + bl.size * U * (abs(SOFTMAX_LOSS0) + np.abs(ref['loss']).sum())
    return dict(p=bp, dlogits=bd, loss=bl, loss_sum=float(bsum))


def softmax_emulation(logits, labels, grad_scale):
    """Plain fp32, step by step: fp32 maximum, exp2(fl(fl(v - M) * log2 e)), sequential fp32 sum, fp32 reciprocal."""
    x = np.asarray(logits, dtype=F32)
    M = x.max(1)
    a = ((x - M[:, None, :]).astype(F32) * F32(np.log2(np.e))).astype(F32)
    e = np.exp2(a.astype(np.float64)).astype(F32)
    S = np.zeros_like(M)
    for q in range(x.shape[1]):
        S = (S + e[:, q, :]).astype(F32)
    inv = (F32(1.0) / S).astype(F32)
    p = (e * inv[:, None, :]).astype(F32)
    xl = np.take_along_axis(x, labels[:, None, :].astype(np.int64), 1)[:, 0, :]
    loss = ((np.log(S.astype(np.float64)).astype(F32) + M).astype(F32) - xl).astype(F32)
    d = ((p - onehot(labels, x.shape[1]).astype(F32)).astype(F32) * F32(grad_scale)).astype(F32)
    ls = F32(SOFTMAX_LOSS0)
    for v in loss.reshape(-1):
        ls = F32(ls + v)
    return dict(p=p, dlogits=d, loss=loss, loss_sum=float(ls))


# ---------------------------------------------------------------------------------------------------- row sums
def _rs(B, C, T, seg, kernel, xoff=0, yoff=0):
    return dict(name='b%d_c%d_t%d_seg%d%s%s' % (B, C, T, seg, '_xoff' if xoff else '', '_yoff' if yoff else ''),
                B=B, C=C, T=T, seg=seg, xoff=xoff, yoff=yoff, kernel=kernel)


def rowsum_cases():
    """`kernel`: the kernel the case is in the table for, taken by its seg_out variants (its total-only ones when seg == 0)."""
    return [_rs(3, 7, 104, 8, 'fast'), _rs(3, 7, 256, 4, 'fast'), _rs(3, 7, 256, 64, 'fast'), _rs(3, 7, 256, 256, 'fast'),
            _rs(2, 5, 1028, 4, 'fast'), _rs(1, 1, 832, 0, 'fast'),
            _rs(3, 7, 37, 0, 'general'), _rs(3, 7, 37, 37, 'general'), _rs(2, 5, 120, 12, 'general'), _rs(2, 5, 120, 2, 'general'),
            _rs(2, 5, 120, 1, 'general'), _rs(1, 3, 1040, 520, 'general'), _rs(1, 1, 833, 0, 'general'),
            _rs(3, 7, 104, 8, 'general', xoff=1), _rs(3, 7, 104, 8, 'general', yoff=1)]


ROWSUM_ALPHAS = (1.0, 0.5, -2.0)


def rowsum_variants(c):
    """(with_y, with_seg, with_total, alpha): with and without y; seg_out only, total only, both; every alpha in each case."""
    if c['seg'] == 0:
        return [(wy, False, True, a) for wy in (False, True) for a in ROWSUM_ALPHAS]
    v = [(wy, ws, wt) for wy in (False, True) for ws, wt in ((True, False), (False, True), (True, True))]
    return [(wy, ws, wt, ROWSUM_ALPHAS[(i + (i // 3)) % 3]) for i, (wy, ws, wt) in enumerate(v)]


def rowsum_legal(c, with_seg):
    return c['B'] > 0 and c['C'] > 0 and c['T'] > 0 and (not with_seg or (c['seg'] >= 1 and c['T'] % c['seg'] == 0))


def rowsum_kernel(c, with_y, with_seg):
    """vqw_rowsum's dispatch, restated: the fast kernel needs 16-byte aligned x (and y), T % 4 == 0 and, for seg_out, a segment
    of four times a power of two, at most 256."""
    aligned = c['xoff'] == 0 and (not with_y or c['yoff'] == 0)
    lps = c['seg'] // 4 if (with_seg and c['seg'] % 4 == 0) else 0
    ok_seg = (not with_seg) or (1 <= lps <= 64 and lps & (lps - 1) == 0)
    return 'fast' if (aligned and c['T'] % 4 == 0 and ok_seg) else 'general'


def rowsum_inputs(c, kind):
    sd = seed_of('rowsum', c['name'], kind)
    sh = (c['B'], c['C'], c['T'])
    return dict(x=operand(kind, sd, *sh), y=operand(kind, sd + 1, *sh), total0=coeff(kind, sd + 2, c['C']))


def rowsum_ref(c, ins, with_y, alpha):
    """-> seg [B][C][T/seg] (None when seg == 0), total [C], and their bars (sum-of-|terms| form, see the module docstring)."""
    B, C, T, seg = c['B'], c['C'], c['T'], c['seg']
    t = _f64(ins['x']) * (_f64(ins['y']) if with_y else 1.0)
    a, r = np.abs(t), int(with_y)
    out = dict(seg=None, seg_bar=None, seg_abs=None)
    if seg > 0:
        out['seg'] = t.reshape(B, C, T // seg, seg).sum(-1)
        out['seg_abs'] = a.reshape(B, C, T // seg, seg).sum(-1)
        out['seg_bar'] = (seg + r) * U * out['seg_abs']
    out['total'] = _f64(ins['total0']) + alpha * t.sum((0, 2))
    out['total_abs'] = np.abs(_f64(ins['total0'])) + abs(alpha) * a.sum((0, 2))
    out['total_bar'] = (B * T + 1 + r + 1) * U * out['total_abs']    # B*T + 1 terms; a product and alpha round once more each
    return out


# ---------------------------------------------------------------------------------------------------- transpose
TRANSPOSE_CASES = ((1, 1, 1), (3, 31, 33), (2, 32, 32), (5, 1, 100), (1, 100, 1), (4, 65, 96))


def transpose_ref(src, batch, rows, cols):
    return np.ascontiguousarray(np.asarray(src).reshape(batch, rows, cols).transpose(0, 2, 1))


# ---------------------------------------------------------------------------------------------------- relu / BatchNorm passes
BN_SHAPES = ((3, 5, 37), (2, 40, 6600))         # the second: 528 000 elements, a second trip of the grid-stride loop (2048 x 256)
GRID_STRIDE_ELEMENTS = 2048 * 256


def bn_relu_bwd_ref(dx, r, scale):
    """dz = dx * scale[c] * (r > 0): ONE fp32 multiply and a mask, hence fp32 here too (bit-exact)."""
    v = (np.asarray(dx, F32) * np.asarray(scale, F32)[None, :, None]).astype(F32)
    return v if r is None else np.where(np.asarray(r) > 0, v, F32(0.0)).astype(F32)


def relu_bn_fwd_ref(x, scale, shift):
    """-> r (fp32, bit-exact), x_new (float64), bar of x_new (None without scale: x_new = r, bit-exact)."""
    r = np.where(np.asarray(x) > 0, np.asarray(x, F32), F32(0.0)).astype(F32)
    if scale is None:
        return r, _f64(r), None
    sr = _f64(scale)[None, :, None] * _f64(r)
    sh = np.broadcast_to(_f64(shift)[None, :, None], sr.shape)
    return r, sr + sh, 3.0 * U * (np.abs(sr) + np.abs(sh))


def relu_bn_fwd_emulation(x, scale, shift):
    r = np.maximum(np.asarray(x, F32), F32(0.0))
    return ((np.asarray(scale, F32)[None, :, None] * r).astype(F32) + np.asarray(shift, F32)[None, :, None]).astype(F32)


BN_SUMS_T = (4, 37, 256, 260, 1028)
BN_SUMS_BC = (3, 7)
BN_SUMS_FORMS = ('r_is_y', 'distinct', 'r_null')
BN_SUMS_DROP = (None, 'dscale', 'dbeta', 'dbias')


def bn_sums_inputs(T, kind):
    B, C = BN_SUMS_BC
    sd = seed_of('bn_sums', T, kind)
    ins = dict(dx=operand(kind, sd, B, C, T), y=with_zeros(operand(kind, sd + 1, B, C, T), sd + 2),
               r=with_zeros(operand(kind, sd + 3, B, C, T), sd + 4), scale=coeff(kind, sd + 5, C))
    for i, n in enumerate(('dscale', 'dbeta', 'dbias')):
        ins[n + '0'] = coeff(kind, sd + 6 + i, C)
    return ins


def bn_sums_ref(ins, form):
    """-> dz (fp32, bit-exact), the three sums (float64, on their initial contents), sum |terms| and the (c) bars."""
    dx, y = _f64(ins['dx']), _f64(ins['y'])
    r = dict(r_is_y=ins['y'], distinct=ins['r'], r_null=None)[form]
    dz = bn_relu_bwd_ref(ins['dx'], r, ins['scale'])
    n = dx.shape[0] * dx.shape[2] + 1
    out = dict(dz=dz)
    for name, t, rounded in (('dscale', dx * y, 1), ('dbeta', dx, 0), ('dbias', _f64(dz), 0)):
        out[name] = _f64(ins[name + '0']) + t.sum((0, 2))
        out[name + '_abs'] = np.abs(_f64(ins[name + '0'])) + np.abs(t).sum((0, 2))
        out[name + '_bar'] = (n + rounded) * U * out[name + '_abs']
    return out


# ---------------------------------------------------------------------------------------------------- Cin == 1 convolutions
def _cc(k, stride, T_out, F, B, pad, bias=True):
    return dict(name='k%d_s%d_t%d_f%d_b%d_%s%s' % (k, stride, T_out, F, B, pad, '' if bias else '_nobias'),
                k=k, stride=stride, T_out=T_out, F=F, B=B, pad=pad, bias=bias)


def conv_cin1_cases():
    """Every (k, stride) with a ragged and a multiple-of-4 length; pad: 'causal' = -(k-1), 'same' = Keras SAME, 'plus2' = +2
    (the window runs past T_in)."""
    return [_cc(5, 2, 37, 17, 3, 'same'), _cc(5, 2, 1024, 40, 1, 'same', bias=False), _cc(5, 2, 2052, 16, 1, 'plus2'),
            _cc(3, 1, 3, 1, 3, 'causal', bias=False), _cc(3, 1, 1028, 16, 1, 'plus2'),
            _cc(8, 1, 1, 17, 1, 'causal'), _cc(8, 1, 2052, 40, 3, 'plus2', bias=False),
            _cc(5, 3, 37, 40, 1, 'plus2'), _cc(5, 3, 1028, 17, 3, 'causal'),
            _cc(8, 4, 1025, 16, 3, 'same'), _cc(8, 4, 1024, 1, 1, 'causal', bias=False),
            _cc(32, 1, 1025, 40, 1, 'causal'), _cc(32, 1, 2052, 16, 3, 'causal', bias=False), _cc(32, 1, 4, 17, 1, 'plus2'),
            _cc(9, 1, 37, 1, 3, 'same'), _cc(9, 1, 1028, 17, 1, 'causal', bias=False),
            _cc(9, 2, 3, 16, 1, 'same', bias=False), _cc(9, 2, 1024, 17, 3, 'same'),
            _cc(32, 4, 1025, 17, 1, 'same', bias=False), _cc(32, 4, 2052, 1, 3, 'causal'), _cc(32, 4, 4, 40, 1, 'plus2')]


def conv_cin1_geometry(c):
    """-> T_in, offset."""
    if c['pad'] == 'same':
        T_in = c['stride'] * c['T_out']
        return T_in, -same_pads(T_in, c['k'], c['stride'])[0]
    T_in = c['stride'] * c['T_out'] + 1
    return T_in, (-(c['k'] - 1) if c['pad'] == 'causal' else 2)


def conv_cin1_instance(c):
    """(KMAX, STRIDE) of the template instance both entries pick: the window lives in registers (compile-time stride) for
    stride 1, and for stride 2 with k <= 8; everything else reads it tap by tap (STRIDE 0)."""
    kmax = 8 if c['k'] <= 8 else 32
    return kmax, (2 if (kmax == 8 and c['stride'] == 2) else (1 if c['stride'] == 1 else 0))


CONV_CIN1_INSTANCES = ((8, 2), (8, 1), (8, 0), (32, 1), (32, 0))
CONV_CIN1_OPTIONS = tuple((relu, scale, save) for relu in (False, True) for scale in (False, True) for save in (False, True))


def conv_cin1_legal(c):
    return c['B'] > 0 and c['T_out'] > 0 and c['F'] > 0 and 1 <= c['k'] <= 32 and 1 <= c['stride'] <= 4 and c['B'] <= 65535


def conv_cin1_out_off(c):
    """Rows of T_out % 4 == 0 need 16-byte aligned out / save_r / dout; ragged ones are given a start one float past."""
    return 0 if c['T_out'] % 4 == 0 else 1


def conv_cin1_inputs(c, kind):
    sd = seed_of('conv_cin1', c['name'], kind)
    T_in, _ = conv_cin1_geometry(c)
    B, F, k, To = c['B'], c['F'], c['k'], c['T_out']
    return dict(x=operand(kind, sd, B, T_in), w=operand(kind, sd + 1, k, F), bias=coeff(kind, sd + 2, F) if c['bias'] else None,
                scale=coeff(kind, sd + 3, F), shift=coeff(kind, sd + 4, F), dout=operand(kind, sd + 5, B, F, To),
                dw0=coeff(kind, sd + 6, k, F))


def _windows(c, x):
    """x[b][stride*t + j + offset] as [B][T_out][k], zero outside [0, T_in)."""
    T_in, off = conv_cin1_geometry(c)
    idx = c['stride'] * np.arange(c['T_out'])[:, None] + np.arange(c['k'])[None, :] + off
    ok = (idx >= 0) & (idx < T_in)
    return np.where(ok[None], _f64(x)[:, np.clip(idx, 0, T_in - 1)], 0.0)


def conv_cin1_fwd_ref(c, ins, relu, scale):
    """-> r, out (float64 [B][F][T_out]), their bars, sum |terms| of out."""
    xg, w = _windows(c, ins['x']), _f64(ins['w'])
    b = np.zeros(c['F']) if ins['bias'] is None else _f64(ins['bias'])
    v = np.einsum('btk,kf->bft', xg, w) + b[None, :, None]
    va = np.einsum('btk,kf->bft', np.abs(xg), np.abs(w)) + np.abs(b)[None, :, None]
    vbar = (c['k'] + 1) * U * va                          # k + 1 terms
    r = np.maximum(v, 0.0) if relu else v
    if not scale:
        return dict(r=r, out=r, r_bar=vbar, out_bar=vbar, out_abs=va)
    sc, sh = _f64(ins['scale'])[None, :, None], _f64(ins['shift'])[None, :, None]
    return dict(r=r, out=sc * r + sh, r_bar=vbar, out_bar=np.abs(sc) * vbar + 2.0 * U * (np.abs(sc * r) + np.abs(sh)),
                out_abs=np.abs(sc) * va + np.abs(sh))


def conv_cin1_wgrad_ref(c, ins):
    xg, d = _windows(c, ins['x']), _f64(ins['dout'])
    dw = _f64(ins['dw0']) + np.einsum('btk,bft->kf', xg, d)
    a = np.abs(_f64(ins['dw0'])) + np.einsum('btk,bft->kf', np.abs(xg), np.abs(d))
    return dict(dw=dw, dw_abs=a, dw_bar=(c['B'] * c['T_out'] + 1) * U * a)         # B * T_out + 1 terms


def conv_cin1_fwd_emulation(c, ins):
    """fp32, tap by tap from the bias, product and sum rounded separately."""
    xg = _windows(c, ins['x']).astype(F32)
    acc = np.zeros((c['B'], c['F'], c['T_out']), F32) + (F32(0) if ins['bias'] is None else ins['bias'][None, :, None])
    for j in range(c['k']):
        acc = (acc + (xg[:, None, :, j] * ins['w'][j][None, :, None]).astype(F32)).astype(F32)
    return acc


# ---------------------------------------------------------------------------------------------------- sums, emulated
def sequential_sum_f32(terms):
    """fp32 sum of the rows of `terms` [n][...] taken one after another (each term rounded to fp32 first)."""
    acc = np.zeros(np.shape(terms)[1:], F32)
    for t in terms:
        acc = (acc + np.asarray(t, np.float64).astype(F32)).astype(F32)
    return acc


# ---------------------------------------------------------------------------------------------------- Adam + EMA
ADAM_N = (1, 3, 4, 5, 1003, 2097157)             # the last: n4 > 2048 * 256, a second trip of the vector loop, with a tail
ADAM_ALIGN = {'aligned': (0, 0, 0, 0, 0), 'all_shifted': (1, 1, 1, 1, 1), 'grad_shifted': (0, 1, 0, 0, 0)}   # param grad m v ema
ADAM_FORMS = ('plain', 'skip0', 'skip1', 'scaled')
ADAM_LR_T = (1e-3, 7e-4)
ADAM_GRAD_SCALE, ADAM_SCALE = 0.5, 0.25
ADAM_TOL = 1e-6


def adam_path(n, align):
    """vqw_adam_ema_step*: 16-byte vectors need all five buffers aligned; n4 = n / 4 vectors then, and a scalar tail."""
    vec = not any(ADAM_ALIGN[align])
    n4 = n // 4 if vec else 0
    return dict(vector=n4 > 0, tail=n > 4 * n4, second_trip=n4 > GRID_STRIDE_ELEMENTS)


def adam_inputs(n):
    """The slots start where one Adam step on a gradient g0 leaves them, m = (1 - b1) g0 and v = (1 - b2) g0^2, so that they are
    non-zero and |m| / sqrt(v) is bounded as in every real run.  (Independent m and v are not a state Adam reaches: among 2e6
    elements some v is ~1e-9 beside m ~0.1, the step lr_t * m / sqrt(v) is of order 1, and the fp32 rounding of 1 - beta2,
    1.3e-5 relative, which the float64 reference does not share, shows in p at 4e-6.)"""
    rng = np.random.default_rng(seed_of('adam', n))
    g = lambda: rng.standard_normal(n).astype(F32)  # noqa: E731
    g0 = g()
    return dict(p=g(), ema=g(), m=g0 * F32(0.1), v=np.square(g0) * F32(0.001), grads=[g(), g()])


def adam_ref(ins, form):
    """Two steps -> (p, m, v, ema) float64; skip1 leaves everything as it was."""
    st = tuple(_f64(ins[n]) for n in ('p', 'm', 'v', 'ema'))
    if form == 'skip1':
        return st
    for g, lr_t in zip(ins['grads'], ADAM_LR_T):
        p, m, v, ema = clip_ref.adam_ema_step(st[0], g, st[1], st[2], st[3], lr_t=lr_t, grad_scale=ADAM_GRAD_SCALE,
                                              scale=ADAM_SCALE if form == 'scaled' else 1.0)
        st = (p, m, v, ema)
    return st


# ---------------------------------------------------------------------------------------------------- wavenet_inputs
WAVENET_INPUTS_BT = ((1, 1), (3, 5), (2, 262200))          # the last: 524 400 positions, a second grid-stride trip
WAVENET_INPUTS_ATOL = 3e-7


def wavenet_inputs_ref(x):
    """labels (the fp32 formula of mu_law_ops.py:11, bit-exact) and inputs = mu-law of x shifted right by one (fp32)."""
    from oracle import ref_ops as R
    x = np.asarray(x, F32)
    sh = np.concatenate([np.zeros((x.shape[0], 1), F32), x[:, :-1]], 1)
    return R.mu_law_encode_np(x, to_int=True).astype(np.int32), R.mu_law_encode_np(sh).astype(F32)
