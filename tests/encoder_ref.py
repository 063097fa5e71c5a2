"""Encoder_64 layer by layer in float64, for tests/test_encoder_ref_cpu.py and tests/test_encoder_routes_gpu.py: what every route of
Encoder64.forward / backward (fp16x3 engine, split-K, fused epilogue; planes-both, p_stride = 2 and fp32 weight gradients; the bias
gradient from q_total or from the BatchNorm pass) has to compute, whichever kernels carry it.

numpy only, no GPU.  Written from oracle/ref_model.py:encoder_64 and oracle/ref_ops.py (keras_conv1d, same_pads,
batch_norm_inference), not from the package: a k = 5 stride-2 SAME conv from the one audio channel, five F -> F, a 1x1 to latent_dim,
each followed by relu (not the last) and the inference-mode BatchNorm affine with eps = 1e-3.  Tensors are [B][C][T], kernels
[k][Cin][Cout] as the reference names them.

Every contraction takes an operand scale per side.  With scales (powers of two) it is evaluated plane-exactly as tests/sconv_ref.py
does: both operands scaled, split into the two fp16 planes of tests/x3_ref.py, a product a1 b1 + a1 b2 + a2 b1 summed in float64 and
divided by the scales.  Without, it is the plain float64 sum over the values given.  Every contraction returns abs_sum beside its
value: the sum of the absolute values of its addends, which the bars are made of.

Bars, elementwise, U = 2^-24, in the form tests/sconv_ref.py derives (no constant of its own):
    e_acc       = n U abs_sum        n = 3 taps channels on the fp16x3 engine, taps channels on the fp32-MFMA engine (input gradient:
                                     the taps of the element's parity); 3 B T / B T for a weight gradient.  The bound of a recursive
                                     fp32 sum of n terms in ANY order: split-K atomics and the split weight gradient have no other.
    conv        sconv_ref.fwd_epilogue: one U per rounding of bias, affine product and affine sum
    layer 0     tests/pointwise_ref.py's bars of conv_cin1_fwd: (k + 1) U (abs_sum + |bias|), then 2U (|scale r| + |shift|)
    dgrad       e_acc + U (|dx| + e_acc); after the BatchNorm / relu pass (ONE fp32 product and a mask): |scale| bar + U |scale dx|
    dw          e_acc + U P + 2U P, P = |dw| + e_acc                  (sconv_ref's bar of a gradient added onto a zero-filled buffer)
    channel sums (dbias, dbeta, dscale, q_total): (B T + 3) U sum |addend|; where the addends are themselves the outcome of an input
                gradient the device forms (dbeta, dscale), their bars, summed, are added.
    d(conv_6)   dz scale: one fp32 product and no mask, bit for bit (as tests/pointwise_ref.py holds bn_relu_bwd's dz)
    affine      scale = gamma / sqrt(var + eps) to 4U, shift = beta - mean scale to two more roundings (affine_fractions)
    dgamma      (dscale - mean dbeta) / sqrt(var + eps) in five fp32 roundings (product, sum, var + eps, rsqrt, product): the bars of
                the two sums carried through, + 5U (|dscale| + |mean dbeta|) / sqrt(var + eps)

Deliberately wrong evaluations (`wrong=`, WRONG) are told apart from the right one by tests/test_encoder_ref_cpu.py."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sconv_ref as S  # noqa: E402
import x3_ref as X  # noqa: E402
from oracle.ref_ops import same_pads  # noqa: E402

U = S.U
F32 = np.float32
KS = 5
BN_EPS = 1e-3                   # oracle/ref_ops.py:batch_norm_inference
EXP_KERNELS, EXP_TENSORS = 14, 13
WRONG = ('pad_prev_t_in', 'dbias_twice', 'dbias_dropped', 'bn_slice_prev', 'dgamma_no_mean', 'parity_swap', 'drop_last_tap')


def conv_scope(i):
    return 'encoder/conv1d' + ('' if i == 0 else '_%d' % i)


def bn_scope(i):
    return 'encoder/batch_normalization' + ('' if i == 0 else '_%d' % i)


# ---------------------------------------------------------------------------------------------------- number format
def scale_rule(amax, target_exp):
    """The power of two that puts amax into [2^(target_exp - 1), 2^target_exp) -- below 2^(target_exp + 1) --, as float; an amax of
    zero keeps the slot's start-up scale of 1 (x3_ref.update_scales)."""
    s, flag = X.update_scales([X.amax_bits(np.float32(amax))], [1.0], target_exp)
    assert flag == 0
    return float(s[0])


def planes(a, s):
    """(h1, h2) of s * a as float64; s None: (a in float64, None) -- no split, no rounding."""
    if s is None:
        return np.asarray(a, np.float64), None
    return X.planes_of(a, s)


def _inv(sa, sb):
    return 1.0 if sa is None else S._inv(sa, sb)


def _mm3(a1, a2, b1, b2):
    """(sum, sum of absolute values) over K of a1 b1 + a1 b2 + a2 b1; a [..][N][K], b [K][M]; a2 / b2 None: a1 b1 alone."""
    if a2 is None:
        return a1 @ b1, np.abs(a1) @ np.abs(b1)
    return a1 @ (b1 + b2) + a2 @ b1, np.abs(a1) @ (np.abs(b1) + np.abs(b2)) + np.abs(a2) @ np.abs(b1)


def _read(h, idx, bound):
    """h [B][C][L] at idx [N] -> [B][C][N], zero outside [0, bound).  bound = L: the row's own extent.  Another bound is a mistake
    (wrong = 'pad_prev_t_in'): the rows are one flat array, and behind a row lies the next one."""
    B, C, L = h.shape
    if bound == L:
        return X.gather(h, idx)
    flat = np.concatenate([h.reshape(-1), np.zeros(bound + 8)])
    base = (np.arange(B * C) * L).reshape(B, C, 1)
    ok = (idx >= 0) & (idx < bound)
    return np.where(ok, flat[np.clip(base + idx, 0, flat.size - 1)], 0.0)


# ---------------------------------------------------------------------------------------------------- the three contractions
def conv_s2(x, w, bias, T_in, sx=None, sw=None, wrong=None):
    """keras_conv1d(stride = 2, padding = 'same'): pre[b][m][t] = bias[m] + sum_j sum_c w[j][c][m] x[b][c][2 t + j - pad_left],
    pad_left = same_pads(T_in, k, 2)[0], zero outside [0, T_in); x [B][C][T_in], w [k][C][M].  Returns (pre, abs_sum) [B][M][ceil(T_in / 2)],
    abs_sum without the bias."""
    ks, C, M = w.shape
    L = x.shape[2]
    pl = same_pads(T_in, ks, 2)[0]
    t = np.arange(-(-L // 2))
    taps = range(ks - (wrong == 'drop_last_tap'))
    x1, x2 = planes(x, sx)
    w1, w2 = planes(w, sw)
    ops = [None if h is None else np.concatenate([_read(h, 2 * t + j - pl, T_in) for j in taps], axis=1).transpose(0, 2, 1) for h in (x1, x2)]
    wm = [None if h is None else h[:len(taps)].reshape(len(taps) * C, M) for h in (w1, w2)]
    val, ab = _mm3(ops[0], ops[1], wm[0], wm[1])
    inv = _inv(sx, sw)
    pre, ab = val.transpose(0, 2, 1) * inv, ab.transpose(0, 2, 1) * inv
    if bias is not None:
        pre = pre + np.asarray(bias, np.float64)[None, :, None]
    return pre, ab


def dgrad_taps_of(T_in, ks=KS):
    """Per input time u < T_in: the number of taps that reach it (those of its parity)."""
    pl = same_pads(T_in, ks, 2)[0]
    return np.array([len(S.dgrad_taps(ks, pl, r)) for r in (0, 1)])[np.arange(T_in) % 2]


def dgrad_s2(dy, w, T_in, sy=None, sw=None, wrong=None):
    """The transposed conv: dx[b][c][u] = sum_{j, t: 2 t + j - pad_left = u} sum_m w[j][c][m] dy[b][m][t], u < T_in; dy [B][M][T_q],
    w [k][C][M] the forward kernel.  Returns (dx, abs_sum) [B][C][T_in]."""
    ks, C, M = w.shape
    pl = same_pads(T_in, ks, 2)[0]
    u = np.arange(T_in)
    taps = range(ks - (wrong == 'drop_last_tap'))
    y1, y2 = planes(dy, sy)
    w1, w2 = planes(w, sw)
    idx = [np.where((u + pl - j) % 2 == 0, (u + pl - j) // 2, -(10 ** 9)) for j in taps]
    ops = [None if h is None else np.concatenate([X.gather(h, i) for i in idx], axis=1).transpose(0, 2, 1) for h in (y1, y2)]
    wm = [None if h is None else h[:len(taps)].transpose(0, 2, 1).reshape(len(taps) * M, C) for h in (w1, w2)]
    val, ab = _mm3(ops[0], ops[1], wm[0], wm[1])
    inv = _inv(sy, sw)
    dx, ab = val.transpose(0, 2, 1) * inv, ab.transpose(0, 2, 1) * inv
    if wrong == 'parity_swap':      # the two parity launches write each other's output times
        assert T_in % 2 == 0
        dx = dx.reshape(dx.shape[0], C, T_in // 2, 2)[..., ::-1].reshape(dx.shape[0], C, T_in)
    return dx, ab


def wgrad_s2(x, dy, sx=None, sy=None, ks=KS, wrong=None):
    """dw[j][c][m] = sum_{b, t} x[b][c][2 t + j - pad_left] dy[b][m][t], zero outside [0, T_in); x [B][C][T_in], dy [B][M][T_q].
    Returns (dw, abs_sum) [k][C][M]."""
    B, C, T_in = x.shape
    M, T = dy.shape[1:]
    pl = same_pads(T_in, ks, 2)[0]
    t = np.arange(T)
    x1, x2 = planes(x, sx)
    q = [None if h is None else h.transpose(0, 2, 1).reshape(B * T, M) for h in planes(dy, sy)]
    dw, ab = [], []
    for j in range(ks):
        a = [None if h is None else X.gather(h, 2 * t + j - pl).transpose(1, 0, 2).reshape(C, B * T) for h in (x1, x2)]
        if wrong == 'drop_last_tap' and j == ks - 1:
            a = [None if h is None else 0.0 * h for h in a]
        v, s = _mm3(a[0], a[1], q[0], q[1])
        dw.append(v)
        ab.append(s)
    inv = _inv(sx, sy)
    return np.stack(dw) * inv, np.stack(ab) * inv


def dbias(dy, sy=None):
    """(sum, sum of absolute values) over batch and time of dy [B][M][T]; sy: of dy as its two planes hold it, (h1 + h2) / sy."""
    q1, q2 = planes(dy, sy)
    q = q1 if q2 is None else (q1 + q2) / float(np.float32(sy))
    return q.sum((0, 2)), np.abs(q).sum((0, 2))


def conv_1x1(x, w, bias):
    """keras_conv1d(k = 1, 'valid'): x [B][C][T], w [C][M] -> (pre, abs_sum) [B][M][T]."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    pre = np.einsum('bct,cm->bmt', x, w, optimize=True)
    ab = np.einsum('bct,cm->bmt', np.abs(x), np.abs(w), optimize=True)
    return (pre if bias is None else pre + np.asarray(bias, np.float64)[None, :, None]), ab


def dgrad_1x1(dy, w):
    dy, w = np.asarray(dy, np.float64), np.asarray(w, np.float64)
    return np.einsum('bmt,cm->bct', dy, w, optimize=True), np.einsum('bmt,cm->bct', np.abs(dy), np.abs(w), optimize=True)


def wgrad_1x1(x, dy):
    x, dy = np.asarray(x, np.float64), np.asarray(dy, np.float64)
    return np.einsum('bct,bmt->cm', x, dy, optimize=True), np.einsum('bct,bmt->cm', np.abs(x), np.abs(dy), optimize=True)


# ---------------------------------------------------------------------------------------------------- BatchNorm and relu
def bn_of(P, i, wrong=None):
    """(gamma, beta, mean, var) of layer i in float64 ('bn_slice_prev': of layer i - 1)."""
    b = bn_scope(i - 1 if (wrong == 'bn_slice_prev' and i > 0) else i)
    return tuple(np.asarray(P[b + '/' + n], np.float64) for n in ('gamma', 'beta', 'moving_mean', 'moving_variance'))


def bn_affine(bn):
    """batch_norm_inference as out = scale r + shift."""
    gamma, beta, mean, var = bn
    scale = gamma / np.sqrt(var + BN_EPS)
    return scale, beta - mean * scale


def bn_relu_bwd(g, r, mask, bn, wrong=None):
    """g = d loss / d (BatchNorm output) [B][C][T], r the BatchNorm's input (the relu output; the conv output where there is no relu),
    mask [B][C][T] bool (None: no relu).  Returns dict: dconv = g scale mask, dbeta = sum g, dscale = sum g r, dgamma, dbias = sum dconv,
    and the sums' absolute sums *_abs."""
    gamma, beta, mean, var = bn
    scale, _ = bn_affine(bn)
    g, r = np.asarray(g, np.float64), np.asarray(r, np.float64)
    dconv = g * scale[None, :, None]
    if mask is not None:
        dconv = dconv * mask
    out = dict(dconv=dconv, dbeta=g.sum((0, 2)), dbeta_abs=np.abs(g).sum((0, 2)), dscale=(g * r).sum((0, 2)), dscale_abs=np.abs(g * r).sum((0, 2)),
               dbias=dconv.sum((0, 2)), dbias_abs=np.abs(dconv).sum((0, 2)))
    inv = 1.0 / np.sqrt(var + BN_EPS)
    out['dgamma'] = (out['dscale'] - (0.0 if wrong == 'dgamma_no_mean' else mean * out['dbeta'])) * inv
    return out


# ---------------------------------------------------------------------------------------------------- bars
def conv_bars(pre, abs_sum, n, bias, scale, shift, relu):
    """(out, r, bar_out, bar_r) of bias -> relu -> affine over the contraction `pre` (without bias) of n products per element."""
    return S.fwd_epilogue(pre, abs_sum, n, bias, scale, shift, relu)


def cin1_bars(pre, abs_sum, bias, scale, shift, ks=KS):
    """Layer 0 (one input channel): (out, r, bar_out, bar_r) as tests/pointwise_ref.py:conv_cin1_fwd_ref; pre without bias."""
    col = lambda v: np.asarray(v, np.float64)[None, :, None]  # noqa: E731
    v = pre + col(bias)
    vbar = (ks + 1) * U * (abs_sum + np.abs(col(bias)))
    r = np.maximum(v, 0.0)
    return col(scale) * r + col(shift), r, np.abs(col(scale)) * vbar + 2.0 * U * (np.abs(col(scale) * r) + np.abs(col(shift))), vbar


def dgrad_bar(dx, abs_sum, n):
    """n: products per element ([T_in] or a number)."""
    e_acc = np.asarray(n, np.float64) * U * abs_sum
    return e_acc + U * (np.abs(dx) + e_acc)


def masked_bar(dx, bar, scale):
    """Of dx scale mask formed by one fp32 product from a dx inside `bar`."""
    s = np.abs(np.asarray(scale, np.float64))[None, :, None]
    return s * bar + U * s * np.abs(dx)


def dw_bar(dw, abs_sum, n):
    e_acc = n * U * abs_sum
    P = np.abs(dw) + e_acc
    return e_acc + U * P + 2 * U * P


def sum_bar(abs_sum, n, carried=0.0):
    """A channel sum of n addends; carried: the sum of the addends' own bars."""
    return (n + 3) * U * abs_sum + carried


def dgamma_bar(bw, bar_dscale, bar_dbeta, bn):
    _, _, mean, var = bn
    inv = 1.0 / np.sqrt(var + BN_EPS)
    return inv * (bar_dscale + np.abs(mean) * bar_dbeta) + 5 * U * inv * (np.abs(bw['dscale']) + np.abs(mean * bw['dbeta']))


# ---------------------------------------------------------------------------------------------------- the chain
def kernels_of(P):
    """([w_0 .. w_5] as [k][Cin][F], w_6 [F][D], [bias_0 .. bias_6]) in float64."""
    w = [np.asarray(P[conv_scope(i) + '/kernel'], np.float64) for i in range(7)]
    return w[:6], w[6][0], [np.asarray(P[conv_scope(i) + '/bias'], np.float64) for i in range(7)]


def encoder_forward(x, P, masks=None):
    """x [B][T] -> dict(X = BatchNorm outputs of layers 0..5, r = relu outputs, pre = conv outputs, y6, z_e [B][D][T / 64]).
    masks: six bool arrays that stand in for pre > 0."""
    w, w6, b = kernels_of(P)
    net = np.asarray(x, np.float64)[:, None, :]
    out = dict(X=[], r=[], pre=[], mask=[])
    for i in range(6):
        pre, _ = conv_s2(net, w[i], b[i], net.shape[2])
        mask = pre > 0 if masks is None else np.asarray(masks[i], bool)
        r = pre * mask
        scale, shift = bn_affine(bn_of(P, i))
        net = scale[None, :, None] * r + shift[None, :, None]
        for k, v in (('pre', pre), ('mask', mask), ('r', r), ('X', net)):
            out[k].append(v)
    out['y6'], _ = conv_1x1(net, w6, b[6])
    scale, shift = bn_affine(bn_of(P, 6))
    out['z_e'] = scale[None, :, None] * out['y6'] + shift[None, :, None]
    return out


def encoder_backward(x, P, fw, dz):
    """dz = d loss / d z_e [B][D][Tz] -> {the reference's variable name: gradient}, from the forward pass fw of encoder_forward."""
    w, w6, _ = kernels_of(P)
    G = {}

    def bn_grads(i, bw):
        G[bn_scope(i) + '/gamma'], G[bn_scope(i) + '/beta'] = bw['dgamma'], bw['dbeta']
        G[conv_scope(i) + '/bias'] = bw['dbias']
    bw = bn_relu_bwd(dz, fw['y6'], None, bn_of(P, 6))
    bn_grads(6, bw)
    G[conv_scope(6) + '/kernel'] = wgrad_1x1(fw['X'][5], bw['dconv'])[0][None]
    g = dgrad_1x1(bw['dconv'], w6)[0]
    for i in range(5, -1, -1):
        bw = bn_relu_bwd(g, fw['r'][i], fw['mask'][i], bn_of(P, i))
        bn_grads(i, bw)
        xin = fw['X'][i - 1] if i else np.asarray(x, np.float64)[:, None, :]
        G[conv_scope(i) + '/kernel'] = wgrad_s2(xin, bw['dconv'])[0]
        if i:
            g = dgrad_s2(bw['dconv'], w[i], xin.shape[2])[0]
    return G


# ---------------------------------------------------------------------------------------------------- one step, layer by layer
def route(B, T, F, D, enc_x3=(), on_w=(), w_planes=()):
    """Which launches of one step ran where: enc_x3 = layers whose conv and input gradient ran on the fp16x3 engine, on_w = layers whose
    weight gradient did (the bias gradient then comes from its q_total), w_planes = those of on_w with both operands as kept planes."""
    return dict(B=B, T=T, F=F, D=D, Tl=[T // 2 ** (i + 1) for i in range(6)], enc_x3=tuple(enc_x3), on_w=tuple(on_w), w_planes=tuple(w_planes))


def used_slots(rt):
    """(slots of the scale table the forward pass sets, slots the whole step sets)."""
    fwd = ({0} | set(rt['enc_x3'])) if rt['enc_x3'] else set()
    bwd = {5 + i for i in set(rt['enc_x3']) | set(rt['on_w'])} | {i for i in rt['on_w'] if i not in rt['enc_x3']}
    return fwd, fwd | bwd


def forward_layer(i, xin, P, rt, es, affine, wrong=None):
    """Layer i from its input (layer 0: x [B][1][T]) -> (out, r, bar_out, bar_r); es: the scale table the forward pass read,
    affine = (scale, shift) over all 6 F + D channels."""
    F = rt['F']
    w, w6, b = kernels_of(P)
    k = i - 1 if (wrong == 'bn_slice_prev') else i
    sc, sh = (np.asarray(a, np.float64)[k * F:k * F + (F if i < 6 else rt['D'])] for a in affine)
    if i == 6:
        pre, ab = conv_1x1(xin, w6, None)
        return conv_bars(pre, ab, F, b[6], sc, sh, False)
    T_in = xin.shape[2] * (2 if wrong == 'pad_prev_t_in' else 1)
    if i == 0:
        pre, ab = conv_s2(xin, w[0], None, T_in, wrong=wrong)
        return cin1_bars(pre, ab, b[0], sc, sh)
    on_c = i in rt['enc_x3']
    sx, sw = (float(es[i]), float(es[0])) if on_c else (None, None)
    pre, ab = conv_s2(xin, w[i], None, T_in, sx, sw, wrong=wrong)
    return conv_bars(pre, ab, (3 if on_c else 1) * KS * F, b[i], sc, sh, True)


def backward_layer(i, dev, P, rt, wrong=None):
    """Everything layer i's backward launches write, from the device's own tensors: {name: (reference, bar)}.  dev: x, X, r, y6, scale,
    dX (d(conv_i output)), d6, dz, es (the scale table after the step)."""
    F, B, es = rt['F'], rt['B'], dev['es']
    w, w6, _ = kernels_of(P)
    sc = np.asarray(dev['scale'], np.float64)
    out = {}
    if i == 6:
        bn = bn_of(P, 6)
        bw = bn_relu_bwd(dev['dz'], dev['y6'], None, bn)
        n = B * dev['dz'].shape[2]
        # (ONE fp32 product: bit-exact, as tests/pointwise_ref.py holds bn_relu_bwd's dz)
        d6 = (np.asarray(dev['dz'], F32) * np.asarray(dev['scale'], F32)[6 * F:][None, :, None]).astype(F32).astype(np.float64)
        out['dconv_6'] = (d6, 0.0)
        bars = (sum_bar(bw['dscale_abs'], n), sum_bar(bw['dbeta_abs'], n))
        out['dbeta_6'] = (bw['dbeta'], bars[1])
        out['dgamma_6'] = (bn_relu_bwd(dev['dz'], dev['y6'], None, bn, wrong)['dgamma'], dgamma_bar(bw, bars[0], bars[1], bn))
        dw, ab = wgrad_1x1(dev['X'][5], dev['d6'])
        out['dw_6'] = (dw[None], dw_bar(dw, ab, n)[None])
        s, sa = dbias(dev['d6'])
        out['dbias_6'] = (s, sum_bar(sa, n))
        g, gab = dgrad_1x1(dev['d6'], w6)
        gbar = dgrad_bar(g, gab, rt['D'])
    else:
        d_i, Ti = dev['dX'][i], rt['Tl'][i]
        xin = dev['X'][i - 1] if i else np.asarray(dev['x'])[:, None, :]
        on_c, on_w, both = i in rt['enc_x3'], i in rt['on_w'], i in rt['w_planes']
        sp, sq = (float(es[i]), float(es[5 + i])) if on_w else (None, None)
        dw, ab = wgrad_s2(xin, d_i, sp, sq, wrong=wrong)
        out['dw_%d' % i] = (dw, dw_bar(dw, ab, (3 if on_w else 1) * B * Ti))
        s, sa = dbias(d_i, sq if both else None)
        out['dbias_%d' % i] = (s * {'dbias_twice': 2.0, 'dbias_dropped': 0.0}.get(wrong, 1.0), sum_bar(sa, B * Ti))
        if i == 0:
            return out
        sy, sw = (float(es[5 + i]), float(es[0])) if on_c else (None, None)
        g, gab = dgrad_s2(d_i, w[i], xin.shape[2], sy, sw, wrong=wrong)
        gbar = dgrad_bar(g, gab, (3 if on_c else 1) * F * dgrad_taps_of(xin.shape[2])[None, None, :])
    # the BatchNorm / relu pass of layer i - 1 over the input gradient g
    k = i - 1
    bn, r = bn_of(P, k), np.asarray(dev['r'][k], np.float64)
    mask = r > 0
    sck = sc[k * F:(k + 1) * F]
    out['dconv_%d' % k] = (g * sck[None, :, None] * mask, masked_bar(g, gbar, sck))
    n = B * rt['Tl'][k]
    bw = bn_relu_bwd(g, r, mask, bn)
    bar_b = sum_bar(bw['dbeta_abs'], n, gbar.sum((0, 2)))
    bar_s = sum_bar(bw['dscale_abs'], n, (gbar * np.abs(r)).sum((0, 2)))
    out['dbeta_%d' % k] = (bw['dbeta'], bar_b)
    out['dgamma_%d' % k] = (bn_relu_bwd(g, r, mask, bn, wrong)['dgamma'], dgamma_bar(bw, bar_s, bar_b, bn))
    return out


GRAD_OF = {'dw': lambda i: conv_scope(i) + '/kernel', 'dbias': lambda i: conv_scope(i) + '/bias',
           'dbeta': lambda i: bn_scope(i) + '/beta', 'dgamma': lambda i: bn_scope(i) + '/gamma'}


def device_value(name, dev):
    """The device tensor a name of backward_layer stands for."""
    kind, i = name.rsplit('_', 1)
    i = int(i)
    if kind == 'dconv':
        return dev['d6'] if i == 6 else dev['dX'][i]
    return np.asarray(dev['grads'][GRAD_OF[kind](i)])


def fraction(got, want, bar, what):
    """max err / bar; a bar of zero wants equality."""
    got = np.asarray(got, np.float64)
    assert got.shape == want.shape, '%s: shape %s, reference %s' % (what, got.shape, want.shape)
    assert np.isfinite(got).all(), what + ': not finite'
    err = np.abs(got - want)
    bar = np.broadcast_to(bar, err.shape)
    with np.errstate(divide='ignore', invalid='ignore'):
        f = np.where(bar > 0, err / bar, np.where(err > 0, np.inf, 0.0))
    return float(f.max())


def affine_fractions(dev, P, rt):
    """ws['scale'] / ws['shift'] against batch_norm_inference's affine.  scale: var + eps rounded (half of it survives the root), a
    reciprocal square root within one ulp either side (2U), the product with gamma: 3.5U, held to 4U; shift: its product and its sum."""
    bns = [bn_of(P, i) for i in range(7)]
    gamma, beta, mean, var = (np.concatenate([b[k] for b in bns]) for k in range(4))
    scale, shift = bn_affine((gamma, beta, mean, var))
    return {'bn_scale': fraction(dev['scale'], scale, 4 * U * np.abs(scale), 'bn scale'),
            'bn_shift': fraction(dev['shift'], shift, 4 * U * np.abs(mean * scale) + 2 * U * (np.abs(beta) + np.abs(mean * scale)), 'bn shift')}


def scale_checks(dev, P, rt):
    """[(slot, value found, value the rule gives)] for every slot the step's routes use, plus (slot, found, 1.0) for the others: a slot
    nobody used keeps its start-up scale.  dev['es_fwd']: the table when the forward pass ended, dev['es']: after the step."""
    fwd, both = used_slots(rt)
    amax = lambda a: float(np.abs(np.asarray(a, np.float32)).max())  # noqa: E731
    w = np.stack([np.asarray(P[conv_scope(i) + '/kernel'], np.float32) for i in range(1, 6)])

    def want(slot):
        if slot == 0:
            return scale_rule(amax(w), EXP_KERNELS)
        return scale_rule(amax(dev['X'][slot - 1] if slot <= 5 else dev['dX'][slot - 5]), EXP_TENSORS)
    out = []
    for name, table, used in (('es_fwd', dev['es_fwd'], fwd), ('es', dev['es'], both)):
        for slot in range(len(table)):
            out.append(('%s[%d]' % (name, slot), float(table[slot]), want(slot) if slot in used else 1.0))
    return out


def check_step(dev, P, rt):
    """{name: worst err / bar} of every tensor one training step of the encoder leaves, each layer from the device's own inputs."""
    out = dict(affine_fractions(dev, P, rt))
    for i in range(7):
        out.update(check_forward(i, dev, P, rt))
    for i in range(6, -1, -1):
        out.update(check_backward(i, dev, P, rt))
    return out


def _input_of(i, dev):
    return dev['X'][i - 1] if i else np.asarray(dev['x'])[:, None, :]


def check_forward(i, dev, P, rt):
    ref, r, bar, bar_r = forward_layer(i, _input_of(i, dev), P, rt, dev['es_fwd'], (dev['scale'], dev['shift']))
    return {'fwd_out_%d' % i: fraction(dev['X'][i] if i < 6 else dev['z_e'], ref, bar, 'layer %d output' % i),
            'fwd_r_%d' % i: fraction(dev['r'][i] if i < 6 else dev['y6'], r, bar_r, 'layer %d relu output' % i)}


def check_backward(i, dev, P, rt):
    return {name: fraction(device_value(name, dev), ref, bar, name) for name, (ref, bar) in backward_layer(i, dev, P, rt).items()}


def with_wrong(dev, P, rt, i, wrong):
    """dev with what layer i's launches write replaced by the wrong evaluation `wrong` of them (from the same inputs)."""
    out = dict(dev, X=list(dev['X']), r=list(dev['r']), dX=list(dev['dX']), grads=dict(dev['grads']))
    o, r, _, _ = forward_layer(i, _input_of(i, dev), P, rt, dev['es_fwd'], (dev['scale'], dev['shift']), wrong)
    out['X'][i], out['r'][i] = np.asarray(o, F32), np.asarray(r, F32)
    for name, (v, _) in backward_layer(i, dev, P, rt, wrong).items():
        kind, k = name.rsplit('_', 1)
        if kind == 'dconv':
            out['dX'][int(k)] = np.asarray(v, F32)
        else:
            out['grads'][GRAD_OF[kind](int(k))] = np.asarray(v, F32)
    return out


# ---------------------------------------------------------------------------------------------------- a device made of this file


def _seq_sum(v):
    """Sum over (b, t) of v [B][C][T], one fp32 addition at a time."""
    acc = np.zeros(v.shape[1], F32)
    for b in range(v.shape[0]):
        for t in range(v.shape[2]):
            acc = (acc + v[b, :, t]).astype(F32)
    return acc


def _emu_contract(cols, w):
    """sum_k cols[k] (x) w[k] in fp32, one product and one addition at a time: cols [K][B][1][N], w [K][M]."""
    acc = np.zeros((cols.shape[1], w.shape[1], cols.shape[3]), F32)
    for k in range(w.shape[0]):
        acc = (acc + (cols[k] * w[k][None, :, None]).astype(F32)).astype(F32)
    return acc


def _emu_fwd(xin, w, T_in):
    ks, C, M = w.shape
    pl = same_pads(T_in, ks, 2)[0]
    t = np.arange(-(-T_in // 2))
    x = np.asarray(xin, np.float64)
    cols = np.stack([X.gather(x, 2 * t + j - pl)[:, c, None, :] for j in range(ks) for c in range(C)]).astype(F32)
    return _emu_contract(cols, np.asarray(w, F32).reshape(ks * C, M))


def _emu_dgrad(dy, w, T_in):
    ks, C, M = w.shape
    pl = same_pads(T_in, ks, 2)[0]
    u = np.arange(T_in)
    y = np.asarray(dy, np.float64)
    cols = np.stack([X.gather(y, np.where((u + pl - j) % 2 == 0, (u + pl - j) // 2, -(10 ** 9)))[:, m, None, :] for j in range(ks) for m in range(M)]).astype(F32)
    return _emu_contract(cols, np.asarray(w, F32).transpose(0, 2, 1).reshape(ks * M, C))


def _emu_wgrad(xin, dy, ks=KS):
    B, C, T_in = xin.shape
    T = dy.shape[2]
    pl = same_pads(T_in, ks, 2)[0]
    g = np.stack([X.gather(np.asarray(xin, np.float64), 2 * np.arange(T) + j - pl) for j in range(ks)]).astype(F32)      # [ks][B][C][T]
    acc = np.zeros((ks, C, dy.shape[1]), F32)
    for b in range(B):
        for t in range(T):
            acc = (acc + (g[:, b, :, t][:, :, None] * np.asarray(dy, F32)[b, :, t][None, None, :]).astype(F32)).astype(F32)
    return acc


def _emu_affine(y, bias, sc, sh, relu):
    col = lambda v: np.asarray(v, F32)[None, :, None]  # noqa: E731
    y = (y + col(bias)).astype(F32)
    r = np.maximum(y, F32(0)) if relu else y
    return ((col(sc) * r).astype(F32) + col(sh)).astype(F32), r


def fake_device(x, P, dz, rt, emulate=False, wrong=None):
    """The tensors check_step reads, made on the CPU layer by layer, every one from the fp32 values of the one before: by the float64
    reference rounded to fp32 (emulate False) or by a sequential fp32 evaluation -- every product and every addition rounded, on
    the engine's layers the three plane products of every (tap, channel) in turn (sconv_ref.emulate_sconv / emulate_wgrad).
    wrong = (name of WRONG, layer): that layer's launches evaluate wrongly."""
    F, D, B = rt['F'], rt['D'], rt['B']
    w, w6, b = kernels_of(P)
    wr = lambda i: wrong[0] if (wrong and wrong[1] == i) else None  # noqa: E731
    bns = [bn_of(P, i) for i in range(7)]
    gamma, beta, mean, var = (np.concatenate([bn[k] for bn in bns]) for k in range(4))
    scale = (gamma.astype(F32) * (F32(1) / np.sqrt((var.astype(F32) + F32(BN_EPS)).astype(F32))).astype(F32)).astype(F32)
    shift = (beta.astype(F32) - (mean.astype(F32) * scale).astype(F32)).astype(F32)
    dev = dict(x=np.asarray(x, F32), X=[], r=[], scale=scale, shift=shift, dX=[None] * 6, grads={})
    es = np.ones(12, F32)
    fwd_slots, all_slots = used_slots(rt)
    if 0 in fwd_slots:
        es[0] = scale_rule(np.abs(np.stack(w[1:]).astype(F32)).max(), EXP_KERNELS)
    sl = lambda i: slice(i * F, i * F + (F if i < 6 else D))  # noqa: E731
    net = dev['x'][:, None, :]
    for i in range(7):
        if i in fwd_slots and i:
            es[i] = scale_rule(np.abs(net).max(), EXP_TENSORS)
        if emulate and wr(i) is None:
            if i == 6:
                y = _emu_contract(np.stack([net[:, c, None, :] for c in range(F)]), np.asarray(w6, F32))
            elif i in rt['enc_x3']:
                c = dict(ks=KS, Cin=F, M=F, B=B, T=net.shape[2] // 2, pad_left=same_pads(net.shape[2], KS, 2)[0], dgrad=False)
                y = S.emulate_sconv(c, dict(x=net, w=np.asarray(w[i], F32), sx=float(es[i]), sw=float(es[0])), None)
            else:
                y = _emu_fwd(net, w[i], net.shape[2])
            out, r = _emu_affine(y, b[i], scale[sl(i)], shift[sl(i)], i < 6)
        else:
            out, r, _, _ = forward_layer(i, net, P, rt, es, (scale, shift), wr(i))
        out, r = np.asarray(out, F32), np.asarray(r, F32)
        if i < 6:
            dev['X'].append(out)
            dev['r'].append(r)
            net = out
        else:
            dev['z_e'], dev['y6'] = out, r
    dev['es_fwd'] = es.copy()
    dev['es'] = es
    dev['dz'] = np.asarray(dz, F32)
    dev['d6'] = (dev['dz'] * scale[sl(6)][None, :, None]).astype(F32)
    for i in range(6, -1, -1):
        if 1 <= i < 6 and (5 + i) in all_slots:
            es[5 + i] = scale_rule(np.abs(dev['dX'][i]).max(), EXP_TENSORS)
        if 1 <= i < 6 and i in all_slots and i not in fwd_slots:
            es[i] = scale_rule(np.abs(dev['X'][i - 1]).max(), EXP_TENSORS)
        ref = {k: v[0] for k, v in backward_layer(i, dev, P, rt, wr(i)).items()}
        if emulate and wr(i) is None:
            d_i = dev['d6'] if i == 6 else dev['dX'][i]
            xin = dev['X'][i - 1] if i else dev['x'][:, None, :]
            g = None
            if i == 6:
                acc = np.zeros((F, D), F32)
                for bb in range(B):
                    for t in range(d_i.shape[2]):
                        acc = (acc + (xin[bb, :, t][:, None] * d_i[bb, :, t][None, :]).astype(F32)).astype(F32)
                ref['dw_6'] = acc[None]
                g = _emu_contract(np.stack([d_i[:, m, None, :] for m in range(D)]), np.asarray(w6, F32).T)
                ref['dbeta_6'], dsc = _seq_sum(dev['dz']), _seq_sum((dev['dz'] * dev['y6']).astype(F32))
                ref['dgamma_6'] = ((dsc - (mean[sl(6)].astype(F32) * ref['dbeta_6']).astype(F32)).astype(F32) * (F32(1) / np.sqrt(var[sl(6)].astype(F32) + F32(BN_EPS)))).astype(F32)
            elif i in rt['on_w']:
                c = dict(ks=KS, pad_left=same_pads(xin.shape[2], KS, 2)[0], B=B, T=d_i.shape[2], Tp=xin.shape[2])
                ins = dict(p=xin, q=d_i, sp=float(es[i]), sq=float(es[5 + i]), dw0=np.zeros((KS, F, F), F32))
                ref['dw_%d' % i] = S.emulate_wgrad(c, ins, np.arange(F), np.arange(F))
            else:
                ref['dw_%d' % i] = _emu_wgrad(xin, d_i)
            q = d_i
            if i in rt['w_planes']:
                h1, h2 = X.split(X.scaled(d_i, float(es[5 + i])))
                q = ((h1.astype(F32) + h2.astype(F32)).astype(F32) / F32(es[5 + i])).astype(F32)
            ref['dbias_%d' % i] = _seq_sum(q)
            if 1 <= i <= 5:
                if i in rt['enc_x3']:
                    c = dict(ks=KS, Cin=F, M=F, B=B, T=d_i.shape[2], pad_left=same_pads(xin.shape[2], KS, 2)[0], dgrad=True)
                    g = S.emulate_sconv(c, dict(x=d_i, w=np.ascontiguousarray(np.asarray(w[i], F32).transpose(0, 2, 1)), sx=float(es[5 + i]), sw=float(es[0])), None)
                else:
                    g = _emu_dgrad(d_i, w[i], xin.shape[2])
            if g is not None:
                k = i - 1
                rk = dev['r'][k]
                ref['dconv_%d' % k] = np.where(rk > 0, (g * scale[sl(k)][None, :, None]).astype(F32), F32(0))
                ref['dbeta_%d' % k], dsc = _seq_sum(g), _seq_sum((g * rk).astype(F32))
                ref['dgamma_%d' % k] = ((dsc - (mean[sl(k)].astype(F32) * ref['dbeta_%d' % k]).astype(F32)).astype(F32) * (F32(1) / np.sqrt(var[sl(k)].astype(F32) + F32(BN_EPS)))).astype(F32)
        for name, v in ref.items():
            kind, k = name.rsplit('_', 1)
            if kind == 'dconv':
                if int(k) < 6:
                    dev['dX'][int(k)] = np.asarray(v, F32)
            else:
                dev['grads'][GRAD_OF[kind](int(k))] = np.asarray(v, F32)
    return dev
