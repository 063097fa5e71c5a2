"""Plane-exact float64 reference of the fp16x3 engine's stride-1 convs -- vqw_f16x3_gate_conv and the five forms of
vqw_f16x3_out_conv (epi 0 residual + skip, epi 0 input gradient, epi 0 whole skip path, epi 1 gate backward, epi 2 head) --,
their seeded case tables, their bars and the buffer checks, for tests/test_x3_conv_ref_cpu.py and
tests/test_x3_conv_kernels_gpu.py.

numpy only, float64, written from the sentences of include/vqwave.h ("The fp16x3 engine" down to vqw_f16x3_out_conv) and not
from the kernels' index arithmetic.  The number format comes from tests/x3_ref.py: every operand is scaled by its power of
two (scaled), split into two fp16 planes (split), and a product is a1 b1 + a1 b2 + a2 b1 summed in float64 and multiplied by
winv = w_scale_inv / (x_scale w_scale).  What is left to the device is its fp32 accumulation and its fp32 epilogue, and the
bars bound exactly that.

Bars, elementwise, U = 2^-24.  abs_sum is the sum of the absolute values of the addends of the same contraction (returned by
every reference function, in the units of the unscaled result), n = 3 * taps * channels the number of products summed:

    e_acc = n U abs_sum                      a recursive fp32 sum of n terms in ANY order
    P     = |pre| + e_acc                    the magnitude the epilogue sees;  e_0 = e_acc + U P   (the product with winv)
    A     = |bias + cond|                    e_A = U A where both are there (their sum is formed first), else 0
    gate pre-activation  e_f = e_0 + e_A + U (P + A)                      (the second term only with bias or cond)
    gate outputs         out0: |sg| e_f + |th| e_g / 4 + BAR_GATE;  save0: e_f + BAR_GATE;  save1: e_g / 4 + BAR_GATE
                         tanh is 1-Lipschitz, the sigmoid 1/4-Lipschitz; BAR_GATE = 2e-5 is the project's bar for the fast
                         device exp / rcp of the activations (tests/conv_ref.py), not derived here and not tightened from
                         what the kernels return.  The 'ints' cases, whose pre-activation is exact (e_f = e_g = 0: their bar
                         is BAR_GATE alone), measure how much of it is used (record_property 'gate_activation_err').
    epi 0                e_0 + [bias] U (P + |b|) + [old value] U (P + |b| + |old|)
    epi 2                e_0 + e_A + [bias or cond] U (P + A) + [net_in] U (P + A + |net_in|); the mask is exact
    epi 1                dg = winv acc: e_dg = e_0, D = |dg| + e_dg.  A product of k factors has k - 1 roundings in either
                         association, bounded on the magnitudes with their errors:
        tanh form        om = 1 - th^2: e_om = U th^2 + U |om|;  F = sg om;  qf: e_dg |F| + D sg e_om + 2U D (|F| + sg e_om)
                         os = 1 - sg:   e_os = U |os|;  G = th sg os;        qg: e_dg |G| + D |th sg| e_os + 3U D (|G| + |th sg| e_os)
        gated form       q = g^2 / sg: the square, v_rcp_f32 (1 ulp = 2U) and the product: e_q = 4U q + 2 |th| e_g, + q where
                         g^2 lies below the smallest normal number (the square underflows: all of q may be lost);
                         ff = sg - q (0 where sg is below the smallest normal number): e_ff = e_q + U |ff|
                                                                             qf: e_dg |ff| + D e_ff + U D (|ff| + e_ff)
                         G = g os;  e_G = |g| e_os + |os| e_g                qg: e_dg |G| + D e_G + 2U D (|G| + e_G)
                         e_g = 0 for fp32 g; for g read from planes 2^-22 |g| (the header's bound of the split) + 2^-25 (the
                         planes of the gated output are unscaled: below 2^-14 the second plane is an fp16 subnormal of
                         spacing 2^-24); through ff it is multiplied by |d ff / d g| = 2 |th|
                         + 2^-126 on every epi 1 bar: a product below the smallest normal number may be flushed to zero
    decoded planes       of an output that has no fp32 copy: bar + 2^-22 |value|

No constant was moved: the sequential fp32 emulations of tests/test_x3_conv_ref_cpu.py (forward, reversed, pairwise halves of K)
stay under EMU_FRACTION of every bar as derived.  e_acc grows with n abs_sum ~ n^2 while the rounding error of a random sum
grows with sqrt(n): measured errors are small fractions of these bars, and the sharp test for a misplaced tap, chunk, row or
frame is the exact-integer family.

Two operand families per case:
 'normal'  seeded standard-normal activations, weights scaled by (ks Cin)^-1/2, gradients of order 1e-5 lifted by power-of-two
           guard scales.
 'ints'    integer activations |x| <= 4 and weights |w| <= 2; bias, condition, net_in, skip multiples of 1/8 in [-1, 1]; scales
           powers of two: every low plane is zero and every partial sum is exact in fp32 in any order.  Linear outputs, their
           planes and their max-abs word must equal the reference bit for bit (but for the sign of the second plane of an element
           that is itself a zero, which the header leaves open: check_planes); mask sources hold +0.0, -0.0 and negative values.
           Gate conv: winv is the power of two that puts the standard deviation of the scaled contraction in (0.5, 1] -- the
           pre-activation is exact and lies on a grid of step winv.  Epi 1: th multiples of 1/8, sg in {1/2, 1/4, 1/8} (where
           v_rcp_f32 is exact) and integer dg: every product has at most 24 significant bits in either association.

Deliberately wrong evaluations (`wrong=` of the reference functions, WRONG below) are told apart from the right one by
tests/test_x3_conv_ref_cpu.py."""
import functools

import numpy as np

import x3_ref as X
from epilogue_cases import GATE_SUBSETS
from sconv_ref import EMU_FRACTION, F32, GUARD, SENTINEL, U, seed_of, unsplit  # noqa: F401

BAR_GATE = 2e-5                 # tests/conv_ref.py
SPLIT_REL = 2.0 ** -22          # include/vqwave.h: h1 + h2 against the fp32 value
TINY = 2.0 ** -126
F16_HALF_STEP = 2.0 ** -25      # half the spacing of fp16 subnormals: what the second plane of an unscaled tensor cannot hold
MIN_NORMAL = float(F32(1.17549435e-38))
PLANE_FILL = 0x2b67             # what every planes buffer holds before a launch
HALF = X.X3_HALF_BLOCKS
MODES = (('m0', 0), ('half', HALF))
KINDS = ('ints', 'normal')
MAX_BYTES = 64 << 20

WRONG = ('leak', 'drop_last_tap', 'drop_last_kstep', 'no_h2h1', 'gate_rows_unpermuted', 'cond_frame_plus_one',
         'cond_bstride_ignored', 'bias_filter_half_only', 'dir_sign', 'net_in_dropped', 'skip_overwritten', 'mask_ge_zero',
         'relu_on_net_out', 'kc0_ignored:xp', 'kc0_ignored:out_planes', 'kc0_ignored:planes', 'kc0_ignored:aux0',
         'plane_scale_ignored', 'bwd_gate_half_uses_filter_factor', 'bwd_underflow_not_zeroed')


# ---------------------------------------------------------------------------------------------------- the contraction
def shifts(ks, dilation, direction=1):
    """Tap j reads x[t - shift_j]: (ks-1-j) * dilation behind (causal) or, dir < 0, ahead."""
    return [(ks - 1 - j) * dilation * (-1 if direction < 0 else 1) for j in range(ks)]


def conv_pre(x, w, sh, sx, sw, winv=None, split=X.split, wrong=None, ch0=0, kslice=None):
    """(pre, abs_sum, n): pre[b][m][t] = winv sum_j sum_c w[j][c][m] x[b][ch0 + c][t - sh[j]] over the planes of sx x and sw w,
    zero outside the batch row.  x [B][C_all][T], w [ks][C][M].  kslice: only these channels are summed (the emulations)."""
    ks, C, M = w.shape
    T = x.shape[2]
    if wrong == 'kc0_ignored:xp':
        ch0 = 0
    x1, x2 = X.planes_of(x[:, ch0:ch0 + C], sx, split)
    w1, w2 = (h.copy() for h in X.planes_of(w, sw, split))
    if wrong == 'drop_last_tap' and ks > 1:
        w1[ks - 1], w2[ks - 1] = 0.0, 0.0
    if wrong == 'drop_last_kstep':
        w1[ks - 1, C - 16:], w2[ks - 1, C - 16:] = 0.0, 0.0
    if kslice is not None:
        x1, x2, w1, w2 = x1[:, kslice], x2[:, kslice], w1[:, kslice], w2[:, kslice]
        C = x1.shape[1]
    t = np.arange(T)
    a1, a2 = (np.concatenate([X.gather(h, t - s, leak=(wrong == 'leak')) for s in sh], axis=1) for h in (x1, x2))
    val, ab = X.three_terms(a1, a2, w1.reshape(ks * C, M), w2.reshape(ks * C, M), wrong == 'no_h2h1')
    winv = 1.0 / (float(F32(sx)) * float(F32(sw))) if winv is None else float(F32(winv))
    return val * winv, ab * winv, 3 * ks * C


def cond_rows(cond, B, rows, cond_T, bstride, T, wrong=None):
    """cond[b * bstride + m * cond_T + t / (T / cond_T)] as [B][rows][T] float64 (cond: the flat buffer)."""
    flat = np.asarray(cond, F32).astype(np.float64).reshape(-1)
    if wrong == 'cond_bstride_ignored':
        bstride = rows * cond_T
    fr = np.arange(T) // (T // cond_T) + (wrong == 'cond_frame_plus_one')
    idx = (np.arange(B) * bstride)[:, None, None] + (np.arange(rows) * cond_T)[None, :, None] + fr[None, None, :]
    return flat[np.minimum(idx, flat.size - 1)]


def _col(v):
    return np.asarray(v, F32).astype(np.float64)[None, :, None]


def _f64(v):
    return np.asarray(v, F32).astype(np.float64)


def _added(pre, ab, n, bias, cond):
    """(pre + bias + cond, its bar, A): bias / cond are [.][M][.] float64 arrays or None."""
    e_acc = n * U * ab
    P = np.abs(pre) + e_acc
    e = e_acc + U * P
    if bias is None and cond is None:
        return pre, e, P
    add = (0.0 if bias is None else bias) + (0.0 if cond is None else cond)
    A = np.abs(add)
    if bias is not None and cond is not None:
        e = e + U * A
    return pre + add, e + U * (P + A), P + A


def plane_image(val, scale=1.0, scale_dev=1.0, kc0=0, KC=0, prefill=None, wrong=None):
    """The planes a kernel writes for its fp32 values val [B][C][T]: [2][KC][B T][8] uint16 with this tensor's chunks from kc0,
    every other chunk as before the launch (prefill, default PLANE_FILL)."""
    B, C, T = val.shape
    KC_ = KC if KC > 0 else C // 8
    into = np.full((2, KC_, B * T, 8), PLANE_FILL, np.uint16) if prefill is None else prefill
    if wrong == 'plane_scale_ignored':
        scale, scale_dev = 1.0, 1.0
    if wrong is not None and wrong.startswith('kc0_ignored:'):
        kc0 = 0
    return X.act_planes(np.asarray(val, F32), scale, scale_dev, kc0, KC_, into=into)


def decode_planes(img, kc0, C, B, T, scale=1.0):
    """The values h1 + h2 (over scale) of the C channels from chunk kc0 of a planes image [2][KC][B T][8] -> [B][C][T] float64."""
    h = img.view(np.float16).astype(np.float64)[:, kc0:kc0 + C // 8]           # [2][C/8][BT][8]
    v = (h[0] + h[1]).transpose(1, 0, 2).reshape(B, T, C).transpose(0, 2, 1)
    return v / scale


# ---------------------------------------------------------------------------------------------------- gate conv
def gate_ref(c, ins, mode=0, split=X.split, wrong=None, kslice=None):
    """dict(out0, save0, save1 [B][R][T], bar_out0, bar_save0, bar_save1, f, g (the pre-activations), e_f, e_g)."""
    B, T, R, ks = c['B'], c['T'], c['R'], c['ks']
    w = ins['w']
    if wrong == 'gate_rows_unpermuted':
        w = w[:, :, X.gate_row_order(R, mode)]
    pre, ab, n = conv_pre(ins['x'], w, shifts(ks, c['dilation']), ins['sx'], ins['sw'], ins['winv'], split, wrong, kslice=kslice)
    bias = cond = None
    if c['bias']:
        b = np.asarray(ins['bias'], F32).copy()
        if wrong == 'bias_filter_half_only':
            b[R:] = 0
        bias = _col(b)
    if c['cond_T']:
        cond = cond_rows(ins['cond'], B, 2 * R, c['cond_T'], c['cond_bstride'], T, wrong)
    y, e, _ = _added(pre, ab, n, bias, cond)
    if ins.get('exact'):          # the integer family: every partial sum and the sum with bias and condition are exact in fp32
        e = np.zeros_like(e)
    f, g, e_f, e_g = y[:, :R], y[:, R:], e[:, :R], e[:, R:]
    th, sg = np.tanh(f), 1.0 / (1.0 + np.exp(-g))
    return dict(out0=th * sg, save0=th, save1=sg, f=f, g=g, e_f=e_f, e_g=e_g, bar_out0=np.abs(sg) * e_f + np.abs(th) * e_g / 4 + BAR_GATE,
                bar_save0=e_f + BAR_GATE, bar_save1=e_g / 4 + BAR_GATE)


# ---------------------------------------------------------------------------------------------------- epi 0
def out_ref(c, ins, split=X.split, wrong=None, kslice=None):
    """dict(skip [B][S][T], net_out [B][R][T], bar_skip, bar_net); w [ks][Cin][S + R]: S skip rows, then R residual rows."""
    R, S, ks = c['R'], c['S'], c['ks']
    d = -c['dir'] if wrong == 'dir_sign' else c['dir']
    pre, ab, n = conv_pre(ins['x'], ins['w'], shifts(ks, c['dilation'], d), ins['sx'], ins['sw'], None, split, wrong,
                          ch0=8 * c['xp_kc0'], kslice=kslice)
    e_acc = n * U * ab
    P = np.abs(pre) + e_acc
    e = e_acc + U * P
    y = pre
    if c['bias']:
        b = _col(ins['bias'])
        y, P = y + b, P + np.abs(b)
        e = e + U * P
    out = {}
    if S:
        old = _f64(ins['skip'])
        out['skip'] = y[:, :S] + (0.0 if wrong == 'skip_overwritten' else old)
        out['bar_skip'] = e[:, :S] + U * (P[:, :S] + np.abs(old))
    if R:
        if c['net_in'] != 'none':
            old = _f64(ins['net_in'])
            out['net_out'] = y[:, S:] + (0.0 if wrong == 'net_in_dropped' else old)
            out['bar_net'] = e[:, S:] + U * (P[:, S:] + np.abs(old))
        else:
            out['net_out'], out['bar_net'] = y[:, S:], e[:, S:]
    return out


# ---------------------------------------------------------------------------------------------------- epi 2
def head_ref(c, ins, split=X.split, wrong=None, kslice=None):
    """dict(net_out [B][R][T], bar_net, plane_src: the tensor whose planes are written -- net_out, or relu(net_out) with flags bit 0)."""
    B, T, R = c['B'], c['T'], c['R']
    pre, ab, n = conv_pre(ins['x'], ins['w'], [0], ins['sx'], ins['sw'], None, split, wrong, kslice=kslice)
    bias = _col(ins['bias']) if c['bias'] else None
    cond = cond_rows(ins['cond'], B, R, c['cond_T'], c['cond_bstride'], T, wrong) if c['cond_T'] else None
    y, e, P = _added(pre, ab, n, bias, cond)
    if c['net_in']:
        old = _f64(ins['net_in'])
        y = y + (0.0 if wrong == 'net_in_dropped' else old)
        e = e + U * (P + np.abs(old))
    if c['mask']:
        m = np.asarray(ins['mask'], F32)
        mk = (m >= 0) if wrong == 'mask_ge_zero' else (m > 0)
        y, e = y * mk, e * mk
    src = np.maximum(y, 0.0) if c['relu'] else y
    if wrong == 'relu_on_net_out':
        y = np.maximum(y, 0.0)
    return dict(net_out=y, bar_net=e, plane_src=src)


# ---------------------------------------------------------------------------------------------------- epi 1
def bwd_ref(c, ins, split=X.split, wrong=None, kslice=None):
    """dict(dpre [B][2R][T] = {dg sg (1 - th^2), dg th sg (1 - sg)}, bar, dg); x = the gradient [B][Cin][T], w [1][Cin][R] (the
    transposed 1x1 kernels), aux form c['aux'] in ('tanh', 'gated', 'planes')."""
    pre, ab, n = conv_pre(ins['x'], ins['w'], [0], ins['sx'], ins['sw'], None, split, wrong, kslice=kslice)
    e_acc = n * U * ab
    dg = pre
    e_dg = e_acc + U * (np.abs(dg) + e_acc)
    D = np.abs(dg) + e_dg
    sg = _f64(ins['sg'])
    os_ = 1.0 - sg
    e_os = U * np.abs(os_)
    if c['aux'] == 'tanh':
        th = _f64(ins['th'])
        om = 1.0 - th * th
        e_om = U * th * th + U * np.abs(om)
        Ff, G = sg * om, th * sg * (om if wrong == 'bwd_gate_half_uses_filter_factor' else os_)
        qf, qg = dg * Ff, dg * G
        bf = e_dg * np.abs(Ff) + D * sg * e_om + 2 * U * D * (np.abs(Ff) + sg * e_om)
        tsg = np.abs(th * sg)
        bg = e_dg * np.abs(G) + D * tsg * e_os + 3 * U * D * (np.abs(G) + tsg * e_os)
    else:
        g = _f64(ins['gated'])
        if wrong == 'kc0_ignored:aux0' and c['aux'] == 'planes':      # chunk 0 of the wider buffer: another layer's gated output
            g = _f64(ins['gated_wide'][:, :c['R']])
        ok = sg >= MIN_NORMAL
        with np.errstate(divide='ignore', invalid='ignore'):
            th = np.where(ok, g / np.where(ok, sg, 1.0), 0.0)
            q = np.where(ok, g * g / np.where(ok, sg, 1.0), 0.0)
        e_g = SPLIT_REL * np.abs(g) + F16_HALF_STEP if c['aux'] == 'planes' else 0.0
        ff = np.where(ok, sg - q, 0.0)
        if wrong == 'bwd_underflow_not_zeroed':      # a denormal sigmoid: an infinite reciprocal times a square that underflowed
            ff = np.where((sg > 0) & ~ok, np.nan, ff)
        e_ff = np.where(ok, 4 * U * q + np.where(g * g < TINY, q, 0.0) + 2 * np.abs(th) * e_g + U * np.abs(ff), 0.0)
        G = g * ((1.0 - th * th) if wrong == 'bwd_gate_half_uses_filter_factor' else os_)
        e_G = np.abs(g) * e_os + np.abs(os_) * e_g
        qf, qg = dg * ff, dg * G
        bf = e_dg * np.abs(ff) + D * e_ff + U * D * (np.abs(ff) + e_ff)
        bg = e_dg * np.abs(G) + D * e_G + 2 * U * D * (np.abs(G) + e_G)
    return dict(dpre=np.concatenate([qf, qg], axis=1), bar=np.concatenate([bf, bg], axis=1) + TINY, dg=dg)


# ---------------------------------------------------------------------------------------------------- the entry points' rules
def legality(kernel, c):
    """None where include/vqwave.h declares the descriptor legal, else the rule it breaks: the constraints stated with
    vqw_f16x3_gate_desc and in the paragraph "Refused before anything is launched" above vqw_f16x3_out_conv.  kernel: 'gate' or 'out'."""
    if c['B'] <= 0 or c['T'] <= 0 or c['T'] % 256:
        return 'T % 256 == 0'
    if not c.get('w_scale_inv', 1.0) > 0:
        return 'w_scale_inv must be positive'
    if c.get('mode', 0) not in (0, 1, 2, 3):
        return 'mode is a bit set of VQW_X3_BF16 | VQW_X3_HALF_BLOCKS'
    ct = c.get('cond_T', 0)
    if ct and (c['T'] % ct or (c['T'] // ct) % 32):
        return '(T / cond_T) % 32 == 0'
    if kernel == 'gate':
        R = c['R']
        if R <= 0 or R % 128:
            return 'R % 128 == 0'
        if not (1 <= c['ks'] <= 8 and c['dilation'] >= 1):
            return '1..8 taps'
        if c.get('out_planes_KC', 0) and c.get('out_planes_kc0', 0) + R // 8 > c['out_planes_KC']:
            return 'out_planes holds KC chunks, this layer from kc0'
        if ct and c.get('cond_bstride', 2 * R * ct) < 2 * R * ct:
            return 'cond_bstride'
        return None
    R, S, epi = c['R'], c.get('S', 0), c.get('epi', 0)
    if R < 0 or S < 0 or R % 256 or S % 256 or R + S == 0:
        return 'R % 256 == 0, S % 256 == 0'
    Cin = c.get('Cin', 0) or R
    ks = c.get('ks', 1) or 1
    KC = c.get('xp_KC', 0) or Cin // 8
    if Cin < 64 or Cin % 32 or not 1 <= ks <= 8:
        return 'Cin a multiple of 32 from 64'
    if c.get('xp_kc0', 0) + Cin // 8 > KC or (ks > 1 and c.get('xp_kc0', 0) > 0):
        return 'the contraction starts at chunk kc0 of KC'
    if epi in (1, 2) and (S > 0 or R == 0):
        return 'epi 1 / 2: S = 0'
    if epi == 2 and ks > 1:
        return 'epi 2: a 1x1 kernel'
    if epi == 2 and ct and c.get('cond_bstride', R * ct) < R * ct:
        return 'cond_bstride'
    return None


# ---------------------------------------------------------------------------------------------------- cases
def _gate(B, T, R, ks, dil, cond_T=0, pad=0, bias=True, subset=None, kc0=0, KC=0, tag=''):
    c = dict(kernel='gate', B=B, T=T, R=R, ks=ks, dilation=dil, cond_T=cond_T, cond_bstride=2 * R * cond_T + pad, bias=bias,
             subset=tuple(subset or ('out0', 'save0', 'save1', 'out_planes')), out_planes_kc0=kc0, out_planes_KC=KC)
    c['name'] = 'gate/B=%d/T=%d/R=%d/ks=%d/d=%d/cond_T=%d/pad=%d/bias=%d/kc0=%d/KC=%d/%s%s' % (
        B, T, R, ks, dil, cond_T, pad, bias, kc0, KC, '+'.join(c['subset']), tag)
    return c


def gate_cases():
    out = [_gate(2, 256, 128, 2, 1, cond_T=8, pad=24),                 # T / cond_T = 32, a batch stride wider than the rows read
           _gate(2, 256, 256, 3, 2, cond_T=4, pad=8),                  # T / 64
           _gate(1, 256, 384, 1, 1, cond_T=1, pad=40),                 # three 256-row blocks, one tap, one frame
           _gate(2, 256, 128, 8, 1, cond_T=8),
           _gate(2, 512, 128, 2, 255, cond_T=16, pad=16),              # a tile - 1
           _gate(2, 512, 128, 3, 256, cond_T=8),                       # a tile = T / 2, and the first tap a whole batch row
           _gate(2, 512, 128, 2, 512, cond_T=8),                       # T
           _gate(2, 512, 128, 2, 1024, cond_T=8),                      # 2T: past the batch row
           _gate(3, 768, 128, 3, 384, cond_T=24, pad=8),               # T / 2 and T on three column tiles per batch row
           _gate(2, 256, 128, 2, 1, cond_T=0, bias=True),              # no condition
           _gate(2, 256, 128, 2, 1, cond_T=8, bias=False),             # no bias
           _gate(2, 256, 128, 2, 1, cond_T=0, bias=False)]
    for sub in GATE_SUBSETS:
        if len(sub) < 4:
            out.append(_gate(2, 256, 128, 2, 1, cond_T=8, pad=24, subset=sub))
    for kc0 in (0, 16, 32):                                            # inside a three-layer buffer
        out.append(_gate(2, 256, 128, 2, 1, cond_T=8, pad=24, kc0=kc0, KC=48, subset=('out0', 'save1', 'out_planes')))
    out.append(_gate(2, 256, 128, 2, 1, cond_T=8, pad=24, kc0=16, KC=48, subset=('save1', 'out_planes')))
    return out


def _out(B, T, R, S, Cin, ks=1, dil=1, direction=1, net_in='distinct', bias=True, planes=False, pkc0=0, pKC=0, plane_scale=0.0,
         out_scale=1.0, xp_kc0=0, xp_KC=0, alias=False):
    c = dict(kernel='out', epi=0, B=B, T=T, R=R, S=S, Cin=Cin, ks=ks, dilation=dil, dir=direction, net_in=net_in if R else 'none',
             bias=bias, planes=planes, planes_kc0=pkc0, planes_KC=pKC, plane_scale=plane_scale, out_scale=out_scale, xp_kc0=xp_kc0,
             xp_KC=xp_KC, alias=alias)
    c['name'] = 'epi0/B=%d/T=%d/R=%d/S=%d/Cin=%d/ks=%d/d=%d/dir=%d/net_in=%s/bias=%d/planes=%d@%d:%d/ps=%g*%g/xp=%d:%d/alias=%d' % (
        B, T, R, S, Cin, ks, dil, direction, c['net_in'], bias, planes, pkc0, pKC, plane_scale, out_scale, xp_kc0, xp_KC, alias)
    return c


def out_cases():
    return [
        _out(2, 256, 256, 512, 256, planes=True, out_scale=4.0, plane_scale=2.0),
        _out(2, 256, 256, 512, 256, planes=True, out_scale=4.0, plane_scale=2.0, alias=True),
        _out(2, 256, 256, 0, 64, planes=True, pkc0=32, pKC=96),                       # 4 K steps; planes inside a wider buffer
        _out(2, 256, 256, 0, 96, planes=True, out_scale=0.5),                        # 6 K steps
        _out(2, 256, 0, 256, 64, xp_kc0=40, xp_KC=96),                                # the skip path from the middle of a wider xp
        _out(2, 256, 0, 256, 768, xp_kc0=0, xp_KC=96),                                # ... and over all of it: 48 K steps
        _out(1, 256, 512, 256, 96, net_in='none', bias=False),
        _out(1, 256, 512, 256, 768, alias=True, planes=True),
        # the input gradient: S = 0, dir < 0
        _out(2, 512, 256, 0, 64, ks=2, dil=255, direction=-1, net_in='none', planes=True, out_scale=2.0),
        _out(2, 512, 256, 0, 64, ks=3, dil=256, direction=-1, net_in='distinct', planes=True, out_scale=2.0),
        _out(2, 512, 256, 0, 64, ks=2, dil=2, direction=-1, net_in='distinct', alias=True, planes=True, out_scale=2.0),
        _out(2, 512, 256, 0, 96, ks=2, dil=512, direction=-1, net_in='none', bias=False),
        _out(2, 512, 256, 0, 64, ks=3, dil=1024, direction=-1, net_in='distinct', bias=False),
        _out(3, 768, 256, 0, 64, ks=3, dil=384, direction=-1, net_in='none', bias=False, planes=True, out_scale=2.0),
        _out(2, 256, 256, 0, 64, ks=2, dil=1, direction=-1, net_in='none', bias=False),
        # taps of a causal conv through the same entry point
        _out(2, 512, 256, 0, 64, ks=2, dil=255, direction=1, net_in='none'),
    ]


def _bwd(B, T, R, Cin, aux, fp32, underflow=False):
    c = dict(kernel='out', epi=1, B=B, T=T, R=R, S=0, Cin=Cin, aux=aux, fp32=fp32, underflow=underflow,
             aux0_kc0=R // 8 if aux == 'planes' else 0, aux0_KC=3 * (R // 8) if aux == 'planes' else 0)
    c['name'] = 'epi1/B=%d/T=%d/R=%d/Cin=%d/aux0=%s/fp32=%d/underflow=%d' % (B, T, R, Cin, aux, fp32, underflow)
    return c


def bwd_cases():
    return [_bwd(2, 256, 256, 64, 'tanh', 1), _bwd(1, 256, 512, 512, 'tanh', 0),
            _bwd(1, 256, 512, 64, 'gated', 1, True), _bwd(2, 256, 256, 512, 'gated', 0, True),
            _bwd(2, 256, 256, 512, 'planes', 1, True), _bwd(2, 256, 256, 64, 'planes', 0, True),
            _bwd(1, 256, 512, 64, 'planes', 1)]


def _head(B, T, R, Cin, alias='none', cond_T=0, pad=0, relu=False, mask=True, net_in=True, bias=True, planes=True):
    c = dict(kernel='out', epi=2, B=B, T=T, R=R, S=0, Cin=Cin, alias=alias, cond_T=cond_T, cond_bstride=R * cond_T + pad, relu=relu,
             mask=mask, net_in=net_in, bias=bias, planes=planes, out_scale=2.0)
    c['name'] = 'epi2/B=%d/T=%d/R=%d/Cin=%d/alias=%s/cond_T=%d/pad=%d/relu=%d/mask=%d/net_in=%d/bias=%d/planes=%d' % (
        B, T, R, Cin, alias, cond_T, pad, relu, mask, net_in, bias, planes)
    return c


def head_cases():
    out = [_head(2, 256, 256, 64, alias=a, cond_T=8 * cd, relu=bool(r)) for a in ('none', 'net_in', 'aux0') for cd in (0, 1) for r in (0, 1)]
    out += [_head(2, 256, 256, 768, cond_T=4, pad=24, relu=True),
            _head(1, 256, 512, 64, cond_T=1, pad=8),
            _head(2, 256, 256, 64, mask=False, net_in=False, bias=False, cond_T=8, pad=8),
            _head(2, 256, 256, 64, mask=False, net_in=False, bias=False, planes=False)]
    return out


def all_cases():
    return gate_cases() + out_cases() + bwd_cases() + head_cases()


def refusal_cases():
    """(name, kernel, kwargs): descriptors include/vqwave.h forbids, each one change to a legal launch."""
    g = dict(B=2, T=256, R=128, ks=2, dilation=1, cond_T=8, w_scale_inv=1.0, mode=0)
    o = dict(B=2, T=256, R=256, S=0, Cin=64, ks=1, dilation=1, epi=0, w_scale_inv=1.0, mode=0, xp_kc0=0, xp_KC=0)
    mk = lambda d, **kw: dict(d, **kw)  # noqa: E731
    return [('gate T=128', 'gate', mk(g, T=128, cond_T=4)), ('out T=128', 'out', mk(o, T=128)), ('gate R=64', 'gate', mk(g, R=64)),
            ('out R=128', 'out', mk(o, R=128)), ('Cin=48', 'out', mk(o, Cin=48)), ('Cin=80', 'out', mk(o, Cin=80)),
            ('gate T/cond_T=16', 'gate', mk(g, cond_T=16)), ('head T/cond_T=16', 'out', mk(o, epi=2, cond_T=16)),
            ('xp_kc0>0 with ks>1', 'out', mk(o, ks=2, xp_kc0=8, xp_KC=24)), ('xp_kc0+Cin/8>xp_KC', 'out', mk(o, xp_kc0=17, xp_KC=24)),
            ('out_planes_kc0+R/8>KC', 'gate', mk(g, out_planes_kc0=33, out_planes_KC=48)),
            ('epi 2 ks=3', 'out', mk(o, epi=2, ks=3)), ('epi 2 S>0', 'out', mk(o, epi=2, S=256)), ('epi 1 S>0', 'out', mk(o, epi=1, S=256)),
            ('gate w_scale_inv=0', 'gate', mk(g, w_scale_inv=0.0)), ('out w_scale_inv=0', 'out', mk(o, w_scale_inv=0.0)),
            ('gate mode=4', 'gate', mk(g, mode=4)), ('out mode=4', 'out', mk(o, mode=4))]


# What the library says when it refuses each entry (a fragment of vqw_last_error): a descriptor refused for another reason than
# the one its name gives would pass a test that only looks for a refusal.
REFUSED_WITH = {
    'gate T=128': 'T must be a positive multiple of 256', 'out T=128': 'T must be a positive multiple of 256',
    'gate R=64': 'R must be a multiple of 128', 'out R=128': 'R and S must be multiples of 256',
    'Cin=48': 'bad contraction range (Cin=48 ', 'Cin=80': 'bad contraction range (Cin=80 ',
    'gate T/cond_T=16': 'T / cond_T must be a multiple of 32', 'head T/cond_T=16': 'T / cond_T must be a multiple of 32',
    'xp_kc0>0 with ks>1': 'bad contraction range (Cin=64 kc0=8 KC=24)', 'xp_kc0+Cin/8>xp_KC': 'bad contraction range (Cin=64 kc0=17 KC=24)',
    'out_planes_kc0+R/8>KC': 'bad output plane range (kc0=33 KC=48)',
    'epi 2 ks=3': 'epi 2 needs S = 0, net_out, Cin and a 1x1 kernel', 'epi 2 S>0': 'epi 2 needs S = 0, net_out, Cin and a 1x1 kernel',
    'epi 1 S>0': 'gate backward needs S = 0', 'gate w_scale_inv=0': 'w_scale_inv must be positive', 'out w_scale_inv=0': 'w_scale_inv must be positive',
    'gate mode=4': 'mode is a bit set of', 'out mode=4': 'mode is a bit set of'}


def options_of(c):
    """The options of the issue's case tables that a case exercises (the coverage assertion of the CPU suite)."""
    o = set()
    if c['kernel'] == 'gate':
        T = c['T']
        o |= {'gate/R=%d' % c['R'], 'gate/ks=%d' % c['ks'], 'gate/subset=' + '+'.join(c['subset'])}
        d = c['dilation']
        for nm, v in (('1', 1), ('2', 2), ('255', 255), ('256', 256), ('T/2', T // 2), ('T', T), ('2T', 2 * T)):
            if d == v and c['ks'] > 1:
                o.add('gate/d=' + nm)
        if c['cond_T']:
            for nm, v in (('1', 1), ('T/64', T // 64), ('T/32', T // 32)):
                if c['cond_T'] == v:
                    o.add('gate/cond_T=' + nm)
            if c['cond_bstride'] > 2 * c['R'] * c['cond_T']:
                o.add('gate/cond_bstride wider')
        else:
            o.add('gate/no cond')
        if not c['bias']:
            o.add('gate/no bias')
        if c['out_planes_KC']:
            o.add('gate/out_planes_kc0=%d/3' % (c['out_planes_kc0'] // (c['R'] // 8)))
    elif c['epi'] == 0:
        T = c['T']
        o |= {'epi0/(R,S)=(%d,%d)' % (c['R'], c['S']), 'epi0/Cin=%d' % c['Cin']}
        if c['R'] == 0:
            o.add('epi0/skip path Cin=%d %s' % (c['Cin'], 'from the middle' if c['xp_kc0'] else 'over all'))
        if c['dir'] < 0:
            o |= {'dgrad/ks=%d' % c['ks'], 'dgrad/net_in=%s' % ('alias' if c['alias'] else c['net_in'])}
            for nm, v in (('1', 1), ('2', 2), ('255', 255), ('256', 256), ('T/2', T // 2), ('T', T), ('2T', 2 * T)):
                if c['dilation'] == v:
                    o.add('dgrad/d=' + nm)
        o.add('epi0/planes=%s' % ('absent' if not c['planes'] else 'wider' if c['planes_KC'] else 'present'))
        if c['planes'] and c['plane_scale'] not in (0.0, 1.0):
            o.add('epi0/plane_scale')
        if c['planes'] and c['out_scale'] != 1.0:
            o.add('epi0/out_scale')
        if c['alias']:
            o.add('epi0/alias')
        if c['net_in'] == 'none' and c['R']:
            o.add('epi0/net_in NULL')
    elif c['epi'] == 1:
        o |= {'epi1/aux0=%s/fp32=%d' % (c['aux'], c['fp32']), 'epi1/R=%d' % c['R'], 'epi1/Cin=%d' % c['Cin']}
        if c['underflow']:
            o.add('epi1/underflow')
    else:
        o |= {'epi2/alias=%s/cond=%d/relu=%d' % (c['alias'], bool(c['cond_T']), c['relu']), 'epi2/Cin=%d' % c['Cin']}
        if c['cond_T'] and c['cond_bstride'] > c['R'] * c['cond_T']:
            o.add('epi2/cond_bstride wider')
        if not (c['mask'] or c['net_in'] or c['bias']):
            o.add('epi2/mask, net_in, bias absent')
    return o


DILATIONS = ('1', '2', '255', '256', 'T/2', 'T', '2T')
REQUIRED_OPTIONS = frozenset(
    ['gate/R=%d' % r for r in (128, 256, 384)] + ['gate/ks=%d' % k for k in (1, 2, 3, 8)] + ['gate/d=' + d for d in DILATIONS]
    + ['gate/cond_T=' + t for t in ('1', 'T/64', 'T/32')] + ['gate/cond_bstride wider', 'gate/no cond', 'gate/no bias']
    + ['gate/subset=' + '+'.join(s) for s in GATE_SUBSETS] + ['gate/out_planes_kc0=%d/3' % i for i in (0, 1, 2)]
    + ['epi0/(R,S)=(%d,%d)' % rs for rs in ((256, 512), (256, 0), (0, 256), (512, 256))] + ['epi0/Cin=%d' % k for k in (64, 96, 256, 768)]
    + ['epi0/skip path Cin=64 from the middle', 'epi0/skip path Cin=768 over all', 'dgrad/ks=2', 'dgrad/ks=3']
    + ['dgrad/d=' + d for d in DILATIONS] + ['dgrad/net_in=' + n for n in ('none', 'distinct', 'alias')]
    + ['epi0/planes=' + p for p in ('absent', 'present', 'wider')] + ['epi0/plane_scale', 'epi0/out_scale', 'epi0/alias', 'epi0/net_in NULL']
    + ['epi1/aux0=%s/fp32=%d' % (a, f) for a in ('tanh', 'gated', 'planes') for f in (0, 1)] + ['epi1/R=256', 'epi1/R=512', 'epi1/Cin=64',
                                                                                                   'epi1/Cin=512', 'epi1/underflow']
    + ['epi2/alias=%s/cond=%d/relu=%d' % (a, cd, r) for a in ('none', 'net_in', 'aux0') for cd in (0, 1) for r in (0, 1)]
    + ['epi2/Cin=64', 'epi2/Cin=768', 'epi2/cond_bstride wider', 'epi2/mask, net_in, bias absent'])


# ---------------------------------------------------------------------------------------------------- operands
def _ints(rng, shape, lim):
    return rng.integers(-lim, lim + 1, shape).astype(F32)


def _eighths(rng, shape):
    return (rng.integers(-8, 9, shape) / 8.0).astype(F32)


def gate_winv(ks, R, dilation=1, T=1 << 30):
    """The power of two that puts the standard deviation of the integer contraction (R products per tap that reaches into the batch
    row, each of a uniform integer in [-4, 4] and one in [-2, 2]: variance 60/9 * 2) into (0.5, 1]."""
    taps = sum(1 for s in shifts(ks, dilation) if s < T)
    sd = (taps * R * (60.0 / 9.0) * 2.0) ** 0.5
    return 2.0 ** -int(np.ceil(np.log2(sd)))


@functools.lru_cache(maxsize=8)
def _inputs(name, kind):
    c = next(c for c in all_cases() if c['name'] == name)
    rng = np.random.default_rng(seed_of(name, kind))
    B, T, R = c['B'], c['T'], c['R']
    g = lambda *s: rng.standard_normal(s).astype(F32)  # noqa: E731
    nrm = kind == 'normal'
    if c['kernel'] == 'gate':
        ks = c['ks']
        n_cond = (B - 1) * c['cond_bstride'] + 2 * R * c['cond_T']
        if nrm:
            return dict(x=g(B, R, T), w=(g(ks, R, 2 * R) * F32((ks * R) ** -0.5)).astype(F32), bias=(g(2 * R) * F32(0.3)).astype(F32),
                        cond=(g(max(n_cond, 1)) * F32(0.3)).astype(F32), sx=1.0, sw=256.0, winv=1.0 / 256.0)
        return dict(x=_ints(rng, (B, R, T), 4), w=_ints(rng, (ks, R, 2 * R), 2), bias=_eighths(rng, 2 * R), cond=_eighths(rng, max(n_cond, 1)),
                    sx=1.0, sw=1.0, winv=gate_winv(ks, R, c['dilation'], T), exact=True)
    Cin, S = c['Cin'], c['S']
    if c['epi'] == 0:
        ks, C_all = c['ks'], 8 * c['xp_KC'] if c['xp_KC'] else Cin
        grad = c['dir'] < 0
        if nrm:
            x = g(B, C_all, T) * F32(1e-5 if grad else 1.0)
            w = g(ks, Cin, S + R) * F32((ks * Cin) ** -0.5)
            mag = F32(1e-5 if grad else 1.0)
            return dict(x=x.astype(F32), w=w.astype(F32), bias=(g(S + R) * F32(0.3) * mag).astype(F32), skip=g(B, S, T), net_in=(g(B, R, T) * mag).astype(F32),
                        sx=2.0 ** 26 if grad else 1.0, sw=256.0)
        return dict(x=_ints(rng, (B, C_all, T), 4), w=_ints(rng, (ks, Cin, S + R), 2), bias=_eighths(rng, S + R), skip=_eighths(rng, (B, S, T)),
                    net_in=_eighths(rng, (B, R, T)), sx=4.0, sw=8.0)
    if c['epi'] == 2:
        n_cond = max((B - 1) * c['cond_bstride'] + R * c['cond_T'], 1)
        if nrm:
            mask = g(B, R, T)
            d = dict(x=g(B, Cin, T), w=(g(1, Cin, R) * F32(Cin ** -0.5)).astype(F32), bias=(g(R) * F32(0.3)).astype(F32), net_in=g(B, R, T),
                     cond=(g(n_cond) * F32(0.3)).astype(F32), sx=1.0, sw=256.0)
        else:
            mask = _eighths(rng, (B, R, T))
            d = dict(x=_ints(rng, (B, Cin, T), 4), w=_ints(rng, (1, Cin, R), 2), bias=_eighths(rng, R), net_in=_eighths(rng, (B, R, T)),
                     cond=_eighths(rng, n_cond), sx=4.0, sw=8.0)
        mask[:, ::3, ::5] = 0.0           # the mask is (aux0 > 0): +0.0, -0.0 and negative values are all "off"
        mask[:, 1::3, 1::5] = -0.0
        d['mask'] = mask
        return d
    # epi 1
    if nrm:
        xf, xg = g(B, R, T) * F32(2.0), g(B, R, T) * F32(3.0)
        if c['underflow']:
            xg[:, ::7, ::5] = -200.0          # sigmoid == 0
            xg[:, 3::7, 1::5] = -88.0         # a denormal sigmoid
            xg[:, 5::7, 2::5] = -87.0         # the smallest normal numbers
            xg[:, 6::7, 3::5] = -87.4
        with np.errstate(under='ignore', over='ignore'):
            th = np.tanh(xf.astype(np.float64)).astype(F32)
            sg = (1.0 / (1.0 + np.exp(-xg.astype(np.float64)))).astype(F32)
            gated = (th * sg).astype(F32)
        d = dict(x=(g(B, Cin, T) * F32(1e-5)).astype(F32), w=(g(1, Cin, R) * F32(Cin ** -0.5)).astype(F32), th=th, sg=sg, gated=gated,
                 sx=2.0 ** 26, sw=64.0, out_scale=2.0 ** 26)
        others = [(np.tanh(g(B, R, T).astype(np.float64)) / (1.0 + np.exp(-g(B, R, T).astype(np.float64)))).astype(F32) for _ in (0, 1)]
    else:
        th = _eighths(rng, (B, R, T))
        sg = rng.choice(F32([0.5, 0.25, 0.125]), (B, R, T)).astype(F32)
        d = dict(x=_ints(rng, (B, Cin, T), 4), w=_ints(rng, (1, Cin, R), 2), th=th, sg=sg, gated=(th * sg).astype(F32), sx=4.0, sw=8.0, out_scale=2.0)
        others = [(_eighths(rng, (B, R, T)) * rng.choice(F32([0.5, 0.25, 0.125]), (B, R, T))).astype(F32) for _ in (0, 1)]
    if c['aux'] == 'planes':      # three layers' gated outputs side by side, this layer's in the middle: what the wider planes buffer holds
        assert c['aux0_kc0'] == R // 8 and c['aux0_KC'] == 3 * (R // 8)
        d['gated_wide'] = np.concatenate([others[0], d['gated'], others[1]], axis=1)
    return d


def inputs(c, kind):
    return _inputs(c['name'], kind)


def reference(c, ins, mode=0, split=X.split, wrong=None, kslice=None):
    if c['kernel'] == 'gate':
        return gate_ref(c, ins, mode, split, wrong, kslice)
    return (out_ref, bwd_ref, head_ref)[c['epi']](c, ins, split, wrong, kslice)


def plane_scales(c, ins):
    """(host plane_scale, device out_scale) of a case's output planes."""
    if c['kernel'] == 'gate':
        return 1.0, 1.0
    if c['epi'] == 1:
        return 1.0, ins['out_scale']
    return (c.get('plane_scale', 0.0) or 1.0), c.get('out_scale', 1.0)


def case_bytes(c):
    """An upper bound of what a case's launch holds on the device: fp32 tensors and planes."""
    B, T, R, S = c['B'], c['T'], c['R'], c.get('S', 0)
    if c['kernel'] == 'gate':
        return 4 * B * T * (R + 3 * R) + 4 * B * T * R + 4 * c['ks'] * R * 2 * R * 2 + 4 * B * T * max(c['out_planes_KC'] * 8, R)
    Cin = c['Cin']
    Call = 8 * c.get('xp_KC', 0) or Cin
    ks = c.get('ks', 1)
    return 8 * B * T * Call + 8 * ks * Cin * (S + R) + 4 * B * T * (S + 4 * R) * 2 + 4 * B * T * max(c.get('planes_KC', 0) * 8, 2 * R, c.get('aux0_KC', 0) * 8)


# ---------------------------------------------------------------------------------------------------- fp32 emulation
def emulate_pre(c, ins, msel, order='forward'):
    """winv * the contraction of the output rows msel, its 3 ks Cin products of fp16 planes (each exact in fp32) added one at a time
    in fp32: 'forward' (tap, channel, term), 'reversed', or 'pairwise' -- the two halves of K summed forward each, then added."""
    ks = c.get('ks', 1)
    w = ins['w']
    C = w.shape[1]
    ch0 = 8 * c.get('xp_kc0', 0)
    sh = shifts(ks, c.get('dilation', 1), c.get('dir', 1))
    x1, x2 = (h.astype(np.float64) for h in X.split(X.scaled(ins['x'][:, ch0:ch0 + C], ins['sx'])))
    w1, w2 = (h.astype(F32)[:, :, msel] for h in X.split(X.scaled(w, ins['sw'])))
    t = np.arange(c['T'])
    terms = []
    for j in range(ks):
        a1, a2 = (X.gather(h, t - sh[j]).astype(F32) for h in (x1, x2))
        for ch in range(C):
            xa, xb = a1[:, ch, None, :], a2[:, ch, None, :]
            wa, wb = w1[j, ch][None, :, None], w2[j, ch][None, :, None]
            terms += [(xa, wb), (xb, wa), (xa, wa)]

    def run(ts):
        acc = np.zeros((c['B'], len(msel), c['T']), F32)
        for a, b in ts:
            acc = (acc + a * b).astype(F32)
        return acc
    if order == 'reversed':
        acc = run(terms[::-1])
    elif order == 'pairwise':
        acc = (run(terms[:len(terms) // 2]) + run(terms[len(terms) // 2:])).astype(F32)
    else:
        acc = run(terms)
    winv = F32(ins['winv']) if 'winv' in ins else F32(1.0 / (float(F32(ins['sx'])) * float(F32(ins['sw']))))
    return (acc * winv).astype(F32)


def emulate(c, ins, msel, order='forward'):
    """The outputs of a case for the contraction rows msel, every epilogue operation rounded to fp32 on its own, in the order the
    header writes it.  Gate conv: the fp32 pre-activations (f, g are taken from rows msel of the 2R).  Returns a dict of the
    same keys as reference() (values float32, no bars)."""
    y = emulate_pre(c, ins, msel, order)
    B, T, R = c['B'], c['T'], c['R']
    col = lambda v: np.asarray(v, F32)[msel][None, :, None]  # noqa: E731
    if c['kernel'] == 'gate' or c['epi'] == 2:
        rows = 2 * R if c['kernel'] == 'gate' else R
        add = None
        if c['bias']:
            add = col(ins['bias'])
        if c['cond_T']:
            cd = cond_rows(ins['cond'], B, rows, c['cond_T'], c['cond_bstride'], T)[:, msel].astype(F32)
            add = cd if add is None else (add + cd).astype(F32)
        if add is not None:
            y = (y + add).astype(F32)
        if c['kernel'] == 'gate':
            return dict(pre=y)
        if c['net_in']:
            y = (np.asarray(ins['net_in'], F32)[:, msel] + y).astype(F32)
        if c['mask']:
            y = (y * (np.asarray(ins['mask'], F32)[:, msel] > 0)).astype(F32)
        return dict(net_out=y)
    if c['epi'] == 0:
        if c['bias']:
            y = (y + col(ins['bias'])).astype(F32)
        S = c['S']
        old = np.concatenate([np.asarray(ins['skip'], F32).reshape(B, S, T),
                              np.asarray(ins['net_in'], F32).reshape(B, R, T) * F32(c['net_in'] != 'none')], axis=1)[:, msel]
        return dict(rows=(old + y).astype(F32))
    th, sg, g = (np.asarray(ins[k], F32)[:, msel] for k in ('th', 'sg', 'gated'))
    one = F32(1.0)
    if c['aux'] == 'tanh':
        om = (one - (th * th).astype(F32)).astype(F32)
        if order == 'reversed':      # the other association of the products
            qf = (y * (sg * om).astype(F32)).astype(F32)
            qg = (y * ((th * sg).astype(F32) * (one - sg).astype(F32)).astype(F32)).astype(F32)
        else:
            qf = ((y * sg).astype(F32) * om).astype(F32)
            qg = (((y * th).astype(F32) * sg).astype(F32) * (one - sg).astype(F32)).astype(F32)
    else:
        ok = sg >= F32(MIN_NORMAL)
        with np.errstate(divide='ignore', invalid='ignore', over='ignore', under='ignore'):
            rc = (one / np.where(ok, sg, one)).astype(F32)
            ff = np.where(ok, (sg - ((g * g).astype(F32) * rc).astype(F32)).astype(F32), F32(0))
            if order == 'reversed':
                qg = (y * (g * (one - sg).astype(F32)).astype(F32)).astype(F32)
            else:
                qg = ((y * g).astype(F32) * (one - sg).astype(F32)).astype(F32)
        qf = (y * ff).astype(F32)
    return dict(qf=qf, qg=qg)


# ---------------------------------------------------------------------------------------------------- comparing buffers
def compare(got, want, bar, kind, what):
    """err / bar of a written tensor; 'ints': bit equality with the float32 of the reference (a zero is compared by value), 0."""
    got64 = np.asarray(got).astype(np.float64)
    if kind == 'ints':
        bad = np.flatnonzero(got64.reshape(-1) != np.asarray(want, np.float64).reshape(-1))
        assert bad.size == 0, '%s: %d of %d elements differ from the exact result (first: %s got %r want %r)' % (
            what, bad.size, got64.size, np.unravel_index(bad[0], got64.shape), got64.reshape(-1)[bad[0]], np.asarray(want).reshape(-1)[bad[0]])
        return 0.0
    err = np.abs(got64 - want)
    over = ~(err <= bar)
    if over.any():
        with np.errstate(divide='ignore', invalid='ignore'):
            i = np.unravel_index(np.argmax(np.where(over, np.where(np.isfinite(err) & (bar > 0), err / bar, np.inf), 0.0)), err.shape)
        raise AssertionError('%s: %d of %d elements over the bar; worst at %s: got %r want %r err %.3e bar %.3e' % (
            what, int(over.sum()), err.size, i, got64[i], want[i], err[i], bar[i]))
    live = bar > 0
    return float((err[live] / bar[live]).max()) if live.any() else 0.0


def check(full, n, want, bar, kind, what):
    """One fp32 output as the device left it: `full` = GUARD sentinels, the n floats of the view, GUARD sentinels.  The guards must
    hold their bits; the view is compared with want / bar (want None: the header leaves the view unwritten -- sentinels still).
    Returns the worst err / bar."""
    full = np.asarray(full, F32)
    assert full.size == n + 2 * GUARD
    sent = np.full(GUARD, SENTINEL, F32).view(np.uint32)
    assert np.array_equal(full[:GUARD].view(np.uint32), sent) and np.array_equal(full[GUARD + n:].view(np.uint32), sent), what + ': a guard band changed'
    view = full[GUARD:GUARD + n]
    if want is None:
        assert np.array_equal(view.view(np.uint32), np.full(n, SENTINEL, F32).view(np.uint32)), what + ': written, but not an output of this launch'
        return 0.0
    return compare(view.reshape(np.shape(want)), want, bar, kind, what)


def check_planes(full, image, what):
    """A planes buffer as the device left it (uint16: 2 GUARD halves of PLANE_FILL, the image, 2 GUARD halves) against the exact
    image -- written chunks and the chunks the header does not write alike, bit for bit.  One exception, which include/vqwave.h
    states ("a second plane that is zero may carry either sign"): where the element itself is a zero -- BOTH planes of the image
    are zeros, that is scale * x is +-0 -- the second plane is compared by value.  IEEE subtraction gives h2 = +0 there, the
    epilogues' conversion leaves -0 for x = -0.0 (a masked-off negative value of epi 2).  Everywhere else, a zero second plane
    beside a non-zero leading plane included, the bits must be the image's."""
    full = np.asarray(full).view(np.uint16).reshape(-1)
    g2 = 2 * GUARD
    assert full.size == image.size + 2 * g2
    assert (full[:g2] == PLANE_FILL).all() and (full[g2 + image.size:] == PLANE_FILL).all(), what + ': a guard band changed'
    got = full[g2:g2 + image.size].reshape(image.shape).copy()
    either = ((image[0] & 0x7fff) == 0) & ((image[1] & 0x7fff) == 0) & ((got[1] & 0x7fff) == 0)
    got[1][either] = image[1][either]
    bad = np.argwhere(got != image)
    assert bad.shape[0] == 0, '%s: %d of %d halves differ (first at [plane, chunk, row, lane] = %s: got 0x%04x want 0x%04x)' % (
        what, bad.shape[0], image.size, bad[0].tolist(), got[tuple(bad[0])], image[tuple(bad[0])])
