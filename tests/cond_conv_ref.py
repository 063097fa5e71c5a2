"""Float64 numpy restatement of the decoder's conditioning conv (include/vqwave.h, vqw_cond_conv_*), the cases
the GPU tests run it on, their operands and bars, and the wrong kernels those cases must catch.

    pl = (k - 1) / 2, zero padding per utterance, rows independent:
    fwd:    out[b][o][t] = bias[o] + sum_{j<k} sum_{d<D} w[j][d][o] z[b][d][t + j - pl]
    dgrad:  dz[b][d][s]  = sum_{j<k} sum_{o<C} w[j][d][o] dout[b][o][s - j + pl]
    wgrad:  dw[j][d][o]  = sum_{b,t} z[b][d][t + j - pl] dout[b][o][t];   db[o] = sum_{b,t} dout[b][o][t]

Everything here runs on the CPU; tests/test_cond_conv_ref_cpu.py pins it against torch's conv1d and autograd in float64.
"""
import numpy as np

U = 2.0 ** -24          # fp32 unit roundoff

# (B, D, C, Tz, k): rows shorter than the kernel; the benchmark's channels at Tz around a wave and at the benchmark's Tz; no
# multiple of any tile with one tap and with seven; more rows than the weight gradient has splits per row
CASES = [(1, 4, 16, 1, 3), (2, 4, 16, 2, 3), (3, 8, 48, 3, 5),
         (2, 64, 128, 63, 3), (2, 64, 128, 64, 3), (2, 64, 128, 65, 3), (2, 64, 128, 104, 3),
         (2, 20, 144, 37, 1), (2, 20, 144, 37, 7),
         (5, 64, 64, 104, 3)]


def case_id(c):
    return 'B%d-D%d-C%d-Tz%d-k%d' % c


def shifted(z, s):
    """z[..., t + s] with zeros outside the row."""
    Tz = z.shape[-1]
    out = np.zeros_like(z)
    if abs(s) < Tz:
        if s >= 0:
            out[..., :Tz - s] = z[..., s:]
        else:
            out[..., -s:] = z[..., :Tz + s]
    return out


def fwd(z, w, bias, flaw=None):
    """z [B][D][Tz], w [k][D][C], bias [C] -> out [B][C][Tz] (float64).  flaw: one of FLAWS, a wrong kernel."""
    z, w, bias = np.asarray(z, np.float64), np.asarray(w, np.float64), np.asarray(bias, np.float64)
    k, pl = w.shape[0], (w.shape[0] - 1) // 2
    B, D, Tz = z.shape
    if flaw == 'taps_reversed':
        w = w[::-1]
    if flaw == 'padding_shifted':
        pl += 1
    out = np.zeros((B, w.shape[2], Tz))
    flat = z.transpose(1, 0, 2).reshape(D, B * Tz)      # the rows end to end: what a kernel without per-row padding reads
    for j in range(k):
        if flaw == 'neighbour_row':
            zs = shifted(flat, j - pl).reshape(D, B, Tz).transpose(1, 0, 2)
        else:
            zs = shifted(z, j - pl)
        out += np.einsum('do,bdt->bot', w[j], zs)
    if flaw != 'bias_omitted':
        out += bias[None, :, None]
    if flaw == 'last_frame_dropped':
        out[:, :, Tz - 1] = 0.0
    return out


def dgrad(w, dout, flaw=None):
    """w [k][D][C], dout [B][C][Tz] -> dz [B][D][Tz]."""
    w, dout = np.asarray(w, np.float64), np.asarray(dout, np.float64)
    k, pl = w.shape[0], (w.shape[0] - 1) // 2
    B, C, Tz = dout.shape
    if flaw == 'taps_reversed':
        w = w[::-1]
    if flaw == 'padding_shifted':
        pl += 1
    dz = np.zeros((B, w.shape[1], Tz))
    flat = dout.transpose(1, 0, 2).reshape(C, B * Tz)
    for j in range(k):
        if flaw == 'neighbour_row':
            gs = shifted(flat, pl - j).reshape(C, B, Tz).transpose(1, 0, 2)
        else:
            gs = shifted(dout, pl - j)
        dz += np.einsum('do,bot->bdt', w[j], gs)
    if flaw == 'last_frame_dropped':
        dz[:, :, Tz - 1] = 0.0
    return dz


def wgrad(z, dout, k, flaw=None):
    """z [B][D][Tz], dout [B][C][Tz] -> (dw [k][D][C], db [C])."""
    z, dout = np.asarray(z, np.float64), np.asarray(dout, np.float64)
    pl = (k - 1) // 2
    B, D, Tz = z.shape
    if flaw == 'padding_shifted':
        pl += 1
    if flaw == 'last_frame_dropped':
        dout = dout.copy()
        dout[:, :, Tz - 1] = 0.0
    flat = z.transpose(1, 0, 2).reshape(D, B * Tz)
    dw = np.zeros((k, D, dout.shape[1]))
    for j in range(k):
        if flaw == 'neighbour_row':
            zs = shifted(flat, j - pl).reshape(D, B, Tz).transpose(1, 0, 2)
        else:
            zs = shifted(z, j - pl)
        dw[j] = np.einsum('bdt,bot->do', zs, dout)
    if flaw == 'taps_reversed':
        dw = dw[::-1].copy()
    db = dout.sum((0, 2))
    if flaw == 'bias_omitted':
        db = np.zeros_like(db)
    return dw, db


FLAWS = ('taps_reversed', 'padding_shifted', 'last_frame_dropped', 'neighbour_row', 'bias_omitted')


def operands(case, kind, seed=0):
    """fp32 (z, w, bias, dout, dw0, db0) of a case.  kind 'exact': small integers (|v| <= 8: every product is at most 64 and
    every partial sum an integer below 2^24, so fp32 adds them exactly in any order); 'random': standard normal."""
    B, D, C, Tz, k = case
    rng = np.random.default_rng(1000 * seed + 7 * B + 11 * D + 13 * C + 17 * Tz + k)
    shapes = ((B, D, Tz), (k, D, C), (C,), (B, C, Tz), (k, D, C), (C,))
    if kind == 'exact':
        return tuple(rng.integers(-8, 9, size=s).astype(np.float32) for s in shapes)
    return tuple(rng.standard_normal(s).astype(np.float32) for s in shapes)


def results(z, w, bias, dout, dw0, db0, flaw=None):
    """The four outputs as the kernels leave them: out, dz, dw0 + dw, db0 + db."""
    dw, db = wgrad(z, dout, w.shape[0], flaw)
    return {'out': fwd(z, w, bias, flaw), 'dz': dgrad(w, dout, flaw), 'dw': dw0.astype(np.float64) + dw, 'db': db0.astype(np.float64) + db}


def bars(case, z, w, bias, dout, dw0, db0):
    """Per element (n + 2) 2^-24 sum |terms|: the bound of an n-term fp32 sum in any order, with or without fma (each of at most
    n roundings is relative to a partial sum that sum |terms| bounds; + 2: the operand that is added to -- the gradient's
    start value -- and first-order slack).  n = k D + 1 (fwd), k C (dgrad), B Tz (dw, db); sum |terms| is the reference on
    absolute values.  No measured constant."""
    B, D, C, Tz, k = case
    mag = results(np.abs(z), np.abs(w), np.abs(bias), np.abs(dout), np.abs(dw0), np.abs(db0))
    n = {'out': k * D + 1, 'dz': k * C, 'dw': B * Tz, 'db': B * Tz}
    return {name: (n[name] + 2) * U * mag[name] for name in mag}
