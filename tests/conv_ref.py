"""Float64 reference of the fp32 conv engine's ABI contract (vqw_conv_gemm / vqw_wgrad_gemm, include/vqwave.h), the seeded
case lists of tests/test_conv_engine_epilogues_gpu.py and the one comparison helper both test files use.

Everything here is numpy on the CPU and is written from the formulas of the header, not from the kernels:

  acc[b][m][t] = sum_j sum_c w[j][c][m] * x[b][c][in_stride*t + tap_shift[j]]      (x = x0|x1, reads outside [0,T_in) = 0)

then one of the five epilogues, stored at out_tstride*t + out_toffset of rows T_store long.  A reference call takes the
caller's buffers as flat arrays, never changes them and returns for every output a float64 COPY with the written positions
replaced, plus the mask of those positions: what the kernel must not touch keeps its old contents and is compared bit for bit.

Operands: every operand is seeded standard normal.  Weights are standard normal too, except for the GATE cases, where they
are scaled by (taps * channels)^-1/2: with unit weights the pre-activations have |v| ~ 15, tanh and sigmoid sit at +-1 / 0 / 1
for nearly every output and a dropped bias or condition would not show.  A single product x*w is then still >= 0.05, far
above every bar.

Bars (tests/test_kernels_gpu.py), each relative to max(1, max |ref|) of the written region, against float64:
conv outputs 2e-4, weight gradients 1e-3, GATE outputs 2e-5."""
import functools

import numpy as np

EPI_STORE, EPI_ACCUM_SPLIT, EPI_GATE, EPI_GATE_BWD, EPI_MASK = range(5)
BAR_CONV, BAR_WGRAD, BAR_GATE = 2e-4, 1e-3, 2e-5
SENTINEL = np.float32(-1234.5)          # NaN-free, far from every value a case computes, exact in fp32
GUARD = 64                              # floats of sentinel on each side of a view (a multiple of 4: 16-byte aligned)
MAX_TAPS = 8


def _f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64).reshape(-1)


def _gather_t(x, idx):
    """x[..., idx] with zeros where idx is outside the last axis."""
    ok = (idx >= 0) & (idx < x.shape[-1])
    out = np.zeros(x.shape[:-1] + (idx.size,))
    out[..., ok] = x[..., idx[ok]]
    return out


class _Outputs:
    """Copies of the caller's output buffers, one per distinct array (two names may share a buffer)."""

    def __init__(self):
        self.by_id = {}

    def of(self, a):
        if id(a) not in self.by_id:
            self.by_id[id(a)] = (_f64(a).copy(), np.zeros(np.asarray(a).size, dtype=bool))
        return self.by_id[id(a)]

    def put(self, a, B, nrows, Ts, rows, pos, vals, add=False):
        """a as [B][nrows][Ts]: rows `rows`, columns `pos` := vals [B][len(rows)][len(pos)]."""
        v, m = self.of(a)
        V, Mk = v[:B * nrows * Ts].reshape(B, nrows, Ts), m[:B * nrows * Ts].reshape(B, nrows, Ts)
        ix = (slice(None), np.asarray(rows)[:, None], np.asarray(pos)[None, :])
        V[ix] = V[ix] + vals if add else vals
        Mk[ix] = True


def conv_acc(*, x0, w, B, T_in, T_out, M, C0, taps, x1=None, C1=0, in_stride=1, ldw=None, in_relu=False, w_tap_stride=0, **_):
    """The accumulator acc[b][m][t] of the header's formula, float64."""
    ldw = M if ldw is None else ldw
    C = C0 + C1
    wts = w_tap_stride if w_tap_stride > 0 else C * ldw
    x = _f64(x0)[:B * C0 * T_in].reshape(B, C0, T_in)
    if C1:
        x = np.concatenate([x, _f64(x1)[:B * C1 * T_in].reshape(B, C1, T_in)], axis=1)
    if in_relu:
        x = np.maximum(x, 0.0)
    wf = _f64(w)
    t = np.arange(T_out)
    acc = np.zeros((B, M, T_out))
    for j, s in enumerate(taps):
        wj = wf[j * wts + np.arange(C)[:, None] * ldw + np.arange(M)[None, :]]
        acc += np.einsum('cm,bct->bmt', wj, _gather_t(x, in_stride * t + int(s)))
    return acc


def conv_ref(*, x0, w, B, T_in, T_out, M, C0, taps, out0, x1=None, C1=0, in_stride=1, ldw=None, in_relu=False,
             epilogue=EPI_STORE, out_relu=False, M0=0, out_tstride=1, out_toffset=0, T_store=0, cond=None, cond_T=0,
             cond_bstride=0, w_tap_stride=0, bias=None, scale=None, shift=None, aux0=None, aux1=None, out1=None,
             save0=None, save1=None, split_k=0, tile=0):
    """vqw_conv_gemm on flat buffers -> {name: (float64 copy of the buffer after the call, mask of the written positions)}
    for every output given.  Names that share one buffer share one entry.  `tile` is accepted and ignored (it must not
    change the result).  split_k > 1: out0 is zeroed first, as the header says; split_k < 0: the result is added to what
    the caller left there."""
    acc = conv_acc(x0=x0, w=w, B=B, T_in=T_in, T_out=T_out, M=M, C0=C0, taps=taps, x1=x1, C1=C1, in_stride=in_stride,
                   ldw=ldw, in_relu=in_relu, w_tap_stride=w_tap_stride)
    out_tstride = out_tstride if out_tstride > 0 else 1
    Ts = T_store if T_store > 0 else out_tstride * T_out
    t = np.arange(T_out)
    pos = out_tstride * t + out_toffset
    assert pos.max() < Ts
    O = _Outputs()

    def rows_of(a, nrows):                      # the caller's ORIGINAL values at the store positions, [B][nrows][T_out]
        return _f64(a)[:B * nrows * Ts].reshape(B, nrows, Ts)[:, :, pos]

    def per_row(a, r0=0, n=M):
        return 0.0 if a is None else _f64(a)[r0:r0 + n][None, :, None]

    cv = 0.0
    if cond_T > 0:
        assert T_out % cond_T == 0
        bs = cond_bstride if cond_bstride else M * cond_T
        ix = np.arange(B)[:, None, None] * bs + np.arange(M)[None, :, None] * cond_T + (t // (T_out // cond_T))[None, None, :]
        cv = _f64(cond)[ix]
    allrows = np.arange(M)
    if epilogue == EPI_STORE:
        m0 = M0 if (0 < M0 <= M and out1 is not None) else M
        r = acc + per_row(bias) + cv
        if out_relu:
            r = np.maximum(r, 0.0)
        if save0 is not None:
            O.put(save0, B, M, Ts, allrows, pos, r)
        v = per_row(scale) * r + per_row(shift) if scale is not None else r
        if aux1 is not None:
            v = v + rows_of(aux1, M)
        if split_k > 1:
            z, zm = O.of(out0)
            z[:B * M * Ts] = 0.0
            zm[:B * M * Ts] = True
        O.put(out0, B, m0, Ts, allrows[:m0], pos, v[:, :m0], add=(split_k > 1 or split_k < 0))
        if m0 < M:
            O.put(out1, B, M - m0, Ts, allrows[:M - m0], pos, v[:, m0:])
    elif epilogue == EPI_ACCUM_SPLIT:
        m0 = min(max(M0, 0), M)
        v = acc + per_row(bias)
        if m0:
            O.put(out0, B, m0, Ts, allrows[:m0], pos, rows_of(out0, m0) + v[:, :m0])
        if m0 < M:
            O.put(out1, B, M - m0, Ts, allrows[:M - m0], pos, rows_of(aux1, M - m0) + v[:, m0:])
    elif epilogue == EPI_GATE:
        H = M // 2
        v = acc + per_row(bias) + cv
        th, sg = np.tanh(v[:, :H]), 1.0 / (1.0 + np.exp(-v[:, H:]))
        O.put(out0, B, H, Ts, allrows[:H], pos, th * sg)
        if save0 is not None:
            O.put(save0, B, H, Ts, allrows[:H], pos, th)
        if save1 is not None:
            O.put(save1, B, H, Ts, allrows[:H], pos, sg)
    elif epilogue == EPI_GATE_BWD:
        th, sg = rows_of(aux0, M), rows_of(aux1, M)
        O.put(out0, B, 2 * M, Ts, allrows, pos, acc * sg * (1.0 - th * th))
        O.put(out0, B, 2 * M, Ts, M + allrows, pos, acc * th * sg * (1.0 - sg))
    elif epilogue == EPI_MASK:
        v = acc * (per_row(scale) if scale is not None else 1.0)
        O.put(out0, B, M, Ts, allrows, pos, np.where(rows_of(aux0, M) > 0, v, 0.0))
    else:
        raise ValueError('unknown epilogue %r' % (epilogue,))
    return {n: O.of(a) for n, a in (('out0', out0), ('out1', out1), ('save0', save0), ('save1', save1)) if a is not None}


def wgrad_ref(*, p, q0, dw, B, T_q, T_p, Cp, Q0, taps, q1=None, Q1=0, p_stride=1, p_relu=False, lddw=None,
              dw_tap_stride=None, splits=0):
    """vqw_wgrad_gemm: dw[j][c][o] += sum_{b,t<T_q} p[b][c][p_stride*t + taps[j]] * q[b][o][t], q = q0|q1
    -> (float64 copy of dw after the call, mask of the positions added to).  `splits` must not change the result."""
    Q = Q0 + Q1
    lddw = Q if lddw is None else lddw
    dts = Cp * lddw if dw_tap_stride is None else dw_tap_stride
    P = _f64(p)[:B * Cp * T_p].reshape(B, Cp, T_p)
    if p_relu:
        P = np.maximum(P, 0.0)
    q = _f64(q0)[:B * Q0 * T_q].reshape(B, Q0, T_q)
    if Q1:
        q = np.concatenate([q, _f64(q1)[:B * Q1 * T_q].reshape(B, Q1, T_q)], axis=1)
    out, mask = _f64(dw).copy(), np.zeros(np.asarray(dw).size, dtype=bool)
    t = np.arange(T_q)
    for j, s in enumerate(taps):
        ix = j * dts + np.arange(Cp)[:, None] * lddw + np.arange(Q)[None, :]
        out[ix] += np.einsum('bct,bot->co', _gather_t(P, p_stride * t + int(s)), q)
        mask[ix] = True
    return out, mask


# ---------------------------------------------------------------------------------------------------- comparison
def check(got_buffers, ref_buffers, guards, bar=BAR_CONV, what=''):
    """The project's single bar on the written region, bit-equality everywhere else.

    got_buffers {name: fp32 array, the WHOLE buffer with its guard bands}; ref_buffers {name: float64 array of the same
    size: the reference where the kernel writes, the buffer's old contents elsewhere}; guards {name: bool array, True where
    the kernel must not write: guard bands, the other stride phase, rows and columns of a wider matrix}.
    Returns the worst err / (bar * max(1, max |ref|)) over the buffers."""
    worst = 0.0
    for name in sorted(ref_buffers):
        g = np.asarray(got_buffers[name]).reshape(-1)
        r = np.asarray(ref_buffers[name], dtype=np.float64).reshape(-1)
        keep = np.asarray(guards[name], dtype=bool).reshape(-1)
        assert g.dtype == np.float32 and g.size == r.size == keep.size, '%s %s: buffer sizes differ' % (what, name)
        same = g[keep].view(np.uint32) == r[keep].astype(np.float32).view(np.uint32)
        assert same.all(), '%s %s: %d of %d positions the kernel must not touch changed (first: element %d, %r -> %r)' % (
            what, name, int((~same).sum()), int(keep.sum()), int(np.flatnonzero(keep)[np.argmin(same)]),
            float(r[keep][np.argmin(same)]), float(g[keep][np.argmin(same)]))
        wr = ~keep
        if not wr.any():
            continue
        scale = max(1.0, float(np.abs(r[wr]).max()))
        d = np.abs(g[wr].astype(np.float64) - r[wr])
        err = float(d.max()) if np.isfinite(d).all() else float('inf')
        assert err <= bar * scale, '%s %s: max abs err %.3e > %.1e * %.3e (written element %d: got %r, want %r)' % (
            what, name, err, bar, scale, int(np.argmax(d)), float(g[wr][np.argmax(d)]), float(r[wr][np.argmax(d)]))
        worst = max(worst, err / (bar * scale))
    return worst


# ---------------------------------------------------------------------------------------------------- buffers
class Buf:
    """n floats inside a sentinel-filled buffer: GUARD floats in front (+ `off`, 0 = 16-byte aligned start, 1 = not) and behind."""

    def __init__(self, n, off=0, init=None):
        self.n, self.lo = n, GUARD + off
        self.full = np.full(GUARD + off + n + GUARD, SENTINEL, dtype=np.float32)
        self.view = self.full[self.lo:self.lo + n]
        if init is not None:
            self.view[:] = np.asarray(init, dtype=np.float32).reshape(-1)

    def expected(self, vals, mask):
        """(ref, guard) of the whole buffer for check() from the reference's (values, mask) of the view."""
        ref = self.full.astype(np.float64)
        ref[self.lo:self.lo + self.n] = vals
        keep = np.ones(self.full.size, dtype=bool)
        keep[self.lo:self.lo + self.n] = ~mask
        return ref, keep


def randn(seed, *shape):
    return np.random.RandomState(seed).standard_normal(shape).astype(np.float32)


def with_zeros(a, seed):
    """Exact zeros on a seeded tenth of a (both signs stay): what relu and MASK have to get right."""
    a = a.copy()
    a.reshape(-1)[np.random.RandomState(seed).rand(a.size) < 0.1] = 0.0
    return a


# ---------------------------------------------------------------------------------------------------- cases
MAIN_TILES = (11, 12, 14, 21, 22, 24)
TILES = (0,) + MAIN_TILES + (10012, 10014, 20022, 10024)            # tile + 10000*n: n main-tile columns go to half-width tiles
GATE_TILES = (0, 21, 22, 24, 20022, 10024)
FAMILIES = ('store', 'accum_split', 'gate', 'gate_bwd', 'mask', 'strides', 'split_k')
EPILOGUE_FAMILIES = ('store', 'accum_split', 'gate', 'gate_bwd', 'mask')


def same_pads(n, k, s):
    out = -(-n // s)
    total = max((out - 1) * s + k - n, 0)
    return total // 2, total - total // 2


def _case(fam, name, B, T, C0, M, taps, **kw):
    c = dict(fam=fam, name='%s/%s' % (fam, name), B=B, T_in=T, T_out=T, C0=C0, C1=0, M=M, taps=list(taps), epilogue=EPI_STORE,
             in_stride=1, ldw=None, woff=0, w_tap_stride=0, in_relu=False, out_relu=False, M0=0, out_tstride=1, out_toffset=0,
             T_store=0, cond_T=0, cond_off=0, cond_pad=0, split_k=0,
             bias=False, affine=False, aux1=False, save0=False, save1=False, out1=False,
             alias=(),           # names of operands that are ONE buffer, e.g. ('aux0', 'out0')
             twice=False,        # the launch is repeated on its own result (accumulation)
             zeroed=False,       # out0 starts as zeros (split_k < 0), not as sentinels
             phases=None)        # strided gradient: [(T_out, out_toffset, woff, taps)] launches into one out0
    c.update(kw)
    return c


def _store_cases():
    opts = ('bias', 'cond', 'out_relu', 'save0', 'affine', 'aux1', 'split', 'in_relu')
    shapes = [dict(B=2, T=260, C0=32, M=132, taps=(-3, 0), ratio=4, M0=36),
              dict(B=3, T=100, C0=16, M=68, taps=(-1, 0, 1), ratio=20, M0=64),
              dict(B=1, T=777, C0=48, M=36, taps=(-64, -32, 0), ratio=777, M0=4)]

    def mk(name, on, s, **over):
        kw = {}
        if 'cond' in on:
            kw.update(cond_T=s['T'] // s['ratio'], cond_off=4, cond_pad=3)
        if 'split' in on:
            kw.update(M0=s['M0'], out1=True)
        for o in ('bias', 'out_relu', 'save0', 'affine', 'aux1', 'in_relu'):
            if o in on:
                kw[o] = True
        kw.update(over)
        return _case('store', name, s['B'], s['T'], s['C0'], s['M'], s['taps'], **kw)

    cases = [mk(o, (o,), shapes[i % 3]) for i, o in enumerate(opts)]
    cases += [mk('all/%d' % i, opts, s) for i, s in enumerate(shapes)]
    # all options on the remaining shapes: T_out < 64 with one 4-row M tile, an interior LDS-DMA shape, two sources with
    # all but one tap outside the signal, one condition frame
    cases.append(mk('all/T37', opts, dict(B=2, T=37, C0=96, M=4, taps=(-1, 0), ratio=37, M0=0), out1=False))
    cases.append(mk('all/T1024', tuple(o for o in opts if o != 'in_relu'), dict(B=1, T=1024, C0=32, M=100, taps=(-2, -1, 0), ratio=4, M0=36)))
    cases.append(mk('all/two_sources', opts, dict(B=2, T=260, C0=16, M=132, taps=(-600, -300, 0), ratio=20, M0=100), C1=16))
    cases.append(mk('all/T255', opts, dict(B=2, T=255, C0=32, M=68, taps=(-5, 0), ratio=255, M0=20)))
    cases.append(mk('all/T250', opts, dict(B=1, T=250, C0=16, M=100, taps=(-300, -7, 0), ratio=50, M0=68)))
    return cases


def _accum_cases():
    A = functools.partial(_case, 'accum_split', epilogue=EPI_ACCUM_SPLIT, bias=True)
    return [
        A('split36/out_of_place', 2, 260, 32, 132, (0,), M0=36, out1=True, aux1=True),
        A('split20/in_place/3taps', 3, 100, 16, 68, (-2, -1, 0), M0=20, out1=True, aux1=True, alias=('aux1', 'out1')),
        A('M0=0/out0_is_out1', 2, 255, 32, 100, (2, 1, 0), M0=0, out1=True, aux1=True, alias=('out0', 'out1')),
        A('M0=0/all_one_buffer', 1, 777, 16, 36, (0,), M0=0, out1=True, aux1=True, alias=('out0', 'out1', 'aux1')),
        A('M0=M', 1, 777, 48, 36, (-1, 0, 1), M0=36),
        A('M0=0/weight_view', 2, 250, 32, 36, (0,), M0=0, out1=True, aux1=True, alias=('out0', 'out1'), ldw=136, woff=100),
        A('M0=0/weight_view/T777', 1, 777, 16, 68, (0,), M0=0, out1=True, aux1=True, alias=('out0', 'out1'), ldw=168, woff=100),
        A('split36/twice', 2, 250, 16, 100, (0,), M0=36, out1=True, aux1=True, twice=True),
        A('M0=0/T37', 2, 37, 96, 4, (0,), M0=0, out1=True, aux1=True, alias=('out0', 'out1', 'aux1'), bias=False),
        A('split100/in_place/T1024', 1, 1024, 32, 132, (-4, -2, 0), M0=100, out1=True, aux1=True, alias=('aux1', 'out1')),
    ]


def _gate_cases():
    G = functools.partial(_case, 'gate', epilogue=EPI_GATE)
    cd = dict(cond_off=8, cond_pad=5)
    return [
        G('H4/all', 2, 37, 16, 8, (-2, -1, 0), bias=True, cond_T=1, save0=True, save1=True, **cd),
        G('H36/cond/save0', 3, 100, 32, 72, (-4, -2, 0), cond_T=5, save0=True, **cd),
        G('H68/bias/save1', 2, 260, 48, 136, (-1, 0), bias=True, save1=True),
        G('H100/all', 1, 777, 16, 200, (-300, -150, 0), bias=True, cond_T=37, save0=True, save1=True, **cd),
        G('H132/all', 2, 260, 32, 264, (-2, -1, 0), bias=True, cond_T=65, save0=True, save1=True, **cd),
        G('H132/plain/T1024', 1, 1024, 16, 264, (-8, -4, 0)),
        G('H36/one_frame', 2, 255, 96, 72, (0,), bias=True, cond_T=1, **cd),
        G('H100/ratio10/T250', 2, 250, 16, 200, (-1, 0), cond_T=25, save0=True, save1=True, **cd),
    ]


def _gate_bwd_cases():
    G = functools.partial(_case, 'gate_bwd', epilogue=EPI_GATE_BWD)
    return [
        G('M36', 2, 260, 64, 36, (0,)),
        G('M100/two_sources', 3, 100, 32, 100, (0,), C1=16),
        G('M36/two_sources/T777', 1, 777, 16, 36, (0,), C1=32),
        G('M100/T37', 2, 37, 48, 100, (0,)),
        G('M100/two_sources/T1024', 1, 1024, 16, 100, (0,), C1=16),
        G('M36/two_sources/T255', 2, 255, 32, 36, (1, 0), C1=32),
        G('M100/T250', 1, 250, 96, 100, (0,)),
    ]


def _mask_cases():
    K = functools.partial(_case, 'mask', epilogue=EPI_MASK)
    ip = dict(alias=('aux0', 'out0'))
    return [
        K('in_place/scale', 2, 260, 32, 132, (0,), affine=True, **ip),
        K('out_of_place', 3, 100, 16, 68, (0,)),
        K('in_place', 1, 777, 48, 36, (0,), **ip),
        K('out_of_place/scale/T37', 2, 37, 16, 4, (0,), affine=True),
        K('in_place/scale/T1024', 1, 1024, 32, 100, (-1, 0), affine=True, **ip),
        K('out_of_place/scale/T255', 2, 255, 96, 132, (0,), affine=True),
        K('in_place/T250', 2, 250, 16, 68, (0,), **ip),
    ]


def _stride_cases():
    S = functools.partial(_case, 'strides')
    cases = []
    for T_in, k, M in ((250, 5, 68), (255, 4, 36), (256, 5, 132), (777, 4, 100)):      # Keras 'same', stride 2; 777: interior blocks
        pl, _ = same_pads(T_in, k, 2)
        cases.append(S('fwd/Tin%d/k%d' % (T_in, k), 2, T_in, 32, M, [j - pl for j in range(k)], T_out=-(-T_in // 2), in_stride=2,
                       bias=True, out_relu=True))
    # the stride-2 input gradient as the encoders issue it: output times tau = 2u + p get the taps j = p + pad_left (mod 2)
    # of the per-tap transposed kernel wT[k][F][F], one launch per parity p
    for T_in, k, F, B, split in ((255, 5, 32, 2, 0), (250, 4, 48, 3, 0), (255, 4, 32, 2, -3), (250, 5, 48, 1, -2), (37, 5, 16, 2, 0),
                                 (777, 5, 64, 1, 0)):             # a full M tile and interior blocks: the LDS-DMA loop on strided taps
        pl, _ = same_pads(T_in, k, 2)
        ph = []
        for p in (0, 1):
            j0 = (p + pl) % 2
            ph.append(((T_in - p + 1) // 2, p, j0 * F * F, [(p + pl - j) // 2 for j in range(j0, k, 2)]))
        cases.append(S('dgrad/Tin%d/k%d/split%d' % (T_in, k, split), B, -(-T_in // 2), F, F, (), phases=ph, out_tstride=2,
                       T_store=T_in, w_tap_stride=2 * F * F, wtaps=k, split_k=split, zeroed=split < 0))
    # one phase only (a 1x1 stride-2 conv's gradient): the odd positions must keep their contents
    cases.append(S('dgrad/even_phase_only', 2, 128, 32, 68, (0,), out_tstride=2, T_store=255))
    cases.append(S('dgrad/odd_phase/toffset1', 1, 125, 16, 36, (-1, 0), out_tstride=2, out_toffset=1, T_store=250))
    return cases


def _split_k_cases():
    S = functools.partial(_case, 'split_k', bias=True)
    cases = [S('auto', 2, 104, 1024, 80, (0,))]          # nblocks * 2 <= CUs and 64 K-steps: the automatic branch
    for n in (2, 7, 50):                                 # 9 K-steps; some taps lie outside some tiles
        cases.append(S('forced%d' % n, 3, 260, 48, 132, (-200, -100, 0), split_k=n))
    cases.append(S('forced7/T777', 1, 777, 96, 36, (-1, 0), split_k=7))
    cases.append(S('forced2/T37/no_bias', 2, 37, 32, 4, (-40, 0), split_k=2, bias=False))
    return cases


@functools.lru_cache(maxsize=None)
def conv_base_cases():
    cases = _store_cases() + _accum_cases() + _gate_cases() + _gate_bwd_cases() + _mask_cases() + _stride_cases() + _split_k_cases()
    for i, c in enumerate(cases):
        c['seed'] = 1000 + 17 * i
    assert len({c['name'] for c in cases}) == len(cases)
    return tuple(cases)


def tiles_of(c):
    if c['fam'] == 'gate':
        return GATE_TILES
    if c['name'] == 'split_k/auto':
        return (0, 12, 22)
    return TILES


def conv_cases():
    """[(base case, tile)]: every base case on every tile its epilogue allows."""
    return [(c, t) for c in conv_base_cases() for t in tiles_of(c)]


def case_id(c, tile):
    return '%s-tile%d' % (c['name'], tile)


def tile_geometry(c, tile):
    """(M tiles, rows in the last M tile, rows per M tile, columns per main tile, tail columns) of a case on an explicit tile."""
    mt, nt = (tile % 100) // 10, tile % 10
    rows = c['M'] // 2 if c['epilogue'] == EPI_GATE else c['M']
    bm = 32 * mt if c['epilogue'] == EPI_GATE else 64 * mt
    n_mt = -(-rows // bm)
    return n_mt, rows - (n_mt - 1) * bm, bm, 64 * nt, tile // 10000


def launches_of(c):
    """The launches of a case as dicts of the integer arguments that differ between them."""
    if c['phases']:
        return [dict(T_out=To, out_toffset=p, woff=wo, taps=tp) for To, p, wo, tp in c['phases']]
    return [dict(T_out=c['T_out'], out_toffset=c['out_toffset'], woff=c['woff'], taps=c['taps'])] * (2 if c['twice'] else 1)


def geometry(c):
    """Derived sizes of a case: row length, rows per output, weight-view and condition sizes."""
    C = c['C0'] + c['C1']
    M = c['M']
    ldw = M if c['ldw'] is None else c['ldw']
    wts = c['w_tap_stride'] if c['w_tap_stride'] > 0 else C * ldw
    Ts = c['T_store'] if c['T_store'] > 0 else c['out_tstride'] * c['T_out']
    ntaps_w = c.get('wtaps', len(c['taps']))
    w_len = max(L['woff'] + (len(L['taps']) - 1) * wts + (C - 1) * ldw + M for L in launches_of(c))
    w_len = max(w_len, ntaps_w * C * ldw)
    epi = c['epilogue']
    if epi == EPI_STORE:
        m0 = c['M0'] if (0 < c['M0'] <= M and c['out1']) else M
    elif epi == EPI_ACCUM_SPLIT:
        m0 = min(max(c['M0'], 0), M)
    else:
        m0 = M
    rows = dict(out0={EPI_GATE: M // 2, EPI_GATE_BWD: 2 * M}.get(epi, m0), out1=M - m0, aux1=M, aux0=M, save0=M, save1=M)
    if epi == EPI_ACCUM_SPLIT:
        rows['aux1'] = M - m0
    if epi == EPI_GATE:
        rows['save0'] = rows['save1'] = M // 2
    bs = M * c['cond_T'] + c['cond_pad']
    return dict(C=C, ldw=ldw, wts=wts, Ts=Ts, w_len=w_len, m0=m0, rows=rows, cond_bstride=bs if c['cond_T'] else 0,
                cond_len=c['cond_off'] + c['B'] * bs)


def legality(c, tile):
    """The wrapper's and the ABI's preconditions a case must meet; a list of the violations (empty = legal)."""
    g, bad = geometry(c), []
    if c['C0'] <= 0 or c['C0'] % 16 or c['C1'] % 16:
        bad.append('C0 / C1 must be multiples of 16')
    if c['M'] % 4 or (c['epilogue'] == EPI_GATE and c['M'] % 8):
        bad.append('M must be a multiple of 4 (GATE: 8)')
    if g['ldw'] % 4 or g['ldw'] < c['M']:
        bad.append('ldw must be a multiple of 4 and >= M')
    if c['cond_T'] and c['T_out'] % c['cond_T']:
        bad.append('T_out must be a multiple of cond_T')
    if c['cond_T'] and g['cond_bstride'] <= c['M'] * c['cond_T']:
        bad.append('the condition comes with a batch stride above M * cond_T')
    if c['in_stride'] not in (1, 2):
        bad.append('in_stride')
    for L in launches_of(c):
        if L['woff'] % 4:
            bad.append('the weight view must start 16-byte aligned')
        if not 1 <= len(L['taps']) <= MAX_TAPS:
            bad.append('1..8 taps')
        if c['out_tstride'] * (L['T_out'] - 1) + L['out_toffset'] >= g['Ts']:
            bad.append('the last store index must lie inside the row')
        if L['woff'] + (len(L['taps']) - 1) * g['wts'] + (g['C'] - 1) * g['ldw'] + c['M'] > g['w_len']:
            bad.append('weight view too short')
    if g['wts'] % 4:
        bad.append('w_tap_stride must keep the taps 16-byte aligned')
    mt, nt = (tile % 100) // 10, tile % 10
    if tile and (mt not in (1, 2) or nt not in (1, 2, 4)):
        bad.append('unsupported tile')
    if tile >= 10000 and nt == 1:
        bad.append('tail tiles need NT > 1')
    if c['epilogue'] == EPI_GATE and tile and mt != 2:
        bad.append('GATE needs an MT=2 tile')
    if c['split_k'] and (c['epilogue'] != EPI_STORE or c['out_relu'] or c['affine'] or c['cond_T'] or c['save0'] or c['aux1'] or c['out1']):
        bad.append('split_k needs the plain STORE epilogue')
    if c['split_k'] < 0 and not c['zeroed']:
        bad.append('split_k < 0 needs a zeroed out0')
    for a in c['alias']:
        if a not in ('out0', 'out1', 'aux0', 'aux1'):
            bad.append('alias of %s' % a)
    if len(c['alias']) > 1 and len({g['rows'][a] for a in c['alias']}) != 1 and not (c['epilogue'] == EPI_ACCUM_SPLIT and g['m0'] == 0):
        bad.append('aliased operands of different sizes')
    return bad


def build_conv(c, off):
    """The operands of a case: ({name: fp32 array} of the inputs, {name: Buf} of the outputs and in-place operands).  Output
    buffers start at GUARD + off floats into a sentinel-filled allocation; aliased names are one Buf."""
    g, s, B, M = geometry(c), c['seed'], c['B'], c['M']
    K = len(c['taps']) if c['taps'] else len(c['phases'][0][3]) * 2
    ins = dict(x0=randn(s, B, c['C0'], c['T_in']))
    if c['C1']:
        ins['x1'] = randn(s + 1, B, c['C1'], c['T_in'])
    if c['in_relu']:
        ins['x0'] = with_zeros(ins['x0'], s + 20)
    ins['w'] = randn(s + 2, g['w_len']) * np.float32((K * g['C']) ** -0.5 if c['epilogue'] == EPI_GATE else 1.0)
    if c['bias']:
        ins['bias'] = randn(s + 3, M)
    if c['affine']:
        ins['scale'] = randn(s + 4, M)
        if c['epilogue'] == EPI_STORE:
            ins['shift'] = randn(s + 5, M)
    if c['cond_T']:
        ins['cond'] = randn(s + 6, g['cond_len'])
    bufs = {}
    Ts = g['Ts']

    def init_of(name):
        n = B * g['rows'][name] * Ts
        if c['epilogue'] == EPI_GATE_BWD and name in ('aux0', 'aux1'):
            v = randn(s + 7 + (name == 'aux1'), n).astype(np.float64)
            return np.tanh(v) if name == 'aux0' else 1.0 / (1.0 + np.exp(-v))
        if name == 'aux0':
            return with_zeros(randn(s + 9, n), s + 21)             # MASK: exact zeros and both signs
        if name == 'aux1':
            return randn(s + 10, n)
        if name == 'out0' and c['epilogue'] == EPI_ACCUM_SPLIT:
            return randn(s + 11, n)                                # the running skip sum
        if name == 'out0' and c['zeroed']:
            return np.zeros(n, np.float32)
        return None                                                # a pure output: sentinels

    used = ['out0']
    used += ['out1'] if c['out1'] else []
    used += ['aux0'] if c['epilogue'] in (EPI_GATE_BWD, EPI_MASK) else []
    used += ['aux1'] if (c['aux1'] or c['epilogue'] == EPI_GATE_BWD) else []
    used += [n for n in ('save0', 'save1') if c[n]]
    for name in used:
        group = list(c['alias']) if name in c['alias'] else [name]
        made = [a for a in group if a in bufs]
        if made:
            bufs[name] = bufs[made[0]]
            continue
        n = max(B * g['rows'][a] * Ts for a in group)
        init = None
        for a in sorted(group, key=lambda a: a.startswith('out')):   # an input among the aliases gives the contents
            if init is None and B * g['rows'][a] * Ts == n:
                init = init_of(a)
        bufs[name] = Buf(n, off, init)
    return ins, bufs


def conv_kwargs(c, L, tile=0):
    """The integer arguments of launch L of case c for kernels.conv_gemm / conv_ref."""
    g = geometry(c)
    return dict(B=c['B'], T_in=c['T_in'], T_out=L['T_out'], M=c['M'], C0=c['C0'], C1=c['C1'], taps=L['taps'],
                in_stride=c['in_stride'], ldw=g['ldw'], in_relu=c['in_relu'], epilogue=c['epilogue'], out_relu=c['out_relu'],
                M0=c['M0'], out_tstride=c['out_tstride'], out_toffset=L['out_toffset'], T_store=c['T_store'],
                cond_T=c['cond_T'], cond_bstride=g['cond_bstride'], w_tap_stride=c['w_tap_stride'], split_k=c['split_k'], tile=tile)


def conv_operands(c, L, ins, views):
    """The array arguments of launch L: `ins` as built (on any device), `views` {name: the view of each Buf}."""
    kw = dict(x0=ins['x0'], x1=ins.get('x1'), w=ins['w'][L['woff']:], bias=ins.get('bias'), scale=ins.get('scale'),
              shift=ins.get('shift'), cond=ins['cond'][c['cond_off']:] if c['cond_T'] else None)
    for n in ('out0', 'out1', 'aux0', 'aux1', 'save0', 'save1'):
        kw[n] = views.get(n)
    return kw


def conv_expected(c, off, operands=None):
    """Reference of a whole case (all its launches): (ins, bufs, {name: (ref, guard)} for check()).  `operands`: an
    (ins, bufs) pair to use in place of build_conv's."""
    ins, bufs = operands if operands is not None else build_conv(c, off)
    state = {id(b): b.view.copy() for b in bufs.values()}      # one array per Buf: conv_ref sees the aliasing as identity
    masks = {id(b): np.zeros(b.n, dtype=bool) for b in bufs.values()}
    for L in launches_of(c):
        views = {n: state[id(b)] for n, b in bufs.items()}
        res = conv_ref(**conv_kwargs(c, L), **conv_operands(c, L, ins, views))
        for n, (vals, mask) in res.items():                    # the next launch starts from this one's result
            state[id(bufs[n])] = vals
            masks[id(bufs[n])] |= mask
    return ins, bufs, {n: b.expected(state[id(b)], masks[id(b)]) for n, b in bufs.items()}


def bar_of(c):
    return BAR_GATE if c['epilogue'] == EPI_GATE else BAR_CONV


# ---------------------------------------------------------------------------------------------------- wgrad cases
def _wcase(name, B, T_q, Cp, Q0, Q1, taps, **kw):
    c = dict(fam='wgrad', name='wgrad/' + name, B=B, T_q=T_q, T_p=T_q, Cp=Cp, Q0=Q0, Q1=Q1, taps=list(taps), p_stride=1,
             p_relu=False, lddw=None, dw_off=0, dw_tap_stride=None, splits=0, nonzero=False)
    c.update(kw)
    return c


@functools.lru_cache(maxsize=None)
def wgrad_cases():
    pl5, _ = same_pads(255, 5, 2)
    pl4, _ = same_pads(665, 4, 2)
    cases = [
        _wcase('Q64+32/T37', 2, 37, 16, 64, 32, (0,)),
        _wcase('Q100+28/T100/relu', 3, 100, 48, 100, 28, (-4, -2, 0), splits=1, p_relu=True),
        _wcase('Q64+256/T333', 1, 333, 32, 64, 256, (-1, 0), splits=3),
        _wcase('Q128+132/T1000/Cp144', 2, 1000, 144, 128, 132, (0,)),
        _wcase('stride2/Tp255', 2, 128, 32, 68, 0, [j - pl5 for j in range(5)], T_p=255, p_stride=2),
        _wcase('stride2/Tp665/relu', 1, 333, 16, 100, 28, [j - pl4 for j in range(4)], T_p=665, p_stride=2, p_relu=True, splits=3),
        _wcase('stride2/Tp665/Cp128', 1, 333, 128, 132, 0, [j - pl4 for j in range(4)], T_p=665, p_stride=2),   # whole tiles: the fast loop
        _wcase('view/lddw136', 2, 100, 32, 36, 0, (-2, -1, 0), lddw=136, dw_off=100, dw_tap_stride=32 * 136 + 8, nonzero=True),
        _wcase('view/two_sources', 3, 333, 96, 64, 32, (0,), lddw=100, dw_off=3, nonzero=True, splits=1),
        _wcase('accumulate/T1000', 1, 1000, 16, 64, 32, (-64, 0), nonzero=True, splits=1),
        _wcase('Q4/T37/splits3', 2, 37, 16, 4, 0, (-1, 0, 1), splits=3),
        _wcase('Q132/T1000/splits3', 1, 1000, 80, 132, 0, (-300, 0), splits=3),
        _wcase('Q100+28/T100/auto', 2, 100, 96, 100, 28, (0,), nonzero=True),
    ]
    for i, c in enumerate(cases):
        c['seed'] = 5000 + 13 * i
    return tuple(cases)


def wgrad_geometry(c):
    Q = c['Q0'] + c['Q1']
    lddw = Q if c['lddw'] is None else c['lddw']
    dts = c['Cp'] * lddw if c['dw_tap_stride'] is None else c['dw_tap_stride']
    view_len = (len(c['taps']) - 1) * dts + (c['Cp'] - 1) * lddw + Q
    return dict(Q=Q, lddw=lddw, dts=dts, view_len=view_len, n=c['dw_off'] + len(c['taps']) * dts + lddw)


def wgrad_legality(c):
    g, bad = wgrad_geometry(c), []
    if g['lddw'] < g['Q']:
        bad.append('lddw too small')
    if c['p_stride'] not in (1, 2) or not 1 <= len(c['taps']) <= MAX_TAPS:
        bad.append('p_stride / taps')
    if c['dw_off'] + g['view_len'] > g['n']:
        bad.append('dw view outside its matrix')
    if g['dts'] < (c['Cp'] - 1) * g['lddw'] + g['Q']:
        bad.append('taps of dw overlap')
    return bad


def build_wgrad(c, off):
    s, B, g = c['seed'], c['B'], wgrad_geometry(c)
    p = randn(s, B, c['Cp'], c['T_p'])
    ins = dict(p=with_zeros(p, s + 9) if c['p_relu'] else p, q0=randn(s + 1, B, c['Q0'], c['T_q']))
    if c['Q1']:
        ins['q1'] = randn(s + 2, B, c['Q1'], c['T_q'])
    # the whole wider matrix is the Buf: what lies between the view's columns must stay as it is
    dw = Buf(g['n'], off, randn(s + 3, g['n']) if c['nonzero'] else np.zeros(g['n'], np.float32))
    return ins, dw


def wgrad_kwargs(c):
    g = wgrad_geometry(c)
    return dict(B=c['B'], T_q=c['T_q'], T_p=c['T_p'], Cp=c['Cp'], Q0=c['Q0'], Q1=c['Q1'], taps=c['taps'], p_stride=c['p_stride'],
                p_relu=c['p_relu'], lddw=g['lddw'], dw_tap_stride=g['dts'], splits=c['splits'])


def wgrad_expected(c, off):
    ins, dw = build_wgrad(c, off)
    o = c['dw_off']
    vals, mask = wgrad_ref(p=ins['p'], q0=ins['q0'], q1=ins.get('q1'), dw=dw.view[o:], **wgrad_kwargs(c))
    full_vals, full_mask = dw.view.astype(np.float64), np.zeros(dw.n, dtype=bool)
    full_vals[o:], full_mask[o:] = vals, mask
    return ins, dw, dw.expected(full_vals, full_mask)
