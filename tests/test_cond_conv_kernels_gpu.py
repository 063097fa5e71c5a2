"""GPU tests of the conditioning conv's kernels (csrc/cond_conv.hip) against the float64 restatement
(tests/cond_conv_ref.py): exact on small integers, inside the rounding bound of an n-term fp32 sum on random operands, row by
row independent, the same bits from two launches, gradients added to a start value, and every refusal of the header.  Every
operand sits between sentinels, activations in buffers with more rows than the kernels use (batch strides larger than the
rows): whatever the kernels do not own is compared bit for bit afterwards."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cond_conv_ref as CR  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = np.float32(-12345.5)
PAD = 96
GAP_ROWS = 5            # rows behind the ones the kernels use: the speaker rows of a condition buffer


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


class Guarded:
    """vals on the device between PAD sentinels; 3-D vals with gap=True: the first rows of a [B][rows + GAP_ROWS][Tz] buffer."""

    def __init__(self, vals, gap=False):
        vals = np.asarray(vals, np.float32)
        shape = (vals.shape[0], vals.shape[1] + GAP_ROWS, vals.shape[2]) if gap else vals.shape
        n = math.prod(shape)
        self.host = np.full(n + 2 * PAD, SENTINEL, np.float32)
        self.mask = np.zeros(n + 2 * PAD, bool)
        sel = (slice(None), slice(0, vals.shape[1])) if gap else Ellipsis
        self.host[PAD:PAD + n].reshape(shape)[sel] = vals
        self.mask[PAD:PAD + n].reshape(shape)[sel] = True
        self.dev = torch.from_numpy(self.host).cuda()
        self.t = self.dev[PAD:PAD + n].view(shape)
        self.bstride = shape[1] * shape[2] if gap else 0
        self.shape = vals.shape

    def values(self):
        return self.dev.cpu().numpy()[self.mask].reshape(self.shape)

    def rest_untouched(self):
        return np.array_equal(bits(self.dev.cpu().numpy()[~self.mask]), bits(self.host[~self.mask]))

    def untouched(self):
        return np.array_equal(bits(self.dev.cpu().numpy()), bits(self.host))


def launch(K, case, ops):
    """All three kernels on guarded operands -> {'out', 'dz', 'dw', 'db'} (numpy); asserts what must stay as it was."""
    B, D, C, Tz, k = case
    z, w, bias, dout, dw0, db0 = ops
    gz, gw, gb, gg = Guarded(z, gap=True), Guarded(w), Guarded(bias), Guarded(dout, gap=True)
    go, gdz = Guarded(np.full((B, C, Tz), SENTINEL), gap=True), Guarded(np.full((B, D, Tz), SENTINEL), gap=True)
    gdw, gdb = Guarded(dw0), Guarded(db0)
    gs = Guarded(np.full((K.cond_conv_wgrad_scratch(B, D, C, Tz, k),), SENTINEL))
    K.cond_conv_fwd(gz.t, gw.t, gb.t, go.t, z_bstride=gz.bstride, out_bstride=go.bstride)
    K.cond_conv_dgrad(gw.t, gg.t, gdz.t, dout_bstride=gg.bstride, dz_bstride=gdz.bstride)
    K.cond_conv_wgrad(gz.t, gg.t, gdw.t, gdb.t, gs.t, z_bstride=gz.bstride, dout_bstride=gg.bstride)
    torch.cuda.synchronize()
    for name, g in (('z', gz), ('w', gw), ('bias', gb), ('dout', gg)):
        assert g.untouched(), '%s was written' % name
    for name, g in (('out', go), ('dz', gdz), ('dw', gdw), ('db', gdb), ('scratch', gs)):
        assert g.rest_untouched(), 'the surroundings of %s were written' % name
    assert not (bits(gs.values()) == bits(SENTINEL)).any(), 'scratch is larger than what the kernel writes'
    return {'out': go.values(), 'dz': gdz.values(), 'dw': gdw.values(), 'db': gdb.values()}


@pytest.mark.parametrize('case', CR.CASES, ids=CR.case_id)
def test_exact_on_small_integers(K, case):
    """|operands| <= 8: every partial sum is an integer below 2^24, so all four outputs equal the reference exactly (the
    gradients on top of a non-zero start value); a second launch gives the same bits."""
    ops = CR.operands(case, 'exact')
    want = CR.results(*ops)
    got, again = launch(K, case, ops), launch(K, case, ops)
    for name in want:
        assert not (bits(got[name]) == bits(SENTINEL)).any(), '%s: an element was not written' % name
        assert np.array_equal(got[name].astype(np.float64), want[name]), name
        assert np.array_equal(bits(got[name]), bits(again[name])), '%s: two launches differ' % name


@pytest.mark.parametrize('case', CR.CASES, ids=CR.case_id)
def test_random_inside_the_fp32_sum_bound(K, case):
    """|got - ref64| <= (n + 2) 2^-24 sum |terms| per element (cond_conv_ref.bars); two launches give the same bits."""
    ops = CR.operands(case, 'random')
    want, bar = CR.results(*ops), CR.bars(case, *ops)
    got, again = launch(K, case, ops), launch(K, case, ops)
    for name in want:
        err = np.abs(got[name].astype(np.float64) - want[name])
        worst = float((err / bar[name]).max())
        print('%s %s: worst error / bar %.3f' % (CR.case_id(case), name, worst))
        assert (err <= bar[name]).all(), '%s: %.3f of the bar' % (name, worst)
        assert np.array_equal(bits(got[name]), bits(again[name])), '%s: two launches differ' % name


@pytest.mark.parametrize('case', [c for c in CR.CASES if c[0] > 1], ids=CR.case_id)
def test_rows_are_independent(K, case):
    """A row's fwd and dgrad outputs computed alone (B = 1) have the bits they have inside the batch."""
    B, D, C, Tz, k = case
    z, w, bias, dout, dw0, db0 = CR.operands(case, 'random')
    zd, wd, bd, gd = (torch.from_numpy(a).cuda() for a in (z, w, bias, dout))
    out, dz = torch.full((B, C, Tz), float('nan'), device='cuda'), torch.full((B, D, Tz), float('nan'), device='cuda')
    K.cond_conv_fwd(zd, wd, bd, out)
    K.cond_conv_dgrad(wd, gd, dz)
    for b in range(B):
        o1, d1 = torch.full((1, C, Tz), float('nan'), device='cuda'), torch.full((1, D, Tz), float('nan'), device='cuda')
        K.cond_conv_fwd(zd[b:b + 1].contiguous(), wd, bd, o1)
        K.cond_conv_dgrad(wd, gd[b:b + 1].contiguous(), d1)
        assert torch.equal(o1[0], out[b]) and torch.equal(d1[0], dz[b]), 'row %d' % b


def test_argument_checks_return_errors(pkg, K):
    """Null pointers, bad sizes, strides below the row size, too little scratch and every aliasing come back through the error
    return, and nothing is launched: no buffer changes."""
    L = pkg._lib
    lib, ptr, st = L.lib(), L.ptr, L.stream()
    B, D, C, Tz, k = 2, 4, 16, 9, 3
    z, w, bias, dout, dw0, db0 = CR.operands((B, D, C, Tz, k), 'random')
    ns = K.cond_conv_wgrad_scratch(B, D, C, Tz, k)
    assert ns == min(B * 1, 16) * (k * D * C + C)
    g = {n_: Guarded(a) for n_, a in (('z', z), ('w', w), ('bias', bias), ('dout', dout), ('dw', dw0), ('db', db0),
                                      ('out', np.full((B, C, Tz), SENTINEL)), ('dz', np.full((B, D, Tz), SENTINEL)),
                                      ('scratch', np.full((ns,), SENTINEL)))}
    p = {n_: ptr(b.t) for n_, b in g.items()}
    zs, os_ = D * Tz, C * Tz
    fwd, dgr, wgr = lib.vqw_cond_conv_fwd, lib.vqw_cond_conv_dgrad, lib.vqw_cond_conv_wgrad

    def refused(rc, word):
        assert rc != 0 and word in lib.vqw_last_error(), lib.vqw_last_error()

    def f(z=p['z'], zb=zs, w=p['w'], b=p['bias'], o=p['out'], ob=os_, dims=(B, D, C, Tz, k)):
        return fwd(z, zb, w, b, o, ob, *dims, st)

    def d(w=p['w'], g_=p['dout'], gb=os_, dz=p['dz'], zb=zs, dims=(B, D, C, Tz, k)):
        return dgr(w, g_, gb, dz, zb, *dims, st)

    def wg(z=p['z'], zb=zs, g_=p['dout'], gb=os_, dw=p['dw'], db=p['db'], s=p['scratch'], n=ns, dims=(B, D, C, Tz, k)):
        return wgr(z, zb, g_, gb, dw, db, s, n, *dims, st)
    for kw in ({'z': None}, {'w': None}, {'b': None}, {'o': None}):
        refused(f(**kw), b'null pointer')
    for kw in ({'w': None}, {'g_': None}, {'dz': None}):
        refused(d(**kw), b'null pointer')
    for kw in ({'z': None}, {'g_': None}, {'dw': None}, {'db': None}, {'s': None}):
        refused(wg(**kw), b'null pointer')
    bad = [((0, D, C, Tz, k), b'positive'), ((B, 0, C, Tz, k), b'positive'), ((B, D, C, 0, k), b'positive'), ((B, D, C, -2, k), b'positive'),
           ((B, D, 0, Tz, k), b'multiple of 16'), ((B, D, 8, Tz, k), b'multiple of 16'), ((B, D, 24, Tz, k), b'multiple of 16'),
           ((B, D, C, Tz, 0), b'odd'), ((B, D, C, Tz, 2), b'odd'), ((B, D, C, Tz, 9), b'odd'), ((B, D, C, Tz, -1), b'odd')]
    for dims, word in bad:
        refused(f(dims=dims), word)
        refused(d(dims=dims), word)
        refused(wg(dims=dims), word)
        n = C_int64()
        assert lib.vqw_cond_conv_wgrad_scratch_floats(*dims, n) != 0
    assert lib.vqw_cond_conv_wgrad_scratch_floats(B, D, C, Tz, k, None) != 0
    for rc in (f(zb=zs - 1), f(ob=os_ - 1), d(gb=os_ - 1), d(zb=zs - 1), wg(zb=zs - 1), wg(gb=os_ - 1)):
        refused(rc, b'batch strides')
    refused(wg(n=ns - 1), b'scratch needs')
    # aliasing: the same buffer, and ranges that only overlap
    inside = lambda b, off: ptr(b.t.view(-1)[off:])  # noqa: E731
    big = Guarded(np.full((4 * B * C * Tz,), SENTINEL))
    refused(f(o=ptr(big.t), z=ptr(big.t)), b'overlap')          # out == z
    refused(f(o=ptr(big.t), z=inside(big, 8)), b'overlap')
    refused(f(o=ptr(big.t), w=inside(big, B * C * Tz - 1)), b'overlap')
    refused(f(o=ptr(big.t), b=inside(big, 3)), b'overlap')
    refused(d(dz=ptr(big.t), g_=inside(big, B * D * Tz - 1)), b'overlap')
    refused(d(dz=ptr(big.t), w=ptr(big.t)), b'overlap')
    refused(wg(dw=ptr(big.t), db=inside(big, k * D * C - 1)), b'overlap')
    refused(wg(dw=ptr(big.t), s=inside(big, 5)), b'overlap')
    refused(wg(db=ptr(big.t), s=inside(big, C - 1)), b'overlap')
    refused(wg(dw=p['z']), b'overlap')
    refused(wg(db=p['dout']), b'overlap')
    refused(wg(s=p['z']), b'overlap')
    refused(wg(s=p['dout'], dw=p['dw']), b'overlap')
    # the Python front end: operands too small for their shapes, the wrong device
    with pytest.raises(ValueError):
        K.cond_conv_fwd(g['z'].t, g['w'].t, g['bias'].t, g['out'].t[:, :C - 1].contiguous())
    with pytest.raises(ValueError):
        K.cond_conv_wgrad(g['z'].t, g['dout'].t, g['dw'].t, g['db'].t, g['scratch'].t[:ns - 1])
    with pytest.raises(RuntimeError, match='overlap'):
        K.cond_conv_dgrad(g['w'].t, g['dout'].t, g['dout'].t.view(-1)[:B * D * Tz].view(B, D, Tz))
    with pytest.raises(ValueError, match='GPU'):
        K.cond_conv_fwd(torch.zeros(B, D, Tz), g['w'].t, g['bias'].t, g['out'].t)
    torch.cuda.synchronize()
    for name, b in list(g.items()) + [('big', big)]:
        assert b.untouched(), '%s changed' % name


def C_int64():
    import ctypes
    return ctypes.byref(ctypes.c_int64(0))
