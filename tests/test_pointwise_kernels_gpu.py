"""The HBM-bound kernels of csrc/pointwise.hip against the float64 and exact-integer references of tests/pointwise_ref.py: the
loss and its gradient seed, row sums, transposes, the relu / BatchNorm passes, the two Cin == 1 convolutions, the optimiser
step and the decoder's input stage, at the smallest shapes that reach each loop, tail, template instance and alignment path.

Outputs and in-place operands are views into sentinel-filled buffers; pointwise_ref.compare holds the written region to the
case's expectation -- bit-equality for what is exact by construction and for the exact-integer inputs of every kernel that sums,
an elementwise bar in units of 2^-24 for standard-normal inputs -- and everything else to bit-equality.

Every test records err / bar of its case (record_property 'err_over_bar', with 'family'); DESIGN 6 lists the maxima."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pointwise_ref as PR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
KINDS = ('ints', 'normal')


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _dev_off(a, off):
    """A device copy of `a` whose first element lies `off` floats past a 16-byte boundary."""
    a = np.ascontiguousarray(a)
    full = torch.empty(a.size + 4, dtype=torch.from_numpy(a).dtype, device=DEV)
    v = full[off:off + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    return v


class DBuf:
    """The device twin of a pointwise_ref.Buf: `view` is what the kernel gets, host() the whole buffer read back."""

    def __init__(self, n, off=0, init=None):
        self.buf = PR.Buf(n, off, init)
        self.full = _dev(self.buf.full)
        self.view = self.full[self.buf.lo:self.buf.lo + n]

    def host(self):
        return self.full.cpu().numpy()

    def check(self, vals, bar, what, mask=None):
        return PR.compare(self.host(), self.buf, vals, bar, mask, what)

    def untouched(self, what):
        return PR.compare(self.host(), self.buf, self.buf.view, None, np.zeros(self.buf.n, dtype=bool), what)


def _ids(cases):
    return [c['name'] for c in cases]


# ---------------------------------------------------------------------------------------------------- softmax cross-entropy
@pytest.mark.parametrize('c', PR.softmax_cases(), ids=_ids(PR.softmax_cases()))
def test_softmax_xent_matches_float64_reference(K, record_property, c):
    x, lab = PR.softmax_inputs(c)
    B, Q, T = x.shape
    gs = c['grad_scale']
    ref = PR.softmax_ref(x, lab)
    bars = PR.softmax_bars(x, lab, ref, gs)
    want = dict(p=ref['p'], d=(ref['p'] - PR.onehot(lab, Q)) * gs, ls=PR.SOFTMAX_LOSS0 + ref['loss'].sum())
    dx, dlab = _dev(x), _dev(lab)
    first, worst = {}, {'loss_sum': 0.0, 'p': 0.0, 'd': 0.0}
    runs = [('fused', d, p) for d in (False, True) for p in (False, True)] + [('fwd', False, False), ('fwd', False, True),
                                                                             ('bwd', True, False), ('bwd_in_place', True, False)]
    for entry, with_d, with_p in runs:
        what = '%s %s dlogits=%d probs=%d' % (c['name'], entry, with_d, with_p)
        ls = DBuf(1, init=[PR.SOFTMAX_LOSS0])
        pb = DBuf(x.size) if with_p else None
        db = (DBuf(x.size, init=x) if entry == 'bwd_in_place' else DBuf(x.size)) if with_d else None
        pv = pb.view.view(B, Q, T) if with_p else None
        dv = db.view.view(B, Q, T) if with_d else None
        if entry == 'fused':
            K.softmax_xent(dx, dlab, loss_sum=ls.view, dlogits=dv, probs=pv, grad_scale=gs)
        elif entry == 'fwd':
            K.softmax_xent_fwd(dx, dlab, loss_sum=ls.view, probs=pv)
        else:
            K.softmax_xent_bwd(dv if entry == 'bwd_in_place' else dx, dlab, dlogits=dv, grad_scale=gs)
        if entry.startswith('bwd'):
            ls.untouched(what + ' loss_sum')
        else:
            worst['loss_sum'] = max(worst['loss_sum'], ls.check([want['ls']], bars['loss_sum'], what + ' loss_sum'))
        for name, buf, bar in (('p', pb, bars['p']), ('d', db, bars['dlogits'])):
            if buf is None:
                continue
            worst[name] = max(worst[name], buf.check(want[name], bar, what + ' ' + name))
            got = buf.view.clone()
            assert torch.equal(first.setdefault(name, got).view(torch.int32), got.view(torch.int32)), what + ': the entries differ in ' + name
    record_property('family', 'softmax_xent')
    record_property('err_over_bar', max(worst.values()))
    for name, r in worst.items():
        record_property('err_over_bar_' + name, r)


# ---------------------------------------------------------------------------------------------------- row sums
@pytest.mark.parametrize('c', PR.rowsum_cases(), ids=_ids(PR.rowsum_cases()))
def test_rowsum_matches_exact_integer_and_float64_references(K, record_property, c):
    B, C, T, seg = c['B'], c['C'], c['T'], c['seg']
    worst = 0.0
    for kind in KINDS:
        ins = PR.rowsum_inputs(c, kind)
        dx, dy = _dev_off(ins['x'], c['xoff']), _dev_off(ins['y'], c['yoff'])
        for with_y, with_seg, with_total, alpha in PR.rowsum_variants(c):
            what = '%s %s y=%d seg_out=%d total=%d alpha=%g (%s kernel)' % (c['name'], kind, with_y, with_seg, with_total, alpha,
                                                                           PR.rowsum_kernel(c, with_y, with_seg))
            ref = PR.rowsum_ref(c, ins, with_y, alpha)
            sb = DBuf(B * C * (T // seg)) if with_seg else None
            tb = DBuf(C, init=ins['total0']) if with_total else None
            K.rowsum(dx, y=dy if with_y else None, seg_out=sb.view if with_seg else None, total=tb.view if with_total else None,
                     alpha=alpha, seg=seg)
            if with_seg:
                worst = max(worst, sb.check(ref['seg'], None if kind == 'ints' else ref['seg_bar'], what + ' seg_out'))
            if with_total:
                worst = max(worst, tb.check(ref['total'], None if kind == 'ints' else ref['total_bar'], what + ' total'))
    record_property('family', 'rowsum')
    record_property('err_over_bar', worst)


# ---------------------------------------------------------------------------------------------------- transpose
@pytest.mark.parametrize('batch,rows,cols', PR.TRANSPOSE_CASES)
def test_transpose_is_bit_exact(K, record_property, batch, rows, cols):
    src = PR.with_zeros(PR.randn(PR.seed_of('transpose', batch, rows, cols), batch, rows, cols), 1)
    dst = DBuf(src.size)
    K.transpose(_dev(src), dst.view, batch, rows, cols)
    dst.check(PR.transpose_ref(src, batch, rows, cols), None, 'transpose %dx%dx%d' % (batch, rows, cols))
    record_property('family', 'transpose')
    record_property('err_over_bar', 0.0)


# ---------------------------------------------------------------------------------------------------- relu / BatchNorm passes
@pytest.mark.parametrize('shape', PR.BN_SHAPES, ids=['x'.join(map(str, s)) for s in PR.BN_SHAPES])
def test_bn_relu_bwd_is_bit_exact(K, record_property, shape):
    sd = PR.seed_of('bn_relu_bwd', shape)
    dx, r, scale = PR.randn(sd, *shape), PR.with_zeros(PR.randn(sd + 1, *shape), sd + 2), PR.randn(sd + 3, shape[1])
    n = dx.size
    for with_r in (True, False):
        want = PR.bn_relu_bwd_ref(dx, r if with_r else None, scale)
        for in_place in (False, True):
            dz = DBuf(n, init=dx if in_place else None)
            K.bn_relu_bwd(dz.view.view(shape) if in_place else _dev(dx), _dev(r) if with_r else None, _dev(scale), dz.view.view(shape))
            dz.check(want, None, 'bn_relu_bwd %s r=%d in_place=%d' % (shape, with_r, in_place))
    record_property('family', 'bn_relu_bwd')
    record_property('err_over_bar', 0.0)


@pytest.mark.parametrize('shape', PR.BN_SHAPES, ids=['x'.join(map(str, s)) for s in PR.BN_SHAPES])
def test_relu_bn_fwd_matches_references(K, record_property, shape):
    worst = 0.0
    for kind in KINDS:
        sd = PR.seed_of('relu_bn_fwd', shape, kind)
        x = PR.with_zeros(PR.operand(kind, sd, *shape), sd + 1)
        scale, shift = PR.coeff(kind, sd + 2, shape[1]), PR.coeff(kind, sd + 3, shape[1])
        for with_r in (True, False):
            for with_scale in (True, False):
                what = 'relu_bn_fwd %s %s r=%d scale=%d' % (shape, kind, with_r, with_scale)
                r, xn, bar = PR.relu_bn_fwd_ref(x, scale if with_scale else None, shift if with_scale else None)
                xb, rb = DBuf(x.size, init=x), (DBuf(x.size) if with_r else None)
                K.relu_bn_fwd(xb.view.view(shape), rb.view.view(shape) if with_r else None, _dev(scale) if with_scale else None,
                              _dev(shift) if with_scale else None)
                worst = max(worst, xb.check(xn, None if (kind == 'ints' or bar is None) else bar, what + ' x'))
                if with_r:
                    rb.check(r, None, what + ' r')
    record_property('family', 'relu_bn_fwd')
    record_property('err_over_bar', worst)


@pytest.mark.parametrize('T', PR.BN_SUMS_T)
def test_bn_relu_bwd_sums_matches_references(K, record_property, T):
    B, C = PR.BN_SUMS_BC
    shape, worst = (B, C, T), 0.0
    for kind in KINDS:
        ins = PR.bn_sums_inputs(T, kind)
        dy, dr, dscale_in = _dev(ins['y']), _dev(ins['r']), _dev(ins['scale'])
        for form in PR.BN_SUMS_FORMS:
            ref = PR.bn_sums_ref(ins, form)
            y, r = dy, dict(r_is_y=dy, distinct=dr, r_null=None)[form]
            for drop in PR.BN_SUMS_DROP:
                for in_place in (False, True):
                    what = 'bn_relu_bwd_sums T=%d %s %s without=%s in_place=%d' % (T, kind, form, drop, in_place)
                    dz = DBuf(B * C * T, init=ins['dx'] if in_place else None)
                    sums = {n: DBuf(C, init=ins[n + '0']) for n in ('dscale', 'dbeta', 'dbias') if n != drop}
                    K.bn_relu_bwd_sums(dz.view.view(shape) if in_place else _dev(ins['dx']), y, r, dscale_in, dz.view.view(shape),
                                       **{n: b.view for n, b in sums.items()})
                    dz.check(ref['dz'], None, what + ' dz')
                    for n, b in sums.items():
                        worst = max(worst, b.check(ref[n], None if kind == 'ints' else ref[n + '_bar'], what + ' ' + n))
    record_property('family', 'bn_relu_bwd_sums')
    record_property('err_over_bar', worst)


# ---------------------------------------------------------------------------------------------------- Cin == 1 convolutions
@pytest.mark.parametrize('c', PR.conv_cin1_cases(), ids=_ids(PR.conv_cin1_cases()))
def test_conv_cin1_matches_exact_integer_and_float64_references(K, record_property, c):
    B, F, k, To = c['B'], c['F'], c['k'], c['T_out']
    _, offset = PR.conv_cin1_geometry(c)
    off, n, worst = PR.conv_cin1_out_off(c), B * F * To, {'fwd': 0.0, 'wgrad': 0.0}
    for kind in KINDS:
        ins = PR.conv_cin1_inputs(c, kind)
        d = {name: (None if a is None else _dev(a)) for name, a in ins.items() if name not in ('dout', 'dw0')}
        for relu, scale, save in PR.CONV_CIN1_OPTIONS:
            what = '%s %s relu=%d scale=%d save_r=%d' % (c['name'], kind, relu, scale, save)
            ref = PR.conv_cin1_fwd_ref(c, ins, relu, scale)
            ob, rb = DBuf(n, off), (DBuf(n, off) if save else None)
            K.conv_cin1_fwd(d['x'], d['w'], d['bias'], ob.view.view(B, F, To), k=k, stride=c['stride'], offset=offset, relu=relu,
                            scale=d['scale'] if scale else None, shift=d['shift'] if scale else None,
                            save_r=rb.view.view(B, F, To) if save else None)
            worst['fwd'] = max(worst['fwd'], ob.check(ref['out'], None if kind == 'ints' else ref['out_bar'], what + ' out'))
            if save:
                worst['fwd'] = max(worst['fwd'], rb.check(ref['r'], None if kind == 'ints' else ref['r_bar'], what + ' save_r'))
        ref = PR.conv_cin1_wgrad_ref(c, ins)
        dw = DBuf(k * F, init=ins['dw0'])
        K.conv_cin1_wgrad(d['x'], _dev_off(ins['dout'], off), dw.view, k=k, stride=c['stride'], offset=offset)
        worst['wgrad'] = max(worst['wgrad'], dw.check(ref['dw'], None if kind == 'ints' else ref['dw_bar'], '%s %s dw' % (c['name'], kind)))
    record_property('family', 'conv_cin1')
    record_property('err_over_bar', max(worst.values()))
    record_property('err_over_bar_fwd', worst['fwd'])
    record_property('err_over_bar_wgrad', worst['wgrad'])


# ---------------------------------------------------------------------------------------------------- Adam + EMA
@pytest.mark.parametrize('n', PR.ADAM_N)
def test_adam_ema_step_matches_float64_reference(K, record_property, n):
    ins = PR.adam_inputs(n)
    refs = {form: PR.adam_ref(ins, 'plain' if form == 'skip0' else form) for form in PR.ADAM_FORMS}
    zero, one = torch.zeros(1, dtype=torch.int32, device=DEV), torch.ones(1, dtype=torch.int32, device=DEV)
    quarter = torch.full((1,), PR.ADAM_SCALE, device=DEV)
    worst = 0.0
    for align, offs in PR.ADAM_ALIGN.items():
        grads = [_dev_off(g, offs[1]) for g in ins['grads']]
        for form in PR.ADAM_FORMS:
            what = 'adam n=%d %s %s' % (n, align, form)
            p, m, v, ema = (DBuf(n, o, init=ins[name]) for name, o in zip(('p', 'm', 'v', 'ema'), (offs[0],) + offs[2:]))
            kw = dict(plain={}, skip0=dict(skip=zero), skip1=dict(skip=one, scale=quarter), scaled=dict(scale=quarter))[form]
            for g, lr_t in zip(grads, PR.ADAM_LR_T):
                K.adam_ema_step(p.view, g, m.view, v.view, ema.view, lr_t=lr_t, grad_scale=PR.ADAM_GRAD_SCALE, **kw)
            for name, b, want in zip(('p', 'm', 'v', 'ema'), (p, m, v, ema), refs[form]):
                bar = None if form == 'skip1' else PR.ADAM_TOL + PR.ADAM_TOL * np.abs(want)
                worst = max(worst, b.check(want, bar, what + ' ' + name))
    record_property('family', 'adam_ema_step')
    record_property('err_over_bar', worst)


# ---------------------------------------------------------------------------------------------------- wavenet_inputs
@pytest.mark.parametrize('B,T', PR.WAVENET_INPUTS_BT)
def test_wavenet_inputs_labels_are_bit_exact(K, record_property, B, T):
    x = np.random.RandomState(PR.seed_of('wavenet_inputs', B, T)).uniform(-1.1, 1.1, (B, T)).astype(np.float32)
    want_l, want_i = PR.wavenet_inputs_ref(x)
    dx, worst = _dev(x), 0.0
    for with_i, with_l in ((True, True), (True, False), (False, True)):
        what = 'wavenet_inputs %dx%d inputs=%d labels=%d' % (B, T, with_i, with_l)
        ib = DBuf(B * T) if with_i else None
        lfull = torch.full((PR.GUARD + B * T + PR.GUARD,), -77, dtype=torch.int32, device=DEV)
        K.wavenet_inputs(dx, ib.view.view(B, T) if with_i else None, lfull[PR.GUARD:PR.GUARD + B * T].view(B, T) if with_l else None)
        if with_i:
            worst = max(worst, ib.check(want_i, PR.WAVENET_INPUTS_ATOL, what + ' inputs'))
        got = lfull.cpu().numpy()
        assert (got[:PR.GUARD] == -77).all() and (got[PR.GUARD + B * T:] == -77).all(), what + ': a label guard band changed'
        inner = got[PR.GUARD:PR.GUARD + B * T]
        assert np.array_equal(inner, want_l.reshape(-1)) if with_l else (inner == -77).all(), what + ' labels'
    record_property('family', 'wavenet_inputs')
    record_property('err_over_bar', worst)


# ---------------------------------------------------------------------------------------------------- the error contract
def _refused(bufs, what):
    torch.cuda.synchronize()
    for b in bufs:
        b.untouched(what)


def test_softmax_q_not_a_multiple_of_four_is_an_error_and_does_not_launch(K):
    B, Q, T = 2, 6, 10
    x, lab = _dev(PR.randn(1, B, Q, T)), _dev(np.zeros((B, T), np.int32))
    ls, d, p = DBuf(1), DBuf(B * Q * T), DBuf(B * Q * T)
    dv, pv = d.view.view(B, Q, T), p.view.view(B, Q, T)
    for call in (lambda: K.softmax_xent(x, lab, loss_sum=ls.view, dlogits=dv, probs=pv),
                 lambda: K.softmax_xent_fwd(x, lab, loss_sum=ls.view, probs=pv),
                 lambda: K.softmax_xent_bwd(x, lab, dlogits=dv)):
        with pytest.raises(RuntimeError, match='must be a multiple of 4'):
            call()
    _refused((ls, d, p), 'softmax_xent with Q = 6')


def test_rowsum_segment_that_does_not_divide_t_is_an_error_and_does_not_launch(K):
    B, C, T, seg = 3, 7, 104, 7
    sb, tb = DBuf(B * C * (T // seg + 1)), DBuf(C)
    with pytest.raises(RuntimeError, match='must divide'):
        K.rowsum(_dev(PR.randn(1, B, C, T)), seg_out=sb.view, total=tb.view, seg=seg)
    _refused((sb, tb), 'rowsum with seg = 7, T = 104')


@pytest.mark.parametrize('bad,match', [(dict(k=33), 'k<=32'), (dict(stride=5), 'stride must be <= 4'), (dict(shift=None), 'scale needs shift'),
                                       (dict(out_off=1), 'out and save_r must be 16-byte aligned'),
                                       (dict(save_off=1), 'out and save_r must be 16-byte aligned')],
                         ids=['k_33', 'stride_5', 'scale_without_shift', 'misaligned_out', 'misaligned_save_r'])
def test_conv_cin1_fwd_refusals_do_not_launch(K, bad, match):
    B, F, To = 2, 17, 8
    k, stride = bad.get('k', 5), bad.get('stride', 2)
    ob, rb = DBuf(B * F * To, bad.get('out_off', 0)), DBuf(B * F * To, bad.get('save_off', 0))
    scale = _dev(PR.randn(3, F))
    with pytest.raises(RuntimeError, match=match):
        K.conv_cin1_fwd(_dev(PR.randn(1, B, stride * To)), _dev(PR.randn(2, k, F)), None, ob.view.view(B, F, To), k=k, stride=stride,
                        offset=-1, relu=True, scale=scale, shift=bad.get('shift', scale), save_r=rb.view.view(B, F, To))
    _refused((ob, rb), 'conv_cin1_fwd with %r' % (bad,))


@pytest.mark.parametrize('bad,match', [(dict(k=33), 'k<=32'), (dict(stride=5), 'stride must be <= 4'),
                                       (dict(dout_off=1), 'dout must be 16-byte aligned')], ids=['k_33', 'stride_5', 'misaligned_dout'])
def test_conv_cin1_wgrad_refusals_do_not_launch(K, bad, match):
    B, F, To = 2, 17, 8
    k, stride = bad.get('k', 5), bad.get('stride', 2)
    dw = DBuf(k * F, init=PR.randn(4, k, F))
    with pytest.raises(RuntimeError, match=match):
        K.conv_cin1_wgrad(_dev(PR.randn(1, B, stride * To)), _dev_off(PR.randn(2, B, F, To), bad.get('dout_off', 0)), dw.view, k=k,
                          stride=stride, offset=-1)
    _refused((dw,), 'conv_cin1_wgrad with %r' % (bad,))


@pytest.mark.parametrize('which', ['dx', 'dz', 'y', 'r'])
def test_bn_relu_bwd_sums_misaligned_vector_rows_are_an_error_and_do_not_launch(K, which):
    B, C, T = 3, 7, 8
    shape = (B, C, T)
    dz, sums = DBuf(B * C * T, int(which == 'dz')), [DBuf(C, init=PR.randn(i, C)) for i in range(3)]
    t = {n: _dev_off(PR.randn(10 + i, *shape), int(which == n)) for i, n in enumerate(('dx', 'y', 'r'))}
    with pytest.raises(RuntimeError, match='must be 16-byte aligned'):
        K.bn_relu_bwd_sums(t['dx'], t['y'], t['r'], _dev(PR.randn(5, C)), dz.view.view(shape), dscale=sums[0].view, dbeta=sums[1].view,
                           dbias=sums[2].view)
    _refused([dz] + sums, 'bn_relu_bwd_sums with a misaligned ' + which)
