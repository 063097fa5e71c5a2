"""vqw_f16x3_gate_conv and the five forms of vqw_f16x3_out_conv against the plane-exact float64 reference of
tests/x3_conv_ref.py, through kernels.py (f16x3_split_activations, f16x3_pack_weights, f16x3_pack_gate_weights -- their byte images
are pinned by tests/test_x3_range_gpu.py --, f16x3_gate_conv, f16x3_out_conv), on both block heights and both operand families.

Every fp32 output is a view into a sentinel-filled buffer and every planes buffer holds a non-zero pattern before the launch:
whatever the header does not write -- guard bands, plane chunks outside [kc0, kc0 + R/8), outputs that were not asked for -- must
keep its bits.  Integer cases must equal the reference bit for bit wherever the output is linear; the gate conv's integer cases have
an exact pre-activation, so elements that share one (f, g) pair must agree bit for bit, and what they miss the float64 activations by
is the share of BAR_GATE the device functions use (record_property 'gate_activation_err').  Planes are compared with the exact split
of the launch's own fp32 output, the max-abs word with that output's largest magnitude; a launch without an fp32 output is run once
more with one.  A refusal must raise from the library, launch nothing and leave every output's bits alone.

Every test records `family` and `worst_fraction` (the worst err / bar of its case)."""
import functools
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import x3_conv_ref as Rf  # noqa: E402
import x3_ref as X  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F32 = np.float32
G = Rf.GUARD
SENT = float(Rf.SENTINEL)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Buf:
    """n floats between two guard bands of sentinels; `view` is what the kernel gets.  init: the view's contents (default sentinels)."""

    def __init__(self, n, init=None):
        self.n = n
        self.full = torch.full((G + n + G,), SENT, device=DEV)
        self.view = self.full[G:G + n]
        if init is not None:
            self.view.copy_(_dev(np.asarray(init, F32).reshape(-1)))
        self.before = self.full.clone()

    def host(self):
        return self.full.cpu().numpy()

    def values(self, shape):
        return self.view.cpu().numpy().reshape(shape)

    def untouched(self, what):
        assert torch.equal(self.full.view(torch.int32), self.before.view(torch.int32)), what + ': changed'


class Planes:
    """n halves of PLANE_FILL between two guard bands of 2 G halves; `view` (float16) is what the kernel gets."""

    def __init__(self, n):
        self.n = n
        self.full = torch.full((4 * G + n,), Rf.PLANE_FILL, dtype=torch.int16, device=DEV)
        self.view = self.full[2 * G:2 * G + n].view(torch.float16)

    def host(self):
        return self.full.cpu().numpy().view(np.uint16)

    def untouched(self, what):
        assert bool((self.full == Rf.PLANE_FILL).all()), what + ': changed'


def _slots():
    return torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)


@functools.lru_cache(maxsize=4)
def _reference(name, kind):
    c = next(c for c in Rf.all_cases() if c['name'] == name)
    return Rf.reference(c, Rf.inputs(c, kind))


def _params(cases):
    return [pytest.param(c, m, k, id='%s/%s/%s' % (c['name'], mn, k)) for c in cases for k in Rf.KINDS for mn, m in Rf.MODES]


def _record(record_property, kind, worst):
    record_property('family', kind)
    record_property('worst_fraction', worst)


def _range_words(amax, flag, values, what):
    assert int(amax.item()) == X.amax_bits(values), what + ': out_amax is not the bit pattern of max |net_out|'
    assert int(flag.item()) == 0, what + ': the range flag was raised'


def _same_bits(a, b, what):
    assert np.array_equal(np.asarray(a).view(np.uint32 if a.dtype == F32 else np.uint16), np.asarray(b).view(np.uint32 if b.dtype == F32 else np.uint16)), what


# ---------------------------------------------------------------------------------------------------- gate conv
def _gate_launch(K, c, ins, mode, subset):
    B, T, R, ks = c['B'], c['T'], c['R'], c['ks']
    xp = torch.empty(2 * B * R * T, dtype=torch.float16, device=DEV)
    wp = torch.empty(2 * ks * R * 2 * R, dtype=torch.float16, device=DEV)
    K.f16x3_split_activations(_dev(ins['x']), xp, B, R, T, scale=ins['sx'], mode=mode)
    K.f16x3_pack_gate_weights(_dev(ins['w']), wp, ks, R, 2 * R, ins['sw'], mode=mode)
    out = {n: Buf(B * R * T) for n in ('out0', 'save0', 'save1')}
    KC = c['out_planes_KC'] or R // 8
    pl = Planes(2 * KC * 8 * B * T)
    get = lambda n: out[n].view if n in subset else None  # noqa: E731
    K.f16x3_gate_conv(xp=xp, wp=wp, out0=get('out0'), B=B, T=T, R=R, ks=ks, dilation=c['dilation'], w_scale_inv=ins['winv'],
                      bias=_dev(ins['bias']) if c['bias'] else None, cond=_dev(ins['cond']) if c['cond_T'] else None, cond_T=c['cond_T'],
                      cond_bstride=c['cond_bstride'] if c['cond_T'] else 0, save0=get('save0'), save1=get('save1'),
                      out_planes=pl.view if 'out_planes' in subset else None, out_planes_kc0=c['out_planes_kc0'],
                      out_planes_KC=c['out_planes_KC'], mode=mode)
    torch.cuda.synchronize()
    return out, pl


def _agree_where_the_pre_activation_agrees(ref, got, what):
    """The device activations are pure functions of their fp32 inputs: save0 of f, save1 of g, out0 of the pair.  Elements whose
    exact inputs agree must agree bit for bit."""
    f, g = (ref[k].astype(F32).view(np.uint32).astype(np.uint64).reshape(-1) for k in ('f', 'g'))
    for n, key in (('save0', f), ('save1', g), ('out0', f << np.uint64(32) | g)):
        if n not in got:
            continue
        order = np.argsort(key, kind='stable')
        same = key[order][1:] == key[order][:-1]
        assert n == 'out0' or same.sum() > key.size // 2, what + ': the integer family must repeat its pre-activations'
        bits = got[n].reshape(-1).view(np.uint32)[order]
        bad = same & (bits[1:] != bits[:-1])
        assert not bad.any(), '%s: %d elements of %s differ from another element with the same pre-activation' % (what, int(bad.sum()), n)


@pytest.mark.parametrize('c,mode,kind', _params(Rf.gate_cases()))
def test_gate_conv(K, record_property, c, mode, kind):
    B, T, R = c['B'], c['T'], c['R']
    ins, ref = Rf.inputs(c, kind), _reference(c['name'], kind)
    out, pl = _gate_launch(K, c, ins, mode, c['subset'])
    worst, got = 0.0, {}
    for n in ('out0', 'save0', 'save1'):
        w = n in c['subset']
        worst = max(worst, Rf.check(out[n].host(), B * R * T, ref[n] if w else None, ref['bar_' + n], 'normal', c['name'] + ' ' + n))
        if w:
            got[n] = out[n].values((B, R, T))
    KC, kc0 = c['out_planes_KC'], c['out_planes_kc0']
    if 'out_planes' not in c['subset']:
        pl.untouched(c['name'] + ' out_planes')
    else:
        own = got.get('out0')
        if own is None:       # no fp32 out0: the planes of the same launch with one, and their decoded values within the bar
            out2, pl2 = _gate_launch(K, c, ins, mode, c['subset'] + ('out0',))
            own = out2['out0'].values((B, R, T))
            _same_bits(pl.host(), pl2.host(), c['name'] + ': planes differ from the launch that also stores out0')
            dec = Rf.decode_planes(pl.host()[2 * G:-2 * G].reshape(2, KC or R // 8, B * T, 8), kc0, R, B, T)
            worst = max(worst, Rf.compare(dec, ref['out0'], ref['bar_out0'] + Rf.SPLIT_REL * np.abs(ref['out0']) + Rf.F16_HALF_STEP, 'normal',
                                          c['name'] + ' decoded planes'))
        Rf.check_planes(pl.host(), Rf.plane_image(own, kc0=kc0, KC=KC), c['name'] + ' out_planes')
    if kind == 'ints':
        _agree_where_the_pre_activation_agrees(ref, got, c['name'])
        record_property('gate_activation_err', max(float(np.abs(got[n].astype(np.float64) - ref[n]).max()) for n in got))
    _record(record_property, kind, worst)


# ---------------------------------------------------------------------------------------------------- out conv, epi 0 and 2
def _out_operands(K, c, ins, mode, dev_scales=False):
    B, T, R, S, Cin = c['B'], c['T'], c['R'], c['S'], c['Cin']
    ks = c.get('ks', 1)
    C_all = ins['x'].shape[1]
    xp = torch.empty(2 * B * C_all * T, dtype=torch.float16, device=DEV)
    wp = torch.empty(2 * ks * Cin * (S + R), dtype=torch.float16, device=DEV)
    sc = torch.tensor([ins['sx'], ins['sw'], ins.get('out_scale', c.get('out_scale', 1.0))], device=DEV)
    if dev_scales:
        K.f16x3_split_activations(_dev(ins['x']), xp, B, C_all, T, scale_dev=sc[0:1], mode=mode)
        K.f16x3_pack_weights(_dev(ins['w']), wp, ks * Cin, S + R, S + R, 1.0, scale_dev=sc[1:2], mode=mode)
        kw = dict(w_scale_inv=1.0, x_scale=sc[0:1], w_scale=sc[1:2])
    else:
        K.f16x3_split_activations(_dev(ins['x']), xp, B, C_all, T, scale=ins['sx'], mode=mode)
        K.f16x3_pack_weights(_dev(ins['w']), wp, ks * Cin, S + R, S + R, ins['sw'], mode=mode)
        kw = dict(w_scale_inv=1.0 / (ins['sx'] * ins['sw']))
    return dict(xp=xp, wp=wp, B=B, T=T, R=R, S=S, Cin=Cin, mode=mode, **kw), sc


def _epi0_launch(K, c, ins, mode, alias):
    B, T, R, S = c['B'], c['T'], c['R'], c['S']
    kw, sc = _out_operands(K, c, ins, mode)
    skip = Buf(B * S * T, ins['skip']) if S else None
    net_in = Buf(B * R * T, ins['net_in']) if c['net_in'] != 'none' else None
    net_out = net_in if alias else Buf(B * R * T) if R else None
    amax, flag = _slots()
    pl = Planes(2 * (c['planes_KC'] * 8 or R) * B * T) if c['planes'] else None
    if pl is not None:
        kw.update(net_out_planes=pl.view, out_scale=sc[2:3], out_amax=amax, flag=flag, planes_kc0=c['planes_kc0'], planes_KC=c['planes_KC'],
                  plane_scale=c['plane_scale'])
    K.f16x3_out_conv(skip=None if skip is None else skip.view, net_in=None if net_in is None else net_in.view,
                     net_out=None if net_out is None else net_out.view, bias=_dev(ins['bias']) if c['bias'] else None, xp_kc0=c['xp_kc0'],
                     xp_KC=c['xp_KC'], ks=c['ks'], dilation=c['dilation'], direction=c['dir'], **kw)
    torch.cuda.synchronize()
    return dict(skip=skip, net_in=net_in, net_out=net_out, planes=pl, amax=amax, flag=flag)


@pytest.mark.parametrize('c,mode,kind', _params(Rf.out_cases()))
def test_out_conv_epi0(K, record_property, c, mode, kind):
    B, T, R, S = c['B'], c['T'], c['R'], c['S']
    ins, ref = Rf.inputs(c, kind), _reference(c['name'], kind)
    o = _epi0_launch(K, c, ins, mode, c['alias'])
    worst = 0.0
    if S:
        worst = max(worst, Rf.check(o['skip'].host(), B * S * T, ref['skip'], ref['bar_skip'], kind, c['name'] + ' skip'))
    if R:
        worst = max(worst, Rf.check(o['net_out'].host(), B * R * T, ref['net_out'], ref['bar_net'], kind, c['name'] + ' net_out'))
        if o['net_in'] is not None and not c['alias']:
            o['net_in'].untouched(c['name'] + ' net_in')
    if c['planes']:
        own = o['net_out'].values((B, R, T))
        ps, osc = Rf.plane_scales(c, ins)
        Rf.check_planes(o['planes'].host(), Rf.plane_image(own, ps, osc, c['planes_kc0'], c['planes_KC']), c['name'] + ' net_out_planes')
        _range_words(o['amax'], o['flag'], own, c['name'])
    if c['alias']:
        p = _epi0_launch(K, c, ins, mode, False)
        for n in ('skip', 'net_out', 'planes'):
            if o[n] is not None:
                _same_bits(o[n].host(), p[n].host(), '%s: %s of the in-place launch differs from the out-of-place launch' % (c['name'], n))
        assert int(o['amax'].item()) == int(p['amax'].item())
    _record(record_property, kind, worst)


def _head_launch(K, c, ins, mode, alias):
    B, T, R = c['B'], c['T'], c['R']
    kw, sc = _out_operands(K, c, ins, mode)
    net_in = Buf(B * R * T, ins['net_in']) if c['net_in'] else None
    mask = Buf(B * R * T, ins['mask']) if c['mask'] else None
    net_out = net_in if alias == 'net_in' else mask if alias == 'aux0' else Buf(B * R * T)
    amax, flag = _slots()
    pl = Planes(2 * R * B * T) if c['planes'] else None
    if pl is not None:
        kw.update(net_out_planes=pl.view, out_scale=sc[2:3], out_amax=amax, flag=flag)
    K.f16x3_out_conv(epi=2, net_in=None if net_in is None else net_in.view, net_out=net_out.view, aux0=None if mask is None else mask.view,
                     bias=_dev(ins['bias']) if c['bias'] else None, cond=_dev(ins['cond']) if c['cond_T'] else None, cond_T=c['cond_T'],
                     cond_bstride=c['cond_bstride'] if c['cond_T'] else 0, relu_planes=c['relu'], **kw)
    torch.cuda.synchronize()
    return dict(net_in=net_in, mask=mask, net_out=net_out, planes=pl, amax=amax, flag=flag)


@pytest.mark.parametrize('c,mode,kind', _params(Rf.head_cases()))
def test_out_conv_epi2(K, record_property, c, mode, kind):
    B, T, R = c['B'], c['T'], c['R']
    ins, ref = Rf.inputs(c, kind), _reference(c['name'], kind)
    o = _head_launch(K, c, ins, mode, c['alias'])
    worst = Rf.check(o['net_out'].host(), B * R * T, ref['net_out'], ref['bar_net'], kind, c['name'] + ' net_out')
    for n in ('net_in', 'mask'):
        if o[n] is not None and o[n] is not o['net_out']:
            o[n].untouched(c['name'] + ' ' + n)
    if c['planes']:
        own = o['net_out'].values((B, R, T))
        src = np.maximum(own, F32(0)) if c['relu'] else own
        ps, osc = Rf.plane_scales(c, ins)
        Rf.check_planes(o['planes'].host(), Rf.plane_image(src, ps, osc), c['name'] + ' net_out_planes')
        _range_words(o['amax'], o['flag'], src, c['name'])
        if kind == 'ints':
            Rf.check_planes(o['planes'].host(), Rf.plane_image(ref['plane_src'], ps, osc), c['name'] + ' net_out_planes against the reference')
    if c['alias'] != 'none':
        p = _head_launch(K, c, ins, mode, 'none')
        for n in ('net_out', 'planes'):
            _same_bits(o[n].host(), p[n].host(), '%s: %s of the in-place launch differs from the out-of-place launch' % (c['name'], n))
        assert int(o['amax'].item()) == int(p['amax'].item())
    _record(record_property, kind, worst)


# ---------------------------------------------------------------------------------------------------- out conv, epi 1
def _bwd_launch(K, c, ins, mode, fp32):
    B, T, R = c['B'], c['T'], c['R']
    kw, sc = _out_operands(K, c, ins, mode, dev_scales=True)
    th, sg, gated = (Buf(B * R * T, ins[k]) for k in ('th', 'sg', 'gated'))
    aux = dict(aux0=th.view)
    if c['aux'] == 'gated':
        aux = dict(aux0=gated.view, aux0_is_gated=True)
    elif c['aux'] == 'planes':        # the gated planes inside a wider planes tensor (three layers side by side)
        gpl = torch.zeros(2 * B * c['aux0_KC'] * 8 * T, dtype=torch.float16, device=DEV)
        wide = ins['gated_wide']                                    # the neighbouring layers' chunks hold their own gated outputs
        assert c['aux0_kc0'] == R // 8 and np.array_equal(wide[:, R:2 * R], ins['gated'])
        for layer in range(3):
            K.f16x3_split_activations(_dev(wide[:, layer * R:(layer + 1) * R]), gpl, B, R, T, kc0=layer * (R // 8), KC=c['aux0_KC'], mode=mode)
        aux = dict(aux0_is_gated=True, aux0_planes=gpl, aux0_KC=c['aux0_KC'], aux0_kc0=c['aux0_kc0'])
    dpre = Buf(B * 2 * R * T)
    amax, flag = _slots()
    pl = Planes(2 * 2 * R * B * T)
    K.f16x3_out_conv(epi=1, aux1=sg.view, net_out=dpre.view if fp32 else None, net_out_planes=pl.view, out_scale=sc[2:3], out_amax=amax, flag=flag,
                     **aux, **kw)
    torch.cuda.synchronize()
    for b, n in ((th, 'th'), (sg, 'sg'), (gated, 'gated')):
        b.untouched(c['name'] + ' ' + n)
    return dict(dpre=dpre, planes=pl, amax=amax, flag=flag)


@pytest.mark.parametrize('c,mode,kind', _params(Rf.bwd_cases()))
def test_out_conv_epi1(K, record_property, c, mode, kind):
    B, T, R = c['B'], c['T'], c['R']
    ins, ref = Rf.inputs(c, kind), _reference(c['name'], kind)
    o = _bwd_launch(K, c, ins, mode, c['fp32'])
    n = B * 2 * R * T
    worst = Rf.check(o['dpre'].host(), n, ref['dpre'] if c['fp32'] else None, ref['bar'], kind, c['name'] + ' dpre')
    ps, osc = Rf.plane_scales(c, ins)
    src = o
    if not c['fp32']:         # planes only: the planes and the max-abs word of the same launch with an fp32 dpre
        src = _bwd_launch(K, c, ins, mode, True)
        worst = max(worst, Rf.check(src['dpre'].host(), n, ref['dpre'], ref['bar'], kind, c['name'] + ' dpre of the fp32 launch'))
        _same_bits(o['planes'].host(), src['planes'].host(), c['name'] + ': planes differ from the launch that also stores dpre')
        assert int(o['amax'].item()) == int(src['amax'].item())
        dec = Rf.decode_planes(o['planes'].host()[2 * G:-2 * G].reshape(2, 2 * R // 8, B * T, 8), 0, 2 * R, B, T, ps * osc)
        worst = max(worst, Rf.compare(dec, ref['dpre'], ref['bar'] + Rf.SPLIT_REL * np.abs(ref['dpre']) + Rf.F16_HALF_STEP / (ps * osc), 'normal',
                                      c['name'] + ' decoded planes'))
    own = src['dpre'].values((B, 2 * R, T))
    Rf.check_planes(o['planes'].host(), Rf.plane_image(own, ps, osc), c['name'] + ' net_out_planes')
    _range_words(o['amax'], o['flag'], own, c['name'])
    _record(record_property, kind, worst)


# ---------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize('name,kernel,kw', Rf.refusal_cases(), ids=[r[0] for r in Rf.refusal_cases()])
def test_illegal_descriptors_are_refused_without_a_launch(K, name, kernel, kw):
    assert Rf.legality(kernel, kw) is not None
    n = 2 * 256 * 1024                      # floats: more than any descriptor of the table asks for
    xp = torch.zeros(8 * n, dtype=torch.float16, device=DEV)
    wp = torch.zeros(8 * n, dtype=torch.float16, device=DEV)
    outs = {k: Buf(n) for k in ('a', 'b', 'c')}
    pl = Planes(8 * n)
    amax, flag = _slots()
    B, T, R = kw['B'], kw['T'], kw['R']
    with pytest.raises(RuntimeError, match=re.escape('libvqwave: vqw_f16x3_%s_conv: ' % kernel) + '.*' + re.escape(Rf.REFUSED_WITH[name])):
        if kernel == 'gate':
            K.f16x3_gate_conv(xp=xp, wp=wp, out0=outs['a'].view, B=B, T=T, R=R, ks=kw['ks'], dilation=kw['dilation'], w_scale_inv=kw['w_scale_inv'],
                              cond=torch.zeros(n, device=DEV), cond_T=kw['cond_T'], save0=outs['b'].view, save1=outs['c'].view, out_planes=pl.view,
                              out_planes_kc0=kw.get('out_planes_kc0', 0), out_planes_KC=kw.get('out_planes_KC', 0), mode=kw['mode'])
        else:
            ct = kw.get('cond_T', 0)
            aux = dict(aux0=torch.ones(n, device=DEV), aux1=torch.ones(n, device=DEV)) if kw['epi'] else {}
            K.f16x3_out_conv(xp=xp, wp=wp, B=B, T=T, R=R, S=kw['S'], Cin=kw['Cin'], ks=kw['ks'], dilation=kw['dilation'], epi=kw['epi'],
                             w_scale_inv=kw['w_scale_inv'], skip=outs['a'].view, net_in=outs['b'].view, net_out=outs['c'].view,
                             net_out_planes=pl.view, xp_kc0=kw['xp_kc0'], xp_KC=kw['xp_KC'], out_amax=amax, flag=flag, mode=kw['mode'],
                             cond=torch.zeros(n, device=DEV) if ct else None, cond_T=ct, cond_bstride=R * ct, **aux)
    torch.cuda.synchronize()
    for k, b in outs.items():
        b.untouched(name + ' output ' + k)
    pl.untouched(name + ' planes')
    assert int(amax.item()) == 0 and int(flag.item()) == 0


# ---------------------------------------------------------------------------------------------------- the reference itself
def test_numpy_reference_matches_torch_float64_on_the_device():
    """Two mid-sized contractions of the tables (a dilated gate conv, an input gradient that reads ahead) once more in torch float64
    on the device, from the same planes: the numpy evaluation is what it says."""
    for c in (Rf.gate_cases()[8], Rf.out_cases()[9]):
        ins = Rf.inputs(c, 'normal')
        ks, dil = c['ks'], c['dilation']
        sh = Rf.shifts(ks, dil, c.get('dir', 1))
        x1, x2 = (_dev(h.astype(np.float64)) for h in X.split(X.scaled(ins['x'], ins['sx'])))
        w1, w2 = (_dev(h.astype(np.float64)) for h in X.split(X.scaled(ins['w'], ins['sw'])))
        T = c['T']

        def read(h, s):
            o = torch.zeros_like(h)
            if s >= 0 and s < T:
                o[:, :, s:] = h[:, :, :T - s]
            elif -T < s < 0:
                o[:, :, :T + s] = h[:, :, -s:]
            return o
        pre = 0.0
        for j in range(ks):
            a1, a2 = read(x1, sh[j]), read(x2, sh[j])
            pre = pre + torch.einsum('bct,cm->bmt', a1, w1[j] + w2[j]) + torch.einsum('bct,cm->bmt', a2, w1[j])
        winv = ins['winv'] if 'winv' in ins else 1.0 / (ins['sx'] * ins['sw'])
        want, ab, n = Rf.conv_pre(ins['x'], ins['w'], sh, ins['sx'], ins['sw'], winv)
        err = np.abs((pre * winv).cpu().numpy() - want)
        assert (err <= 1e-13 * ab + 1e-300).all(), (c['name'], float((err / np.maximum(ab, 1e-300)).max()))
