"""tests/x3_conv_ref.py -- the float64 reference tests/test_x3_conv_kernels_gpu.py holds the fp16x3 stride-1 convs to -- pinned
without a GPU: against torch float64 and autograd where the split is taken away, against its own plane images, against each of
its deliberately wrong evaluations, against sequential fp32 emulations in three orders, and its case tables against the caps the
bars and the bit-equality demands rest on."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import x3_conv_ref as Rf  # noqa: E402
import x3_ref as X  # noqa: E402

F32 = np.float32
CASES = Rf.all_cases()
BY_NAME = {c['name']: c for c in CASES}


def _t(a):
    return torch.from_numpy(np.asarray(a, np.float64))


def _causal(x, wf, d):
    """y[b][m][t] = sum_j sum_c wf[j][c][m] x[b][c][t - (ks-1-j) d] with torch: a dilated conv1d over the left-padded input."""
    ks = wf.shape[0]
    return F.conv1d(F.pad(x, ((ks - 1) * d, 0)), wf.permute(2, 1, 0).contiguous(), dilation=d)


# ---------------------------------------------------------------------------------------------------- independent evaluations
@pytest.mark.parametrize('i', (0, 1, 3, 5, 7, 8))
def test_gate_reference_without_the_split_is_torch_float64(i):
    c = Rf.gate_cases()[i]
    ins = dict(Rf.inputs(c, 'normal'), sx=1.0, sw=1.0, winv=1.0)
    ref = Rf.gate_ref(c, ins, split=Rf.unsplit)
    B, T, R = c['B'], c['T'], c['R']
    pre = _causal(_t(ins['x']), _t(ins['w']), c['dilation']) + _t(ins['bias'])[None, :, None]
    ct = c['cond_T']
    cond = torch.as_strided(_t(ins['cond']), (B, 2 * R, ct), (c['cond_bstride'], ct, 1))
    pre = pre + cond.repeat_interleave(T // ct, dim=2)
    want = torch.tanh(pre[:, :R]) * torch.sigmoid(pre[:, R:])
    np.testing.assert_allclose(ref['out0'], want.numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(ref['save0'], torch.tanh(pre[:, :R]).numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(ref['save1'], torch.sigmoid(pre[:, R:]).numpy(), rtol=0, atol=1e-12)


@pytest.mark.parametrize('i', (0, 2, 4, 5, 6))
def test_epi0_reference_without_the_split_is_torch_float64(i):
    c = Rf.out_cases()[i]
    ins = dict(Rf.inputs(c, 'normal'), sx=1.0, sw=1.0)
    ref = Rf.out_ref(c, ins, split=Rf.unsplit)
    S, Cin, ch0 = c['S'], c['Cin'], 8 * c['xp_kc0']
    y = torch.einsum('bct,cm->bmt', _t(ins['x'])[:, ch0:ch0 + Cin], _t(ins['w'])[0])
    if c['bias']:
        y = y + _t(ins['bias'])[None, :, None]
    if S:
        np.testing.assert_allclose(ref['skip'], (_t(ins['skip']) + y[:, :S]).numpy(), rtol=0, atol=1e-11)
    if c['R']:
        old = _t(ins['net_in']) if c['net_in'] != 'none' else 0.0
        np.testing.assert_allclose(ref['net_out'], (old + y[:, S:]).numpy(), rtol=0, atol=1e-11)


@pytest.mark.parametrize('i', (8, 9, 10, 11, 12, 13))
def test_input_gradient_is_autograd_of_the_causal_conv(i):
    """The out conv with dir < 0 and kernels w[j][o][c] = wf[j][c][o] is the gradient of y = causal conv(x; wf) towards x."""
    c = Rf.out_cases()[i]
    assert c['dir'] < 0
    ins = dict(Rf.inputs(c, 'normal'), sx=1.0, sw=1.0)
    ref = Rf.out_ref(dict(c, bias=False, net_in='none'), ins, split=Rf.unsplit)
    dy = _t(ins['x'])                                               # [B][O][T]
    wf = _t(ins['w']).permute(0, 2, 1).contiguous()                 # [ks][c][o]
    x = torch.zeros(c['B'], c['R'], c['T'], dtype=torch.float64, requires_grad=True)
    (dx,) = torch.autograd.grad(_causal(x, wf, c['dilation']), x, dy)
    scale = float(dx.abs().max())
    np.testing.assert_allclose(ref['net_out'], dx.numpy(), rtol=0, atol=1e-12 * scale)
    # ... and the causal taps of the same entry point are the forward conv
    fwd = Rf.out_ref(dict(c, bias=False, net_in='none', dir=1), ins, split=Rf.unsplit)
    np.testing.assert_allclose(fwd['net_out'], _causal(dy, _t(ins['w']), c['dilation']).numpy(), rtol=0, atol=1e-12 * scale)


@pytest.mark.parametrize('aux', ('tanh', 'gated', 'planes'))
def test_gate_backward_is_autograd_of_tanh_times_sigmoid(aux):
    c = next(c for c in Rf.bwd_cases() if c['aux'] == aux and not c['underflow']) if aux != 'gated' else Rf.bwd_cases()[3]
    B, T, R, Cin = c['B'], c['T'], c['R'], c['Cin']
    rng = np.random.default_rng(5)
    f = torch.tensor(rng.standard_normal((B, R, T)), requires_grad=True)
    g = torch.tensor(rng.standard_normal((B, R, T)) * 2, requires_grad=True)
    dz, wo = rng.standard_normal((B, Cin, T)).astype(F32), (rng.standard_normal((R, Cin)) * 0.05).astype(F32)
    gated = torch.tanh(f) * torch.sigmoid(g)
    z = torch.einsum('brt,rk->bkt', gated, _t(wo))
    df, dg = torch.autograd.grad(z, (f, g), _t(dz))
    th, sg = torch.tanh(f).detach().numpy().astype(F32), torch.sigmoid(g).detach().numpy().astype(F32)
    ins = dict(x=dz, w=np.ascontiguousarray(wo.T)[None], th=th, sg=sg, gated=(th * sg).astype(F32), sx=1.0, sw=1.0)
    ref = Rf.bwd_ref(dict(c, underflow=False), ins, split=Rf.unsplit)
    want = torch.cat([df, dg], dim=1).numpy()
    np.testing.assert_allclose(ref['dpre'], want, rtol=0, atol=4e-7 * np.abs(want).max())      # th, sg, g enter as fp32


@pytest.mark.parametrize('i', (0, 5, 12, 14))
def test_head_reference_without_the_split_is_torch_float64(i):
    c = Rf.head_cases()[i]
    ins = dict(Rf.inputs(c, 'normal'), sx=1.0, sw=1.0)
    ref = Rf.head_ref(c, ins, split=Rf.unsplit)
    B, T, R = c['B'], c['T'], c['R']
    y = torch.einsum('bct,cm->bmt', _t(ins['x']), _t(ins['w'])[0])
    if c['bias']:
        y = y + _t(ins['bias'])[None, :, None]
    if c['cond_T']:
        ct = c['cond_T']
        y = y + torch.as_strided(_t(ins['cond']), (B, R, ct), (c['cond_bstride'], ct, 1)).repeat_interleave(T // ct, dim=2)
    if c['net_in']:
        y = y + _t(ins['net_in'])
    if c['mask']:
        y = y * (_t(ins['mask']) > 0)
    np.testing.assert_allclose(ref['net_out'], y.numpy(), rtol=0, atol=1e-11)
    np.testing.assert_allclose(ref['plane_src'], (torch.relu(y) if c['relu'] else y).numpy(), rtol=0, atol=1e-11)


def test_the_split_reference_is_x3_refs_contraction():
    c = Rf.out_cases()[3]
    ins = Rf.inputs(c, 'normal')
    pre, _, n = Rf.conv_pre(ins['x'], ins['w'], [0], ins['sx'], ins['sw'])
    want = X.contract(ins['w'][0].T, ins['x'][1], ins['sw'], ins['sx'])
    assert n == 3 * c['Cin']
    np.testing.assert_allclose(pre[1], want, rtol=0, atol=1e-13 * np.abs(want).max())


# ---------------------------------------------------------------------------------------------------- plane images
@pytest.mark.parametrize('kc0,KC,scale,dev', ((0, 0, 1.0, 1.0), (32, 96, 1.0, 1.0), (0, 0, 2.0, 4.0), (16, 48, 1.0, 0.5)))
def test_plane_images_are_the_split_of_the_fp32_value(kc0, KC, scale, dev):
    rng = np.random.default_rng(3)
    B, C, T = 2, 128, 256
    v = rng.standard_normal((B, C, T))
    img = Rf.plane_image(v, scale, dev, kc0, KC)
    KC_ = KC or C // 8
    assert img.shape == (2, KC_, B * T, 8) and img.dtype == np.uint16
    prefill = np.full((2, KC_, B * T, 8), Rf.PLANE_FILL, np.uint16)
    assert np.array_equal(img, X.act_planes(v.astype(F32), scale, dev, kc0, KC_, into=prefill))
    outside = np.ones(KC_, bool)
    outside[kc0:kc0 + C // 8] = False
    assert (img[:, outside] == Rf.PLANE_FILL).all() and (prefill == Rf.PLANE_FILL).all()
    dec = Rf.decode_planes(img, kc0, C, B, T, scale * dev)
    assert (np.abs(dec - v.astype(F32)) <= Rf.SPLIT_REL * np.abs(v) + Rf.F16_HALF_STEP / (scale * dev)).all()


def test_check_sees_guards_unwritten_outputs_and_plane_chunks():
    n, G = 32, Rf.GUARD
    full = np.full(n + 2 * G, Rf.SENTINEL, F32)
    assert Rf.check(full, n, None, None, 'normal', 'x') == 0.0
    want = np.arange(n, dtype=np.float64)
    full[G:G + n] = want
    assert Rf.check(full, n, want, np.ones(n), 'ints', 'x') == 0.0
    bad = full.copy()
    bad[G - 1] = 0.0
    with pytest.raises(AssertionError, match='guard'):
        Rf.check(bad, n, want, np.ones(n), 'ints', 'x')
    bad = full.copy()
    bad[G + 3] += 1
    with pytest.raises(AssertionError, match='differ'):
        Rf.check(bad, n, want, np.full(n, 2.0), 'ints', 'x')
    assert Rf.check(bad, n, want, np.full(n, 2.0), 'normal', 'x') == 0.5
    with pytest.raises(AssertionError, match='over the bar'):
        Rf.check(bad, n, want, np.full(n, 0.5), 'normal', 'x')
    bad[G + 3] = np.nan
    with pytest.raises(AssertionError, match='over the bar'):
        Rf.check(bad, n, want, np.full(n, 2.0), 'normal', 'x')
    with pytest.raises(AssertionError, match='not an output'):
        Rf.check(full, n, None, None, 'normal', 'x')
    val = np.ones((1, 16, 4))
    val[0, 0, 0] = -0.0                                             # [plane][chunk 1][row 0][lane 0] of the image
    img = Rf.plane_image(val, kc0=1, KC=4)
    assert img[0, 1, 0, 0] == 0x8000 and img[1, 1, 0, 0] == 0 and img[0, 1, 0, 1] == 0x3c00 and img[1, 1, 0, 1] == 0
    buf = np.concatenate([np.full(2 * G, Rf.PLANE_FILL, np.uint16), img.reshape(-1), np.full(2 * G, Rf.PLANE_FILL, np.uint16)])
    Rf.check_planes(buf, img, 'p')
    for pos in (2 * G - 1, 2 * G, buf.size - 2 * G):           # a guard, a chunk the launch does not own, the other guard
        b2 = buf.copy()
        b2[pos] ^= 1
        with pytest.raises(AssertionError):
            Rf.check_planes(b2, img, 'p')
    b2 = buf.copy()
    b2[2 * G + img.size // 2 + 4 * 8] = 0x8000                     # the second plane of an element that is a zero: either sign
    Rf.check_planes(b2, img, 'p')
    b2[2 * G + 4 * 8] ^= 0x8000                                    # the leading plane: its sign is the value's
    with pytest.raises(AssertionError):
        Rf.check_planes(b2, img, 'p')
    b2 = buf.copy()
    b2[2 * G + img.size // 2 + 4 * 8 + 1] = 0x8000                 # ... of an element that is 1.0: the residual is +0, bit for bit
    with pytest.raises(AssertionError):
        Rf.check_planes(b2, img, 'p')
    b2 = buf.copy()
    b2[2 * G + img.size // 2 + 4 * 8] = 0x0001                     # a zero element's second plane must still BE a zero
    with pytest.raises(AssertionError):
        Rf.check_planes(b2, img, 'p')


# ---------------------------------------------------------------------------------------------------- discrimination
def _uses(wrong, c):
    """Does the case exercise what the wrong evaluation gets wrong?"""
    g, epi = c['kernel'] == 'gate', c.get('epi')
    ks, d = c.get('ks', 1), c.get('dilation', 1)
    return {
        'leak': ks > 1 and c['B'] > 1 and d < c['T'],
        'drop_last_tap': ks > 1,
        'drop_last_kstep': True,
        'no_h2h1': True,
        'gate_rows_unpermuted': g,
        'cond_frame_plus_one': bool(c.get('cond_T')) and c.get('cond_T') > 1,
        'cond_bstride_ignored': bool(c.get('cond_T')) and c['B'] > 1 and c['cond_bstride'] > (2 if g else 1) * c['R'] * c['cond_T'],
        'bias_filter_half_only': g and c['bias'],
        'dir_sign': epi == 0 and ks > 1 and d < c['T'],
        'net_in_dropped': (epi == 0 and c['net_in'] != 'none') or (epi == 2 and c['net_in']),
        'skip_overwritten': epi == 0 and c['S'] > 0,
        'mask_ge_zero': epi == 2 and c['mask'],
        'relu_on_net_out': epi == 2 and c['relu'],
        'kc0_ignored:xp': epi == 0 and c['xp_kc0'] > 0,
        'kc0_ignored:out_planes': g and c['out_planes_kc0'] > 0 and 'out_planes' in c['subset'],
        'kc0_ignored:planes': epi == 0 and c['planes'] and c['planes_kc0'] > 0,
        'kc0_ignored:aux0': epi == 1 and c['aux'] == 'planes',
        'plane_scale_ignored': epi == 0 and c['planes'] and c['plane_scale'] not in (0.0, 1.0),
        'bwd_gate_half_uses_filter_factor': epi == 1,
        'bwd_underflow_not_zeroed': epi == 1 and c['aux'] != 'tanh' and c['underflow'],
    }[wrong]


def _outputs(c, r):
    """[(value, bar)] of a reference result; plane placements and scales as images (bar None: compared bit for bit)."""
    if c['kernel'] == 'gate':
        return [(r[n], r['bar_' + n]) for n in ('out0', 'save0', 'save1')]
    if c['epi'] == 0:
        return ([(r['skip'], r['bar_skip'])] if c['S'] else []) + ([(r['net_out'], r['bar_net'])] if c['R'] else [])
    if c['epi'] == 1:
        return [(r['dpre'], r['bar'])]
    return [(r['net_out'], r['bar_net']), (r['plane_src'], r['bar_net'])]


def _image(c, ins, r, wrong=None):
    w = wrong if wrong in ('plane_scale_ignored', 'kc0_ignored:out_planes', 'kc0_ignored:planes') else None
    if c['kernel'] == 'gate':
        return Rf.plane_image(r['out0'], kc0=c['out_planes_kc0'], KC=c['out_planes_KC'], wrong=w)
    ps, osc = Rf.plane_scales(c, ins)
    return Rf.plane_image(r['net_out'], ps, osc, c['planes_kc0'], c['planes_KC'], wrong=w)


def _told_apart(c, kind, wrong, mode):
    ins = Rf.inputs(c, kind)
    right, off = Rf.reference(c, ins, mode), Rf.reference(c, ins, mode, wrong=wrong)
    if wrong in ('plane_scale_ignored', 'kc0_ignored:out_planes', 'kc0_ignored:planes'):
        return not np.array_equal(_image(c, ins, right), _image(c, ins, right, wrong))
    for (v, bar), (w, _) in zip(_outputs(c, right), _outputs(c, off)):
        if kind == 'ints' and not np.array_equal(v, w, equal_nan=False):
            return True
        if kind == 'normal' and not (np.abs(w - v) <= bar).all():
            return True
    return False


# what the integer family cannot show, by construction: its low planes are all zero, and its sigmoids are 1/2, 1/4, 1/8
NOT_IN_INTS = ('no_h2h1', 'bwd_underflow_not_zeroed')


@pytest.mark.parametrize('wrong', Rf.WRONG)
@pytest.mark.parametrize('kind', Rf.KINDS)
def test_every_wrong_evaluation_is_told_apart(wrong, kind):
    if kind == 'ints' and wrong in NOT_IN_INTS:
        for c in CASES:         # ... which is asserted, not assumed
            ins = Rf.inputs(c, 'ints')
            if wrong == 'no_h2h1':
                assert not X.split(X.scaled(ins['x'], ins['sx']))[1].any() and not X.split(X.scaled(ins['w'], ins['sw']))[1].any()
            elif c.get('epi') == 1:
                assert float(ins['sg'].min()) >= 0.125
        return
    users = [c for c in CASES if _uses(wrong, c)]
    assert users, 'no case uses ' + wrong
    modes = [m for _, m in Rf.MODES] if wrong == 'gate_rows_unpermuted' else [0]
    for mode in modes:
        assert any(_told_apart(c, kind, wrong, mode) for c in users[:6]), '%s is not told apart on any %s case (mode %d)' % (wrong, kind, mode)


# ---------------------------------------------------------------------------------------------------- fp32 emulations
def _rows(c):
    M = 2 * c['R'] if c['kernel'] == 'gate' else c['R'] + c.get('S', 0)
    return np.array([0, M // 2 - 1, M // 2, M - 1])


def _emu_fraction(c, kind, order):
    """The worst err / bar of the fp32 emulation of four output rows against the float64 reference."""
    ins = Rf.inputs(c, kind)
    ref = Rf.reference(c, ins)
    ms = _rows(c)
    e = Rf.emulate(c, ins, ms, order)
    B, R = c['B'], c['R']
    if c['kernel'] == 'gate':
        pairs = [(e['pre'], np.concatenate([ref['f'], ref['g']], 1)[:, ms], np.concatenate([ref['e_f'], ref['e_g']], 1)[:, ms])]
    elif c['epi'] == 0:
        S = c['S']
        full = np.concatenate([ref.get('skip', np.zeros((B, 0, c['T']))), ref.get('net_out', np.zeros((B, 0, c['T'])))], 1)
        bar = np.concatenate([ref.get('bar_skip', np.zeros((B, 0, c['T']))), ref.get('bar_net', np.zeros((B, 0, c['T'])))], 1)
        assert full.shape[1] == S + R
        pairs = [(e['rows'], full[:, ms], bar[:, ms])]
    elif c['epi'] == 2:
        pairs = [(e['net_out'], ref['net_out'][:, ms], ref['bar_net'][:, ms])]
    else:
        pairs = [(e['qf'], ref['dpre'][:, ms], ref['bar'][:, ms]), (e['qg'], ref['dpre'][:, R + ms], ref['bar'][:, R + ms])]
    worst = 0.0
    for got, want, bar in pairs:
        err = np.abs(got.astype(np.float64) - want)
        assert np.isfinite(err).all()
        if kind == 'ints':
            assert not err.any(), '%s: the fp32 emulation (%s) of an integer case is not exact' % (c['name'], order)
            continue
        live = bar > 0
        assert not err[~live].any()
        worst = max(worst, float((err[live] / bar[live]).max()))
    return worst


@pytest.mark.parametrize('order', ('forward', 'reversed', 'pairwise'))
@pytest.mark.parametrize('name', [c['name'] for c in CASES])
def test_sequential_fp32_stays_inside_the_bars(name, order):
    """Normal operands: under EMU_FRACTION of every bar.  Integer operands: exact, in every order and -- epi 1 -- in either association
    of the products ('reversed' also multiplies the factors before the gradient)."""
    c = BY_NAME[name]
    assert _emu_fraction(c, 'normal', order) < Rf.EMU_FRACTION
    assert _emu_fraction(c, 'ints', order) == 0.0


# ---------------------------------------------------------------------------------------------------- conditions on the tables
def test_tables_are_legal_named_once_small_and_cover_every_option():
    assert len(BY_NAME) == len(CASES)
    for c in CASES:
        assert Rf.legality(c['kernel'], c) is None, c['name']
        assert c['B'] in (1, 2, 3) and c['T'] in (256, 512, 768) and max(c['R'], c.get('S', 0), c.get('Cin', 0)) <= 768, c['name']
        assert Rf.case_bytes(c) <= Rf.MAX_BYTES, c['name']
    for name, kernel, kw in Rf.refusal_cases():
        assert Rf.legality(kernel, kw) is not None, name
    assert set(Rf.REFUSED_WITH) == {r[0] for r in Rf.refusal_cases()} and len(Rf.REFUSED_WITH) == len(Rf.refusal_cases())
    # every case runs on both block heights and both families (the GPU module's parametrisation): the table itself must name every option
    assert [m for _, m in Rf.MODES] == [0, X.X3_HALF_BLOCKS] and Rf.KINDS == ('ints', 'normal')
    have = set().union(*(Rf.options_of(c) for c in CASES))
    assert not Rf.REQUIRED_OPTIONS - have, sorted(Rf.REQUIRED_OPTIONS - have)


def _exact32(a):
    a = np.asarray(a, np.float64)
    return np.array_equal(a.astype(F32).astype(np.float64), a)


@pytest.mark.parametrize('name', [c['name'] for c in CASES])
def test_integer_cases_are_exact_in_fp32_and_gate_cases_sensitive(name):
    c = BY_NAME[name]
    ins = Rf.inputs(c, 'ints')
    for k in ('x', 'w'):
        h1, h2 = X.split(X.scaled(ins[k], ins['s' + k]))
        assert not h2.any() and np.isfinite(h1.astype(F32)).all()
    r = Rf.reference(c, ins)
    if c['kernel'] != 'gate':
        for v, _ in _outputs(c, r):
            assert _exact32(v), name
        if c['epi'] == 1:
            assert _exact32(r['dg']) and np.abs(r['dg']).max() < 2 ** 13
        return
    f, g, w = r['f'], r['g'], ins['winv']
    assert _exact32(f) and _exact32(g) and np.array_equal(np.round(f / w), f / w)
    pre, _, _ = Rf.conv_pre(ins['x'], ins['w'], Rf.shifts(c['ks'], c['dilation']), 1.0, 1.0, 1.0)
    assert np.array_equal(pre, np.round(pre))
    # the cap the integer family rests on: +-1 in the integer contraction moves the activation by more than twice its bar
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))  # noqa: E731
    moved0 = np.minimum(np.abs(np.tanh(f + w) - r['save0']), np.abs(np.tanh(f - w) - r['save0'])) > 2 * r['bar_save0']
    moved1 = np.minimum(np.abs(sig(g + w) - r['save1']), np.abs(sig(g - w) - r['save1'])) > 2 * r['bar_save1']
    assert moved0.mean() >= 0.95 and moved1.mean() >= 0.95, (name, moved0.mean(), moved1.mean())
    sd = float(pre.std()) * w
    assert 0.5 < sd <= 1.0, (name, sd)
