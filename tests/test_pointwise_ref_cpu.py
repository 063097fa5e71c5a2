"""tests/pointwise_ref.py checked on the CPU: its float64 references against what the project already trusts (torch in float64,
oracle.ref_ops and autograd) to 1e-12, and the conditions its case tables rest on -- the exact-integer bound, every (c) bar
against a plain fp32 emulation of its formula (at most pointwise_ref.EMU_FRACTION of the bar), legality under the entries'
VQW_CHECKs, and that every template instance, both rowsum kernels, the softmax kernel's chunk and tail loops and the second grid-stride trips are reached."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pointwise_ref as PR  # noqa: E402
from oracle import ref_ops as R  # noqa: E402

F32 = np.float32
TOL = 1e-12


def _close(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = float(np.abs(a - b).max()) / max(1.0, float(np.abs(b).max()))
    assert err <= TOL, '%s: %.3e' % (what, err)


def _t64(a, grad=False):
    return torch.from_numpy(np.asarray(a, np.float64)).requires_grad_(grad)


# ---------------------------------------------------------------------------------------------------- references
@pytest.mark.parametrize('c', PR.softmax_cases()[::3], ids=[c['name'] for c in PR.softmax_cases()[::3]])
def test_softmax_reference_is_torch_cross_entropy(c):
    x, lab = PR.softmax_inputs(c)
    ref = PR.softmax_ref(x, lab)
    B, Q, T = x.shape
    xt = _t64(x, True)
    rows = xt.permute(0, 2, 1).reshape(-1, Q)
    loss = F.cross_entropy(rows, torch.from_numpy(lab.reshape(-1).astype(np.int64)), reduction='none')
    loss.sum().backward()
    _close(ref['loss'].reshape(-1), loss.detach().numpy(), 'loss')
    _close(ref['p'], torch.softmax(xt.detach(), 1).numpy(), 'probs')
    _close(ref['p'] - PR.onehot(lab, Q), xt.grad.numpy(), 'dlogits')


def _shifted(c, x):
    """-> [B][T][1] float64 tensor; a positive offset becomes a VALID conv of x[offset:] with the zeros it runs into appended."""
    T_in, off = PR.conv_cin1_geometry(c)
    if c['pad'] == 'plus2':
        need = c['stride'] * (c['T_out'] - 1) + c['k']
        x = np.concatenate([x[:, off:], np.zeros((x.shape[0], need), x.dtype)], 1)[:, :need]
    return _t64(x)[:, :, None]


@pytest.mark.parametrize('c', PR.conv_cin1_cases(), ids=[c['name'] for c in PR.conv_cin1_cases()])
def test_conv_cin1_reference_is_the_oracles_conv(c):
    ins = PR.conv_cin1_inputs(c, 'normal')
    k, Fo, To = c['k'], c['F'], c['T_out']
    w = _t64(ins['w'].reshape(k, 1, Fo), True)
    b = None if ins['bias'] is None else _t64(ins['bias'])
    xt = _shifted(c, ins['x'])
    if c['pad'] != 'causal':
        y = R.keras_conv1d(xt, w, b, stride=c['stride'], padding='same' if c['pad'] == 'same' else 'valid')
    else:
        y = R.conv1d_v2(xt, w, b, stride=c['stride'])
    y = y[:, :To, :]
    assert y.shape[1] == To
    for relu in (False, True):
        for scale in (False, True):
            ref = PR.conv_cin1_fwd_ref(c, ins, relu, scale)
            r = torch.relu(y) if relu else y
            _close(ref['r'], r.detach().permute(0, 2, 1).numpy(), 'r')
            want = r * _t64(ins['scale']) + _t64(ins['shift']) if scale else r
            _close(ref['out'], want.detach().permute(0, 2, 1).numpy(), 'out')
    (y * _t64(ins['dout']).permute(0, 2, 1)).sum().backward()
    _close(PR.conv_cin1_wgrad_ref(c, ins)['dw'], ins['dw0'].astype(np.float64) + w.grad.reshape(k, Fo).numpy(), 'dw')


@pytest.mark.parametrize('T', PR.BN_SUMS_T)
def test_bn_sums_reference_is_autograd_of_relu_then_affine(T):
    ins = PR.bn_sums_inputs(T, 'ints')           # integers: the fp32 product of dz is exact, so float64 autograd gives the same dz
    z = _t64(ins['y'], True)                     # r_is_y: y = r = relu(z) has the mask of z
    sc, sh = _t64(ins['scale'], True), torch.zeros(PR.BN_SUMS_BC[1], dtype=torch.float64, requires_grad=True)
    out = sc[None, :, None] * torch.relu(z) + sh[None, :, None]
    (out * _t64(ins['dx'])).sum().backward()
    relu_y = dict(ins, y=np.maximum(ins['y'], 0))
    ref = PR.bn_sums_ref(relu_y, 'r_is_y')
    _close(ref['dz'], z.grad.numpy(), 'dz')
    _close(ref['dscale'] - ins['dscale0'], sc.grad.numpy(), 'dscale')
    _close(ref['dbeta'] - ins['dbeta0'], sh.grad.numpy(), 'dbeta')
    _close(ref['dbias'] - ins['dbias0'], z.grad.sum((0, 2)).numpy(), 'dbias')
    # the plain pass is the same dz
    assert np.array_equal(PR.bn_relu_bwd_ref(ins['dx'], relu_y['y'], ins['scale']), ref['dz'])


@pytest.mark.parametrize('c', PR.rowsum_cases(), ids=[c['name'] for c in PR.rowsum_cases()])
def test_rowsum_reference_is_reshape_sum(c):
    ins = PR.rowsum_inputs(c, 'normal')
    for with_y, _, _, alpha in PR.rowsum_variants(c):
        ref = PR.rowsum_ref(c, ins, with_y, alpha)
        t = _t64(ins['x']) * (_t64(ins['y']) if with_y else 1.0)
        if c['seg']:
            _close(ref['seg'], t.reshape(c['B'], c['C'], c['T'] // c['seg'], c['seg']).sum(-1).numpy(), 'seg_out')
        _close(ref['total'], (_t64(ins['total0']) + alpha * t.sum((0, 2))).numpy(), 'total')


def test_transpose_and_relu_bn_references():
    for b, r, c in PR.TRANSPOSE_CASES:
        src = PR.randn(1, b, r, c)
        assert torch.equal(torch.from_numpy(PR.transpose_ref(src, b, r, c)), torch.from_numpy(src).transpose(1, 2).contiguous())
    x, sc, sh = PR.with_zeros(PR.randn(2, 3, 5, 37), 3), PR.randn(4, 5), PR.randn(5, 5)
    r, xn, bar = PR.relu_bn_fwd_ref(x, sc, sh)
    _close(r, torch.relu(_t64(x)).numpy(), 'r')
    _close(xn, (_t64(sc)[None, :, None] * torch.relu(_t64(x)) + _t64(sh)[None, :, None]).numpy(), 'x')
    assert bar.shape == x.shape and PR.relu_bn_fwd_ref(x, None, None)[2] is None


# ---------------------------------------------------------------------------------------------------- (b): the integer bound
def _exact(total_abs, what):
    """Every value is a multiple of 1/2: exact in fp32 in every order while 2 * sum |terms| < 2^24."""
    assert 2.0 * float(np.max(total_abs)) < 2.0 ** 24, what


def _halves_only(*arrays):
    for a in arrays:
        if a is not None:
            assert np.array_equal(np.asarray(a) * 2, np.round(np.asarray(a) * 2)) and np.abs(a).max() <= 4


def test_integer_cases_stay_exact_in_fp32():
    for c in PR.rowsum_cases():
        ins = PR.rowsum_inputs(c, 'ints')
        _halves_only(*ins.values())
        for with_y, _, _, alpha in PR.rowsum_variants(c):
            ref = PR.rowsum_ref(c, ins, with_y, alpha)
            _exact(ref['total_abs'], c['name'])
            if c['seg']:
                _exact(ref['seg_abs'], c['name'])
    for T in PR.BN_SUMS_T:
        ins = PR.bn_sums_inputs(T, 'ints')
        _halves_only(*ins.values())
        for form in PR.BN_SUMS_FORMS:
            ref = PR.bn_sums_ref(ins, form)
            for n in ('dscale', 'dbeta', 'dbias'):
                _exact(ref[n + '_abs'], (T, form, n))
    for c in PR.conv_cin1_cases():
        ins = PR.conv_cin1_inputs(c, 'ints')
        _halves_only(*ins.values())
        assert np.array_equal(ins['x'], np.round(ins['x'])) and np.array_equal(ins['w'], np.round(ins['w']))
        _exact(PR.conv_cin1_fwd_ref(c, ins, True, True)['out_abs'], c['name'])
        a = PR.conv_cin1_wgrad_ref(c, ins)['dw_abs']
        _exact(a, c['name'])
        assert a.max() < 1e5
    for shape in PR.BN_SHAPES:
        x, sc, sh = PR.ints(1, *shape), PR.halves(2, shape[1]), PR.halves(3, shape[1])
        _, xn, _ = PR.relu_bn_fwd_ref(x, sc, sh)
        assert np.array_equal(xn, xn.astype(F32).astype(np.float64)) and np.array_equal(xn, PR.relu_bn_fwd_emulation(x, sc, sh))


# ---------------------------------------------------------------------------------------------------- (c): emulation under the bars
def _under(emu, ref, bar, what):
    r = PR.ratio_of(emu, ref, bar, what)
    assert r <= PR.EMU_FRACTION, '%s: the fp32 emulation reaches %.2f of its bar' % (what, r)
    return r


@pytest.mark.parametrize('c', PR.softmax_cases(), ids=[c['name'] for c in PR.softmax_cases()])
def test_softmax_bars_hold_a_plain_fp32_emulation(c, record_property):
    x, lab = PR.softmax_inputs(c)
    ref = PR.softmax_ref(x, lab)
    bars = PR.softmax_bars(x, lab, ref, c['grad_scale'])
    emu = PR.softmax_emulation(x, lab, c['grad_scale'])
    rp = _under(emu['p'], ref['p'], bars['p'], 'probs')
    rd = _under(emu['dlogits'], (ref['p'] - PR.onehot(lab, c['Q'])) * c['grad_scale'], bars['dlogits'], 'dlogits')
    rl = _under(emu['loss'], ref['loss'], bars['loss'], 'loss')
    rs = _under(emu['loss_sum'], PR.SOFTMAX_LOSS0 + ref['loss'].sum(), bars['loss_sum'], 'loss_sum')
    record_property('emulation_over_bar', dict(p=rp, dlogits=rd, loss=rl, loss_sum=rs))


def test_sum_bars_hold_a_sequential_fp32_emulation():
    for c in PR.rowsum_cases():
        ins = PR.rowsum_inputs(c, 'normal')
        B, C, T, seg = c['B'], c['C'], c['T'], c['seg']
        for with_y, _, _, alpha in PR.rowsum_variants(c):
            ref = PR.rowsum_ref(c, ins, with_y, alpha)
            t = (ins['x'] * ins['y']).astype(F32) if with_y else ins['x']
            if seg:
                emu = PR.sequential_sum_f32(np.moveaxis(t.reshape(B, C, T // seg, seg), -1, 0))
                _under(emu, ref['seg'], ref['seg_bar'], c['name'] + ' seg_out')
            rows = PR.sequential_sum_f32(np.moveaxis(t, -1, 0))                    # [B][C]
            tot = ins['total0'].copy()
            for b in range(B):
                tot = (tot + (F32(alpha) * rows[b]).astype(F32)).astype(F32)
            _under(tot, ref['total'], ref['total_bar'], c['name'] + ' total')
    for T in PR.BN_SUMS_T:
        ins = PR.bn_sums_inputs(T, 'normal')
        for form in PR.BN_SUMS_FORMS:
            ref = PR.bn_sums_ref(ins, form)
            terms = dict(dscale=(ins['dx'] * ins['y']).astype(F32), dbeta=ins['dx'], dbias=ref['dz'])
            for n, t in terms.items():
                emu = PR.sequential_sum_f32([ins[n + '0']] + list(np.moveaxis(t, 1, -1).reshape(-1, t.shape[1])))
                _under(emu, ref[n], ref[n + '_bar'], 'bn_sums T=%d %s %s' % (T, form, n))
    for shape in PR.BN_SHAPES:
        x, sc, sh = PR.with_zeros(PR.randn(1, *shape), 2), PR.randn(3, shape[1]), PR.randn(4, shape[1])
        _, xn, bar = PR.relu_bn_fwd_ref(x, sc, sh)
        _under(PR.relu_bn_fwd_emulation(x, sc, sh), xn, bar, 'relu_bn_fwd x')


@pytest.mark.parametrize('c', PR.conv_cin1_cases(), ids=[c['name'] for c in PR.conv_cin1_cases()])
def test_conv_cin1_bars_hold_a_sequential_fp32_emulation(c):
    ins = PR.conv_cin1_inputs(c, 'normal')
    acc = PR.conv_cin1_fwd_emulation(c, ins)
    for relu in (False, True):
        ref = PR.conv_cin1_fwd_ref(c, ins, relu, True)
        r = np.maximum(acc, F32(0)) if relu else acc
        _under(r, ref['r'], ref['r_bar'], 'r')
        out = ((ins['scale'][None, :, None] * r).astype(F32) + ins['shift'][None, :, None]).astype(F32)
        _under(out, ref['out'], ref['out_bar'], 'out')
    xg = PR._windows(c, ins['x']).astype(F32)                                       # [B][T][k]
    terms = (xg[:, :, :, None] * np.moveaxis(ins['dout'], 1, -1)[:, :, None, :]).astype(F32).reshape(-1, c['k'], c['F'])
    ref = PR.conv_cin1_wgrad_ref(c, ins)
    _under(PR.sequential_sum_f32([ins['dw0']] + list(terms)), ref['dw'], ref['dw_bar'], 'dw')


# ---------------------------------------------------------------------------------------------------- legality and reach
def test_every_case_is_legal():
    for c in PR.softmax_cases():
        assert PR.softmax_legal(c), c['name']
        x, lab = PR.softmax_inputs(c)
        assert lab.min() >= 0 and lab.max() < c['Q'] and np.isfinite(x).all()
    for c in PR.rowsum_cases():
        for _, with_seg, with_total, _ in PR.rowsum_variants(c):
            assert (with_seg or with_total) and PR.rowsum_legal(c, with_seg), c['name']
    for c in PR.conv_cin1_cases():
        assert PR.conv_cin1_legal(c), c['name']
        assert c['T_out'] % 4 != 0 or PR.conv_cin1_out_off(c) == 0, c['name']        # vector rows: 16-byte aligned outputs
    for T in PR.BN_SUMS_T:
        assert T > 0
    names = [c['name'] for f in (PR.softmax_cases, PR.rowsum_cases, PR.conv_cin1_cases) for c in f()]
    assert len(names) == len(set(names))


def test_the_tables_reach_every_kernel_instance_and_loop():
    # softmax: tail only, chunks only, chunks + tail; short, full and partial tiles; labels on every boundary
    paths = [PR.softmax_paths(c) for c in PR.softmax_cases()]
    assert any(p['tail'] and not p['chunks'] for p in paths) and any(p['chunks'] and not p['tail'] for p in paths)
    assert any(p['chunks'] and p['tail'] for p in paths)
    assert any(c['T'] < 64 for c in PR.softmax_cases()) and any(p['partial_tile'] and p['full_tile'] for p in paths)
    assert {(c['Q'], c['T']) for c in PR.softmax_cases()} >= {(q, t) for q in PR.SOFTMAX_Q for t in PR.SOFTMAX_T}
    for Q in PR.SOFTMAX_Q:
        mine = [c for c in PR.softmax_cases() if c['Q'] == Q]
        assert {c['B'] for c in mine} == {1, 3} and {c['gs'] for c in mine} == {'quarter', 'mean'}
        assert {c['logits'] for c in mine} == set(PR.SOFTMAX_SETS)
        seen = set()
        for c in mine:
            seen |= set(PR.softmax_inputs(c)[1].reshape(-1).tolist())
        assert seen >= set(PR.boundary_labels(Q)), Q
    assert PR.boundary_labels(68) == sorted({w * 17 + e for w in range(4) for e in (0, 15, 16)})
    # the wide sets underflow: the other waves' sums vanish against the maximum's wave
    for c in PR.softmax_cases():
        if c['logits'].startswith('wide') and c['Q'] >= 8:
            x, _ = PR.softmax_inputs(c)
            w, qn = int(c['logits'][4:]), c['Q'] // 4
            other = np.delete(x, np.s_[w * qn:(w + 1) * qn], 1)
            assert float((other.max(1) - x.max(1)).max()) < -104       # exp(-104) < 2^-149: zero in fp32
    # rowsum: both kernels, each named case on the kernel it is in the table for
    kernels = set()
    for c in PR.rowsum_cases():
        for with_y, with_seg, _, _ in PR.rowsum_variants(c):
            kernels.add(PR.rowsum_kernel(c, with_y, with_seg))
        named = [PR.rowsum_kernel(c, True, c['seg'] > 0)]
        if not c['yoff']:
            named.append(PR.rowsum_kernel(c, False, c['seg'] > 0))
        assert set(named) == {c['kernel']}, c['name']
        assert {a for _, _, _, a in PR.rowsum_variants(c)} == set(PR.ROWSUM_ALPHAS)
    assert kernels == {'fast', 'general'}
    fast = [c for c in PR.rowsum_cases() if c['kernel'] == 'fast']
    assert any(c['T'] // 4 < 64 for c in fast) and any(c['T'] // 4 > 64 and c['T'] // 4 % 64 for c in fast)
    assert any(c['B'] * c['C'] % 4 for c in fast) and {c['seg'] for c in fast} >= {0, 4, 8, 64, 256}
    # conv_cin1: all five instances of each template, each with a ragged and a multiple-of-4 length
    cc = PR.conv_cin1_cases()
    for inst in PR.CONV_CIN1_INSTANCES:
        mine = [c for c in cc if PR.conv_cin1_instance(c) == inst]
        assert any(c['T_out'] % 4 for c in mine) and any(c['T_out'] % 4 == 0 for c in mine), inst
    for ks in {(c['k'], c['stride']) for c in cc}:
        mine = [c for c in cc if (c['k'], c['stride']) == ks]
        assert any(c['T_out'] % 4 for c in mine) and any(c['T_out'] % 4 == 0 for c in mine), ks
    assert {(c['k'], c['stride']) for c in cc} == {(5, 2), (3, 1), (8, 1), (5, 3), (8, 4), (32, 1), (9, 1), (9, 2), (32, 4)}
    assert {c['T_out'] for c in cc} >= {1, 3, 37, 1024, 1025, 1028, 2052} and {c['F'] for c in cc} == {1, 16, 17, 40}
    assert {c['B'] for c in cc} == {1, 3} and {c['pad'] for c in cc} == {'causal', 'same', 'plus2'}
    assert any(not c['bias'] for c in cc) and any(c['bias'] for c in cc)
    for c in cc:
        T_in, off = PR.conv_cin1_geometry(c)
        if c['pad'] == 'plus2':
            assert c['stride'] * (c['T_out'] - 1) + c['k'] - 1 + off >= T_in, c['name']     # the window runs past T_in
    # grid-stride loops: a second trip
    assert np.prod(PR.BN_SHAPES[-1]) > PR.GRID_STRIDE_ELEMENTS and np.prod(PR.WAVENET_INPUTS_BT[-1]) > PR.GRID_STRIDE_ELEMENTS
    paths = {(n, a): PR.adam_path(n, a) for n in PR.ADAM_N for a in PR.ADAM_ALIGN}
    assert any(p['second_trip'] and p['tail'] for p in paths.values())
    assert any(not p['vector'] and n >= 4 for (n, a), p in paths.items() if a != 'aligned')
    assert any(not p['vector'] and a == 'aligned' for (n, a), p in paths.items())                  # n < 4
    assert all(not p['vector'] for (n, a), p in paths.items() if a != 'aligned')
