"""tests/sconv_ref.py held to independent statements of the same operations, on the CPU: torch's conv1d and its autograd in
float64, the split model of the number format, the VQW_X3_S2D image of x3_ref.act_planes, the entry point's rules (legality,
path) at three CU counts, a sequential fp32 emulation under EMU_FRACTION of every bar, and the deliberately wrong evaluations
(sconv_ref.WRONG) each told apart from the right one."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_ref  # noqa: E402
import sconv_ref as S  # noqa: E402
import x3_ref as X  # noqa: E402

F32 = np.float32
CUS = (32, 256, 304)
EMU_ROWS = 24           # output channels per case the fp32 emulation and the mutations evaluate (each is a contraction of its own)


def _ids(cases):
    return [c['name'] for c in cases]


def _t(a):
    return torch.from_numpy(np.asarray(a, np.float64))


def _padded(x, left, right):
    """F.pad with zeros; a negative amount crops."""
    if right < 0:
        x, right = x[..., :right], 0
    return Fn.pad(x, (left, right))


def _torch_conv(x, w, pad_left, T):
    """conv1d(stride 2) of x [B][C][L] with w [ks][C][M] giving exactly T outputs."""
    ks = w.shape[0]
    right = 2 * (T - 1) + ks - 1 - pad_left - (x.shape[-1] - 1)
    return Fn.conv1d(_padded(x, pad_left, right), w.permute(2, 1, 0), None, stride=2)


def _msel(c, n=EMU_ROWS):
    rng = np.random.default_rng(S.seed_of('msel', c['name']))
    return np.sort(rng.choice(c['M'], min(n, c['M']), replace=False))


FWD = [c for c in S.table_cases() if not c['dgrad']]


@pytest.mark.parametrize('c', FWD, ids=_ids(FWD))
def test_forward_and_input_gradient_match_torch_float64(c):
    """sconv_fwd with unsplit operands against conv1d over F.pad(x, (pad_left, ks - 2 - pad_left)) (cropped where that is
    negative), bias -> relu -> affine; sconv_dgrad against autograd of the same expression."""
    ins = S.sconv_inputs(c, 'normal')
    x, w = _t(ins['x']).requires_grad_(True), _t(ins['w'])
    y = _torch_conv(x, w, c['pad_left'], c['T'])
    assert y.shape[-1] == c['T']
    r = torch.relu(y + _t(ins['bias'])[None, :, None])
    want = _t(ins['bn_scale'])[None, :, None] * r + _t(ins['bn_shift'])[None, :, None]
    out, save_r, _, _, ab = S.sconv_fwd(ins['x'], ins['w'], ins['bias'], ins['bn_scale'], ins['bn_shift'], True, c['pad_left'],
                                        split=S.unsplit, full=True)
    scale = max(1.0, ab.max())
    assert np.abs(save_r - r.detach().numpy()).max() <= 1e-12 * scale
    assert np.abs(out - want.detach().numpy()).max() <= 1e-12 * scale * max(1.0, np.abs(ins['bn_scale']).max())
    out0, r0 = S.sconv_fwd(ins['x'], ins['w'], None, None, None, False, c['pad_left'], split=S.unsplit)
    assert np.abs(out0 - y.detach().numpy()).max() <= 1e-12 * scale and out0 is r0
    rng = np.random.default_rng(5)
    dy = rng.standard_normal(y.shape).astype(F32)
    want_dx, = torch.autograd.grad(y, x, _t(dy))
    wt = np.ascontiguousarray(ins['w'].transpose(0, 2, 1))          # wt[j][o][m] = w[j][m][o]
    dx, _, ab = S.sconv_dgrad(dy, wt, c['pad_left'], split=S.unsplit, full=True)
    assert np.abs(dx - want_dx.numpy()).max() <= 1e-12 * max(1.0, ab.max())


def test_same_padding_is_the_tables_pad_left():
    for T in (1, 3, 37, 104, 128):
        assert conv_ref.same_pads(2 * T, 5, 2)[0] == 1 and conv_ref.same_pads(2 * T - 1, 5, 2)[0] == 2
    assert (5, 1) in S.WG_TAPS and (5, 2) in S.WG_TAPS
    assert {g[4:] for g in S.GEOMETRIES} >= {(5, 1), (5, 2)}


WG_SMALL = [c for c in S.wgrad_cases() if c['T'] <= 36]


@pytest.mark.parametrize('c', WG_SMALL, ids=_ids(WG_SMALL))
def test_weight_gradient_matches_torch_autograd(c):
    ins = S.wgrad_inputs(c, 'normal')
    sel = np.arange(0, S.WG_C, 8)
    p, q = ins['p'][:, sel], ins['q'][:, sel]
    ks = c['ks']
    w = torch.zeros(ks, len(sel), len(sel), dtype=torch.float64, requires_grad=True)
    y = _torch_conv(_t(p), w, c['pad_left'], c['T'])
    want, = torch.autograd.grad(y, w, _t(q))
    dw, tot, _, _, ab = S.wgrad_s2(p, q, S.wgrad_taps(c), c['Tp'], split=S.unsplit, full=True)
    assert np.abs(dw - want.numpy()).max() <= 1e-12 * max(1.0, ab.max())
    assert np.abs(tot - q.astype(np.float64).sum((0, 2))).max() <= 1e-12 * np.abs(q).sum((0, 2)).max()
    dw0 = ins['dw0'][:, sel][:, :, sel]
    dw2, tot2 = S.wgrad_s2(p, q, S.wgrad_taps(c), c['Tp'], split=S.unsplit, dw0=dw0, total0=np.ones(len(sel)), total_cols=(3, 9))
    assert np.array_equal(dw2, dw + dw0)
    assert np.array_equal(tot2[3:9], 1.0 + tot[3:9]) and (np.delete(tot2, np.arange(3, 9)) == 1.0).all()


SMALL = [c for c in S.table_cases() + S.split_cases()]


@pytest.mark.parametrize('c', SMALL, ids=_ids(SMALL))
def test_split_model_against_unsplit_operands(c):
    """The plane-exact evaluation differs from the unsplit one by the dropped h2 h2 term and the second plane's rounding only:
    at most 2^-21 abs_sum on standard-normal operands, nothing on integers (every low plane is zero)."""
    cs, _ = S.sliced(c, S.sconv_inputs(c, 'ints'), _msel(c))
    for kind in S.KINDS:
        _, ins = S.sliced(c, S.sconv_inputs(c, kind), _msel(c))
        a = S.reference(cs, ins, S.options('none'))
        b = S.reference(cs, ins, S.options('none'), split=S.unsplit)
        if kind == 'ints':
            assert np.array_equal(a[0], b[0])
            assert np.array_equal(a[0].astype(F32).astype(np.float64), a[0]), 'an integer case is not exact in fp32'
            assert 32 * a[-1].max() < 2 ** 24, 'partial sums of the scaled planes must stay below 2^24'
        else:
            assert (np.abs(a[0] - b[0]) <= 2.0 ** -21 * a[-1]).all()
            assert np.abs(a[0] - b[0]).max() > 0


def test_weight_gradient_split_model():
    for c in S.wgrad_cases()[:8]:
        for kind in S.KINDS:
            ins = S.wgrad_inputs(c, kind)
            sel = np.arange(0, S.WG_C, 16)
            p, q = ins['p'][:, sel], ins['q'][:, sel]
            a = S.wgrad_s2(p, q, S.wgrad_taps(c), c['Tp'], ins['sp'], ins['sq'], full=True)
            b = S.wgrad_s2(p, q, S.wgrad_taps(c), c['Tp'], ins['sp'], ins['sq'], split=S.unsplit, full=True)
            if kind == 'ints':
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
            else:
                assert (np.abs(a[0] - b[0]) <= 2.0 ** -21 * a[-1]).all()


@pytest.mark.parametrize('c', FWD, ids=_ids(FWD))
def test_forward_is_a_stride1_contraction_over_the_s2d_planes(c):
    """The header's statement of VQW_X3_S2D: tap j with e = j - pad_left reads chunk block e & 1 at row offset e >> 1 of
    x3_ref.act_planes(x, mode = X3_S2D).  Decoded back to float64 those are the operands of sconv_fwd, bit for bit."""
    for kind in S.KINDS:
        ins = S.sconv_inputs(c, kind)
        planes = X.act_planes(ins['x'], ins['sx'], mode=X.X3_S2D)
        ops = S.fwd_operands_s2d(planes, c['B'], c['Cin'], c['T'], c['ks'], c['pad_left'])
        o = S.options('all')
        _, ins_s = S.sliced(c, ins, _msel(c))
        want = S.reference(c, ins_s, o)
        got = S.sconv_fwd(ins_s['x'], ins_s['w'], ins_s['bias'], ins_s['bn_scale'], ins_s['bn_shift'], True, c['pad_left'], ins['sx'], ins['sw'],
                          operands=ops, full=True)
        for g, w_ in zip(got, want):
            assert np.array_equal(g, w_)


def test_every_case_is_legal_and_every_refusal_is_not():
    for cus in CUS:
        for c in S.all_sconv_cases(cus):
            assert S.legality(c) is None, c['name']
            assert c['Cin'] <= S.MAX_CIN and c['M'] <= S.MAX_M
    for c in S.table_cases() + S.split_cases() + S.ignored_split_cases():
        assert c['B'] * c['T'] <= S.MAX_COLS, c['name']
    for name, c in S.refusal_cases():
        assert S.legality(c) is not None, name
    assert {g for g in S.GEOMETRIES} == {(c['B'], c['T'], c['Cin'], c['M'], c['ks'], c['pad_left']) for c in FWD}
    for c in S.wgrad_cases():
        assert c['T'] % 4 == 0 and S.WG_LDDW % 4 == 0 and S.WG_LDDW > S.WG_C


@pytest.mark.parametrize('cus', CUS)
def test_path_reaches_every_outcome(cus):
    """path(case, cus): every automatic case lands where it was built to land; block shapes 2..5 are each reached by an
    automatic case (shape 1 is never chosen: the launcher's rule has no branch that ends there -- forced cases alone run it);
    one round, two rounds and unsplit are each reached with ksplit = 0; every explicit split count fits; an explicit ksplit on a
    forced shape 1, 3, 4 or 5 runs unsplit."""
    auto = S.auto_cases(cus)
    for c in auto:
        assert S.path(c, cus) == c['expect'], (c['name'], S.path(c, cus))
    assert {S.path(c, cus)['shape'] for c in auto if not c['slab']} == {2, 3, 4, 5}
    assert {S.path(c, cus)['rounds'] for c in auto if c['slab']} == {0, 1, 2}
    for c in S.split_cases():
        assert S.fits(c, c['ksplit']) and S.path(c, cus)['S'] == c['ksplit'], c['name']
    for c in S.ignored_split_cases():
        assert S.path(c, cus) == dict(shape=c['shape'], S=1, rounds=0)
    boundary = [c for c in S.split_cases() if min(S.steps(c)) // c['ksplit'] == 8]
    assert any(not c['dgrad'] for c in boundary) and any(c['dgrad'] for c in boundary)
    for g in S.GEOMETRIES:
        for sh in S.shapes_for(g[3]):
            assert S.legality(dict(B=g[0], T=g[1], Cin=g[2], M=g[3], ks=g[4], pad_left=g[5], dgrad=False, shape=sh)) is None
    assert {sh for g in S.GEOMETRIES for sh in S.shapes_for(g[3])} == {0, 1, 2, 3, 4, 5}


# ---------------------------------------------------------------------------------------------------- the bars
def _emu_cases():
    return S.table_cases() + S.split_cases() + S.ignored_split_cases() + S.auto_cases(256)


@pytest.mark.parametrize('c', _emu_cases(), ids=_ids(_emu_cases()))
def test_fp32_emulation_stays_under_the_bars(c):
    """Condition on the inputs and the formula: the same sum step by step in fp32 (split launches: partial sums first, then added
    in split order) stays under EMU_FRACTION of every elementwise bar."""
    msel = _msel(c, c['M'] if c['B'] * c['T'] <= 100 else EMU_ROWS)          # (every output channel of the smallest geometries)
    cs, ins = S.sliced(c, S.sconv_inputs(c, 'normal'), msel)
    nsplit = S.path(c, 256)['S']
    if c['B'] * c['T'] > S.MAX_COLS:          # (the cases sized from the CU count: three batch rows -- each is a problem of its own)
        cs, ins = dict(cs, B=3), dict(ins, x=ins['x'][[0, c['B'] // 2, c['B'] - 1]])
    y = S.emulate_sconv(cs, ins, None, S=nsplit)
    if c['dgrad']:
        dx, bar, _ = S.reference(cs, ins)
        assert (bar >= 0).all()          # (zero where no tap reaches the element: pad_left = ks - 1 leaves u = 2T - 1 empty)
        assert (np.abs(y.astype(np.float64) - dx) <= S.EMU_FRACTION * bar).all(), np.max(np.abs(y - dx) / bar)
        return
    for o in S.OPTION_SETS:
        opts = S.options(o[0])
        out, r, bar, bar_r, _ = S.reference(cs, ins, opts)
        e_out, e_r = S.emulate_epilogue(y, ins, opts, np.arange(len(msel)))
        assert (np.abs(e_out.astype(np.float64) - out) <= S.EMU_FRACTION * bar).all(), (o[0], np.max(np.abs(e_out - out) / bar))
        assert (np.abs(e_r.astype(np.float64) - r) <= S.EMU_FRACTION * bar_r).all(), (o[0], np.max(np.abs(e_r - r) / bar_r))
        if opts['relu']:
            assert 0.2 < (r > 0).mean() < 0.8, 'the relu should cut about half'


@pytest.mark.parametrize('c', S.wgrad_cases(), ids=_ids(S.wgrad_cases()))
def test_weight_gradient_emulation_stays_under_the_bar(c):
    ins = S.wgrad_inputs(c, 'normal')
    rng = np.random.default_rng(S.seed_of('wsel', c['name']))
    nsel = S.WG_C if c['B'] * c['T'] <= 108 else 48          # every element where the sums are short and the bars smallest
    csel, osel = np.sort(rng.choice(S.WG_C, nsel, replace=False)), np.sort(rng.choice(S.WG_C, nsel, replace=False))
    got = S.emulate_wgrad(c, ins, csel, osel)
    sub = dict(ins, p=ins['p'][:, csel], q=ins['q'][:, osel], dw0=ins['dw0'][:, csel][:, :, osel])
    dw, tot, bar, bar_t, _ = S.wgrad_s2(sub['p'], sub['q'], S.wgrad_taps(c), c['Tp'], ins['sp'], ins['sq'], dw0=sub['dw0'],
                                        total0=ins['total0'][osel], full=True)
    assert (np.abs(got.astype(np.float64) - dw) <= S.EMU_FRACTION * bar).all(), np.max(np.abs(got - dw) / bar)
    # q_total: the fp32 values summed one at a time onto the pre-filled value
    acc = ins['total0'][osel].copy()
    for b in range(c['B']):
        for t in range(c['T']):
            acc = (acc + sub['q'][b, :, t]).astype(F32)
    assert (np.abs(acc.astype(np.float64) - tot) <= S.EMU_FRACTION * bar_t).all()


# ---------------------------------------------------------------------------------------------------- detection power
def _find(cases, **kw):
    return next(c for c in cases if all(c[k] == v for k, v in kw.items()))


def _without(c, tap=None, chunk=None):
    m = S.kmask_all(c['ks'], c['Cin'])
    if tap is not None:
        m[tap] = False
    if chunk is not None:
        m[:, 16 * chunk:][:, :16] = False
    return m


def _told_apart(right, wrong, bar, kind):
    """More than 4 bars somewhere on a standard-normal case, any bit on an integer case."""
    if kind == 'ints':
        return not np.array_equal(np.asarray(right, F32), np.asarray(wrong, F32))
    return bool((np.abs(right - wrong) > 4 * bar).any())


def _sconv_detects(wrong, cases, opts_name='all', out_index=0, kmask_of=None):
    hits = 0
    for c in cases:
        for kind in S.KINDS:
            cs, ins = S.sliced(c, S.sconv_inputs(c, kind), _msel(c))
            opts = S.options(opts_name)
            good = S.reference(cs, ins, opts)
            if kmask_of is not None:
                bad = S.reference(cs, ins, opts, kmask=kmask_of(cs))
            else:
                bad = S.reference(cs, ins, opts, wrong=wrong)
            bar = good[1] if c['dgrad'] else good[2 + out_index]
            hits += _told_apart(good[out_index], bad[out_index], bar, kind)
    return hits


def test_wrong_references_are_told_apart():
    table, split = S.table_cases(), S.split_cases()
    fwd_small = [_find(table, B=5, T=3, dgrad=False), _find(table, B=2, T=40, ks=8, pad_left=3, dgrad=False), _find(table, B=1, T=257, dgrad=False)]
    dg_small = [_find(table, B=5, T=3, dgrad=True), _find(table, B=2, T=40, ks=8, pad_left=3, dgrad=True), _find(table, B=1, T=257, dgrad=True)]
    both = fwd_small + dg_small
    seen = {}
    seen['pad_plus_one'] = _sconv_detects('pad_plus_one', both)
    seen['parity_swap'] = _sconv_detects('parity_swap', dg_small)
    seen['leak'] = _sconv_detects('leak', [both[0], both[1], both[3], both[4]])
    seen['drop_last_tap'] = _sconv_detects(None, both, kmask_of=lambda c: _without(c, tap=c['ks'] - 1))
    seen['drop_last_chunk'] = _sconv_detects(None, both, kmask_of=lambda c: _without(c, chunk=c['Cin'] // 16 - 1))
    seen['drop_last_col'] = _sconv_detects('drop_last_col', both)
    sp = [split[0], _find(split, dgrad=True, pad_left=2)]
    seen['drop_split'] = _sconv_detects(None, sp, kmask_of=lambda c: ~S.split_kmask(c, c['ksplit'], c['ksplit'] - 1))
    seen['bias_after_relu'] = _sconv_detects('bias_after_relu', fwd_small)
    seen['bn_on_save_r'] = _sconv_detects('bn_on_save_r', fwd_small, out_index=1)
    seen['relu_forced'] = _sconv_detects('relu_forced', fwd_small, opts_name='bias')
    seen['no_h2h1'] = 0
    for name in ('wgrad_no_zero_behind_tp', 'dw_overwritten', 'no_h2h1'):
        hits = 0
        for c in [w for w in S.wgrad_cases() if w['T'] <= 36 and w['Tp'] == 2 * w['T'] - 1]:
            for kind in S.KINDS:
                ins = S.wgrad_inputs(c, kind)
                sel = np.arange(0, S.WG_C, 8)
                args = (ins['p'][:, sel], ins['q'][:, sel], S.wgrad_taps(c), c['Tp'], ins['sp'], ins['sq'])
                dw0 = ins['dw0'][:, sel][:, :, sel]
                good = S.wgrad_s2(*args, dw0=dw0, full=True)
                bad = S.wgrad_s2(*args, dw0=dw0, wrong=name, full=True)
                hits += _told_apart(good[0], bad[0], good[2], kind)
        seen[name] = seen.get(name, 0) + hits
    assert set(seen) == set(S.WRONG) and len(seen) >= 12
    assert all(v > 0 for v in seen.values()), seen
    # the format's own mutation shows only where low planes exist: never on an integer case
    c = S.wgrad_cases()[0]
    ins = S.wgrad_inputs(c, 'ints')
    a = S.wgrad_s2(ins['p'][:, :16], ins['q'][:, :16], S.wgrad_taps(c), c['Tp'], ins['sp'], ins['sq'])
    b = S.wgrad_s2(ins['p'][:, :16], ins['q'][:, :16], S.wgrad_taps(c), c['Tp'], ins['sp'], ins['sq'], wrong='no_h2h1')
    assert np.array_equal(a[0], b[0])
