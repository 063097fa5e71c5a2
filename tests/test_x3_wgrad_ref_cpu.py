"""tests/x3_wgrad_ref.py on the CPU: wgrad() against torch float64 (einsum over the unsplit operands, autograd of conv1d) and against
sconv_ref.wgrad_s2 on a case both can state, the bars against sequential fp32 emulations in two orders, path() and legality() on
hand-written rows, and the power to tell every deliberately wrong evaluation from the right one."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sconv_ref as S  # noqa: E402
import x3_wgrad_ref as R  # noqa: E402
import x3_ref as X  # noqa: E402

CASES = R.all_cases()
BY_NAME = {c['name']: c for c in CASES}


def _shift64(x, sh):
    T = x.shape[2]
    out = torch.zeros_like(x)
    if -T < sh < T:
        if sh >= 0:
            out[:, :, :T - sh] = x[:, :, sh:]
        else:
            out[:, :, -sh:] = x[:, :, :T + sh]
    return out


def _unsplit_planes(monkeypatch):
    """wgrad() over the operands themselves: the first plane is the fp32 value, there is no second one."""
    monkeypatch.setattr(R, 'pieces', lambda x, s, bf16: S.unsplit(X.scaled(x, s)))


def test_table_is_well_formed():
    names = [c['name'] for c in CASES]
    assert len(set(names)) == len(names)
    for c in CASES:
        assert R.legality(c) is None, '%s: %s' % (c['name'], R.legality(c))
        assert c['B'] <= 3 and c['T'] in (32, 64, 96, 192, 40, 72) and c['Cp'] in (256, 512) and c['Q0'] in (256, 512) and c['Q1'] in (0, 256)
        assert c['T'] % 32 == 0 or c['form'] == 'pq'
        assert c['T'] <= 96 or c['family'] == 'splits'
    for name, c, _ in R.refusal_cases():
        assert R.legality(c) is not None, name + ' is legal per legality()'
    seen = {R.instantiation(R.path(c, 256)) for c in CASES}
    assert seen == set(R.stride1_instantiations()) and len(seen) == 12


@pytest.mark.parametrize('name', ['rowcol/Q0-512-Q1-ff', 'taps/pq-positive', 'taps/ff-T64-padding', 'relu/ff-unaligned-f16x3'])
def test_wgrad_is_the_float64_einsum_of_the_unsplit_operands(monkeypatch, name):
    _unsplit_planes(monkeypatch)
    c = BY_NAME[name]
    ins = R.inputs(c, 'normal')
    dw, _, _, _, _, _, ab = R.reference(c, ins)
    p = torch.from_numpy(ins['p']).double()
    p = p.clamp(min=0) if c['p_relu'] else p
    q = torch.from_numpy(np.concatenate([ins['q0']] + ([ins['q1']] if c['Q1'] else []), axis=1)).double()
    want = torch.stack([torch.einsum('bct,bot->co', _shift64(p, sh), q) for sh in c['taps']]) + torch.from_numpy(ins['dw0']).double()
    assert np.abs(dw - want.numpy()).max() <= 1e-12 * max(1.0, ab.max())


def test_wgrad_is_the_autograd_of_a_float64_conv1d():
    """Exact images (ints): dw of a causal conv with taps t - (ks - 1 - j) d is the gradient of its kernel, at 1e-12."""
    import torch.nn.functional as Fn
    ks, d = 3, 2
    c = R._case('pin/autograd', taps=tuple(-(ks - 1 - j) * d for j in range(ks)), B=3, Q1=256)
    ins = R.inputs(c, 'ints')
    dw, _, _ = R.wgrad(ins['p'], ins['q0'], ins['q1'], c['taps'], ins['sp'], ins['sq0'], ins['sq1'])
    x = torch.from_numpy(ins['p']).double()
    w = torch.zeros(c['Q0'] + c['Q1'], c['Cp'], ks, dtype=torch.float64, requires_grad=True)
    y = Fn.conv1d(Fn.pad(x, ((ks - 1) * d, 0)), w, dilation=d)
    dy = torch.from_numpy(np.concatenate([ins['q0'], ins['q1']], axis=1)).double()
    g, = torch.autograd.grad(y, w, dy)
    assert np.abs(dw - g.permute(2, 1, 0).numpy()).max() <= 1e-12
    for mode in (0, 1):     # the planes are exact images: the same under both modes
        assert np.array_equal(R.wgrad(ins['p'], ins['q0'], ins['q1'], c['taps'], ins['sp'], ins['sq0'], ins['sq1'], mode=mode)[0], dw)


@pytest.mark.parametrize('kind', R.KINDS)
def test_wgrad_agrees_with_the_stride2_reference_on_a_shared_case(kind):
    """wgrad_s2 reads p at 2 t + tap: over a p whose odd samples are another tensor, its even taps are this module's taps / 2."""
    c = R._case('pin/s2', taps=(-2, -1, 0), B=3, T=32, total=True, total_cols=(64, 200))
    ins = R.inputs(c, kind)
    rng = np.random.default_rng(5)
    p2 = rng.standard_normal((c['B'], c['Cp'], 2 * c['T'])).astype(np.float32)
    p2[:, :, 0::2] = ins['p']
    a = R.wgrad(ins['p'], ins['q0'], None, c['taps'], ins['sp'], ins['sq0'], dw0=ins['dw0'], total=True, total0=ins['total0'], total_cols=(64, 200), full=True)
    b = S.wgrad_s2(p2, ins['q0'], [2 * sh for sh in c['taps']], 2 * c['T'], ins['sp'], ins['sq0'], dw0=ins['dw0'], total0=ins['total0'],
                   total_cols=(64, 200), full=True)
    assert np.abs(a[0] - b[0]).max() <= 1e-12 * max(1.0, np.abs(b[0]).max()) and np.array_equal(a[1], b[1])
    assert np.allclose(a[6], b[4], rtol=1e-12, atol=0) and np.array_equal(a[4], b[3])
    P = np.abs(a[0] - ins['dw0']) + 3 * c['B'] * c['T'] * R.U * a[6]
    assert np.allclose(a[3], b[2] + R.U * P, rtol=1e-9, atol=0)                                  # the same bar but for the reduce kernel's one add


def test_planes_images_decode_to_the_pieces():
    """The uint16 images the device gets hold exactly the values wgrad() multiplies, chunk offsets and host factors included."""
    for name in ('wide/both-kc0-pq-bf16', 'wide/hscale-pq', 'wide/tap-chunk-kc0-pf'):
        c = BY_NAME[name]
        ins = R.inputs(c, 'normal')
        pp, qp = R.plane_images(c, ins)
        B, T, bf = c['B'], c['T'], bool(c['mode'] & 1)
        for img, x, s, KC in ((pp, ins['p'], ins['sp'] * c['p_hscale'], c['p_KC']), (qp, ins['q0'], ins['sq0'] * c['q_hscale'], c['q_KC'])):
            if img is None:
                continue
            assert img.shape == (1 if bf else 2, KC or x.shape[1] // 8, B * T, 8)
            h = R.pieces(x, s, bf)
            for k in range(img.shape[0]):
                val = (img[k].astype(np.uint32) << 16).view(np.float32) if bf else img[k].view(np.float16)
                val = val.astype(np.float64).transpose(1, 0, 2).reshape(B, T, -1).transpose(0, 2, 1)
                assert np.array_equal(val, h[k]), name


WORST = {}


def _emu_nsplit(c):
    return R.path(c, 256)['nsplit']


@pytest.mark.parametrize('c', CASES, ids=[c['name'] for c in CASES])
def test_bars_hold_the_fp32_emulations(c):
    """Both orders of the sequential fp32 emulation stay under EMU_FRACTION of every bar ('normal') and are exact ('ints'), on a
    sample of rows and columns that has the edges of every tile."""
    cs, os_ = R.sample_rows(c)
    cs, os_ = cs[::2], os_[::2]
    ns = _emu_nsplit(c)
    for i in range(min(c['n'], 2)):
        for kind in R.KINDS:
            ins = R.inputs(c, kind, i)
            dw, tot, seg, bar, bar_t, bar_s, _ = R.reference(c, ins, i, csel=cs, osel=os_)
            for order in ('time', 'split') if ns > 1 else ('time',):
                e_dw, e_tot, e_seg = R.emulate(c, ins, cs, os_, order, ns, i)
                for got, want, b, what in ((e_dw, dw, bar, 'dw'), (e_tot, tot, bar_t, 'q_total'), (e_seg, seg, bar_s, 'q_seg')):
                    if want is None:
                        assert got is None
                        continue
                    err = np.abs(got.astype(np.float64) - want)
                    if kind == 'ints':
                        assert not err.any(), '%s %s %s: the integer case is not exact' % (c['name'], order, what)
                    else:
                        live = b > 0
                        assert not err[~live].any()
                        worst = float((err[live] / b[live]).max()) if live.any() else 0.0
                        WORST[what] = max(WORST.get(what, 0.0), worst)
                        assert worst <= R.EMU_FRACTION, '%s %s %s: the emulation uses %.3f of its bar' % (c['name'], order, what, worst)


def test_print_the_worst_emulation_fractions():
    print('emulation / bar, worst over the table: %s' % WORST)


def test_path_on_hand_written_rows():
    row = lambda **kw: R.path(R._case('pin/path', **kw), 256)  # noqa: E731
    inst = lambda **kw: R.instantiation(row(**kw))  # noqa: E731
    assert inst(form='ff', taps=(-8, -4, 0)) == ('reg', False, False, False, False, False)
    assert inst(form='ff', taps=(-8, -3, 0), mode=1) == ('reg', True, True, False, False, False)
    assert inst(form='fq', taps=(-2, 0)) == ('reg', True, False, False, True, False)
    assert inst(form='pf', taps=(-2, 1), mode=1) == ('reg', False, True, False, False, True)
    assert inst(form='pq', taps=(-1, 0)) == ('dma', False, False, False, True, True)
    assert inst(form='ff', taps=(0,), p_stride=2) == ('reg', False, False, True, False, False)
    assert inst(form='ff', n=2, taps=((-4, 0), (-4, -1))) == ('reg', True, False, False, False, False)      # one unaligned shift in any problem
    # tiles = n * taps * Cp / 256 * (Q0 + Q1) / 256; nsplit = CUs / tiles, clamped to [1, B * ceil(T / 32)]
    r = R.path(R._case('pin/a', taps=tuple(range(-7, 1)), Cp=512, Q0=512, Q1=256, B=2, T=96, nsplit=0), 256)
    assert (r['tiles'], r['nsplit']) == (48, 5)
    assert R.path(R._case('pin/b', taps=tuple(range(-7, 1)), Cp=512, Q0=512, Q1=256, B=2, T=96, nsplit=0), 304)['nsplit'] == 6
    assert R.path(R._case('pin/c', taps=tuple(range(-7, 1)), Cp=512, Q0=512, Q1=256, B=2, T=96, nsplit=0), 40)['nsplit'] == 1
    assert R.path(R._case('pin/d', taps=(0,), nsplit=0), 256)['nsplit'] == 4                                  # 256 / 1, clamped to 2 * 2 pairs
    assert R.path(R._case('pin/e', form='pq', T=72, B=1, nsplit=5), 256)['nsplit'] == 3                        # ceil(72 / 32) pairs
    assert R.path(R._case('pin/f', n=5, taps=tuple((0, -1, -2) for _ in range(5)), nsplit=0, B=3, T=192), 256) == dict(
        kernel='reg', odd=True, bf=False, s2=False, qp=False, pp=False, nsplit=17, tiles=15)
    assert [R.split_range(3, 64, 4, k) for k in range(4)] == [(0, 1), (1, 3), (3, 4), (4, 6)]
    assert R.step_mask(2, 40, 1, 3).sum(1).tolist() == [8, 32]


# the cases each deliberately wrong evaluation is looked for on (at least one must tell it apart)
LOOK = {'shift_plus_one': ('forms/ff-unaligned-f16x3', 'forms/pq-aligned-bf16'), 'drop_last_tap': ('taps/ff-eight', 'forms/pq-unaligned-f16x3'),
        'drop_last_pair': ('forms/fq-unaligned-f16x3', 'taps/pq-ragged-T40'), 'drop_last_split': ('splits/17-ff', 'splits/4-pf'),
        'leak_before_t0': ('taps/ff-unaligned4', 'taps/pq-T64-far'), 'ragged_tail_read': ('taps/pq-ragged-T40', 'taps/pq-ragged-T72'),
        'window_not_moved': ('taps/ff-unaligned4', 'taps/fq-unaligned4-bf16'), 'no_h2h1': ('forms/ff-aligned-f16x3', 'forms/pq-aligned-f16x3'),
        'dw_overwritten': ('forms/ff-aligned-f16x3', 'taps/pq-T64-padding'), 'q1_scale_from_q0': ('rowcol/Q1-ff', 'rowcol/Q0-512-Q1-ff'),
        'row_tile_reads_first': ('rowcol/Cp512-ff', 'rowcol/Cp512-pq'), 'no_relu': ('relu/ff-aligned-f16x3', 'relu/fq-unaligned-bf16'),
        'relu_after_split': ('relu/ff-aligned-f16x3', 'relu/fq-aligned-f16x3'), 'total_all_cols': ('sums/total-inside-a-tile', 'sums/total-q1-only'),
        'seg_from_rounded': ('sums/fp32-q-bf16', 'sums/fp32-q-bf16-pf'), 'p_kc0_ignored': ('wide/p-kc0-pq', 'wide/p-kc0-pf-bf16'),
        'p_tap_chunk_ignored': ('wide/tap-chunk-pq', 'wide/tap-chunk-kc0-pf'), 'q_hscale_ignored': ('wide/hscale-pq', 'wide/q-hscale-fq-bf16')}


def departs(c, kind, wrong, full_tiles=False):
    """How a wrong evaluation departs from the right one on a case: 'bit' (an 'ints' element differs), a number of bars ('normal',
    the largest over dw, q_total and q_seg), or None."""
    cs, os_ = (None, None) if full_tiles else R.sample_rows(c)
    ins = R.inputs(c, kind)
    right = R.reference(c, ins, csel=cs, osel=os_)
    bad = R.reference(c, ins, wrong=wrong, csel=cs, osel=os_)
    worst = 0.0
    for k in range(3):
        if right[k] is None:
            continue
        d = np.abs(bad[k] - right[k])
        if kind == 'ints':
            if d.any():
                return 'bit'
        else:
            b = right[3 + k]
            worst = max(worst, float((d[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0, np.inf if d[b == 0].any() else 0.0)
    return worst if kind == 'normal' and worst > 0 else None


@pytest.mark.parametrize('wrong', R.WRONG)
def test_every_wrong_evaluation_is_told_apart(wrong):
    assert set(LOOK) == set(R.WRONG)
    found = {}
    for name in LOOK[wrong]:
        for kind in R.KINDS:
            found[(name, kind)] = departs(BY_NAME[name], kind, wrong)
    caught = [k for k, v in found.items() if v == 'bit' or (v is not None and v != 'bit' and v > 4.0)]
    assert caught, '%s is not told apart on any of %s' % (wrong, found)
    print('%s: %s' % (wrong, found))


def test_the_low_planes_matter_only_off_the_integers():
    """The two evaluations that differ in a low plane only (no h2 h1, relu after the split) are invisible to integer operands and
    several bars on the standard-normal ones at B * T = 32: the reason both kinds run on every case."""
    for wrong, name in (('no_h2h1', 'forms/ff-aligned-f16x3'), ('relu_after_split', 'relu/ff-aligned-f16x3')):
        assert departs(BY_NAME[name], 'ints', wrong) is None
        assert departs(BY_NAME[name], 'normal', wrong) > 4.0
