"""vqw_f16x3_strided_conv (forward, input gradient, split-K) and the stride-2 forms of vqw_f16x3_wgrad against the plane-exact
float64 reference of tests/sconv_ref.py, through kernels.py (f16x3_split_activations, f16x3_pack_weights, f16x3_strided_conv,
f16x3_wgrad), at the smallest shapes that reach every tap parity, batch edge, partial tile, block shape and split outcome.

Every output -- out, save_r, dx, dw with its wider lddw row, q_total -- is a view into a sentinel-filled buffer; the split slab is
NaN-filled and sized exactly, inside a longer sentinel buffer; the ticket counters are zero for `tiles` ints with sentinels
behind them.  Whatever a launch does not own must keep its bits, counters must be zero after every launch.  Integer cases must
equal the reference bit for bit (save_r included), standard-normal cases stay within the elementwise bars of sconv_ref, and a
refusal must raise, launch nothing and leave its outputs' bits alone.  (p_stride = 2 in bf16 mode is refused too:
test_bf16_kernels_gpu.py::test_wgrad_bf16_refuses_stride_2.)

Which block shape an automatic launch took cannot be seen from outside; path(case, cus) is asserted against the device's CU
count for every automatic case, and the split count it names is checked against what the launch wrote into the slab.

Every test records err / bar of its case (record_property 'err_over_bar_<family>'); DESIGN 6 lists the maxima."""
import copy
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sconv_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F32 = np.float32
G = S.GUARD
ISENT = -77


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ids(cases):
    return [c['name'] for c in cases]


def _cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def _bits(t):
    return t.view(torch.int32)


class Guarded:
    """n floats between two guard bands of sentinels; `view` is what the kernel gets.  init: the view's contents (default sentinels)."""

    def __init__(self, n, init=None, fill=float(S.SENTINEL), tail=G):
        self.n = n
        self.full = torch.full((G + n + tail,), float(S.SENTINEL), device=DEV)
        self.view = self.full[G:G + n]
        if init is not None:
            self.view.copy_(_dev(np.asarray(init, F32).reshape(-1)))
        elif fill != float(S.SENTINEL):
            self.view.fill_(fill)
        self.before = self.full.clone()

    def guards_ok(self, what):
        assert torch.equal(_bits(self.full[:G]), _bits(self.before[:G])) and torch.equal(_bits(self.full[G + self.n:]), _bits(self.before[G + self.n:])), \
            what + ': a guard band changed'

    def untouched(self, what):
        assert torch.equal(_bits(self.full), _bits(self.before)), what + ': changed'

    def host(self, shape):
        return self.view.cpu().numpy().reshape(shape)


class Scratch:
    """The split slab (NaN, exactly `floats` long, sentinels behind it) and the ticket counters (zero for `tiles` ints, sentinels behind)."""

    def __init__(self, floats, tiles, tail=4096):
        self.slab = Guarded(floats, fill=float('nan'), tail=tail)
        self.cfull = torch.full((tiles + 64,), ISENT, dtype=torch.int32, device=DEV)
        self.cfull[:tiles] = 0
        self.counters = self.cfull[:tiles]
        self.tiles = tiles

    def share(self, tiles):
        """The same scratch with a counters view of `tiles` ints (split_counters_n == tiles of the launch that gets it)."""
        s = copy.copy(self)
        s.counters = self.cfull[:tiles]
        return s

    def check(self, what, written=None):
        self.slab.guards_ok(what + ' slab')
        assert int(self.cfull[:self.tiles].abs().sum()) == 0, what + ': ticket counters not back at zero'
        assert bool((self.cfull[self.tiles:] == ISENT).all()), what + ': ints behind the ticket counters changed'
        if written is not None:
            n = int((~torch.isnan(self.slab.view)).sum())
            assert n == written, '%s: %d floats of the slab written, %d expected' % (what, n, written)


def _compare(got, want, bar, kind, what):
    """err / bar (0 for a bit-exact kind).  A written zero is compared by value."""
    got64 = got.astype(np.float64)
    if kind == 'ints':
        bad = np.flatnonzero(got64.reshape(-1) != want.reshape(-1))
        assert bad.size == 0, '%s: %d of %d elements differ from the exact result (first: %s got %r want %r)' % (
            what, bad.size, got.size, np.unravel_index(bad[0], got.shape), got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]])
        return 0.0
    assert np.isfinite(got64).all(), what + ': not finite'
    err = np.abs(got64 - want)
    over = err > bar
    if over.any():
        i = np.unravel_index(np.argmax(np.where(bar > 0, err / np.where(bar > 0, bar, 1), np.where(err > 0, np.inf, 0))), err.shape)
        raise AssertionError('%s: %d of %d elements over the bar; worst at %s: got %r want %r err %.3e bar %.3e' % (
            what, int(over.sum()), err.size, i, got[i], want[i], err[i], bar[i]))
    live = bar > 0
    return float((err[live] / bar[live]).max()) if live.any() else 0.0


@functools.lru_cache(maxsize=4)
def _inputs(key, kind):
    c = dict(zip(('B', 'T', 'Cin', 'M', 'ks', 'pad_left', 'dgrad'), key))
    return S.sconv_inputs(c, kind)


@functools.lru_cache(maxsize=2)
def _contraction(key, kind):
    """The float64 contraction of a geometry, shared by every block shape, option set and split count that runs on it."""
    c = dict(zip(('B', 'T', 'Cin', 'M', 'ks', 'pad_left', 'dgrad'), key))
    ins = _inputs(key, kind)
    if c['dgrad']:
        return S.sconv_dgrad(ins['x'], ins['w'], c['pad_left'], ins['sx'], ins['sw'], full=True)
    return S.fwd_pre(ins['x'], ins['w'], c['pad_left'], ins['sx'], ins['sw'])


def _key(c):
    return (c['B'], c['T'], c['Cin'], c['M'], c['ks'], c['pad_left'], c['dgrad'])


class Operands:
    """The device operands of a case in one scale mode: 'dev' = scales in device slots, w_scale_inv = 1; 'host' = host-side plane
    scales, NULL slots and w_scale_inv = 1 / (sx sw)."""

    def __init__(self, K, c, ins, mode):
        B, T, Cin, M, ks = c['B'], c['T'], c['Cin'], c['M'], c['ks']
        L = T if c['dgrad'] else 2 * T
        self.sc = torch.tensor([ins['sx'], ins['sw']], device=DEV)
        dev = mode == 'dev'
        self.xp = torch.empty(2 * B * Cin * L, dtype=torch.float16, device=DEV)
        self.wp = torch.empty(2 * ks * Cin * M, dtype=torch.float16, device=DEV)
        K.f16x3_split_activations(_dev(ins['x']), self.xp, B, Cin, L, scale=1.0 if dev else ins['sx'], scale_dev=self.sc[0:1] if dev else None,
                                  mode=0 if c['dgrad'] else K.X3_S2D)
        K.f16x3_pack_weights(_dev(ins['w']), self.wp, ks * Cin, M, M, 1.0 if dev else ins['sw'], scale_dev=self.sc[1:2] if dev else None, mode=0)
        self.kw = dict(xp=self.xp, wp=self.wp, B=B, T=T, Cin=Cin, M=M, ks=ks, pad_left=c['pad_left'], dgrad=c['dgrad'],
                       x_scale=self.sc[0:1] if dev else None, w_scale=self.sc[1:2] if dev else None,
                       w_scale_inv=1.0 if dev else 1.0 / (ins['sx'] * ins['sw']))
        self.dev = {k: _dev(ins[k]) for k in ('bias', 'bn_scale', 'bn_shift')}


def _launch(K, c, ops, opts, kind, what, shape=0, scratch=None, ksplit=0, written=None):
    """One launch into fresh guarded outputs, held to the reference.  Returns (outputs as host arrays, {family: err / bar})."""
    B, T, M = c['B'], c['T'], c['M']
    ins = _inputs(_key(c), kind)
    n_out = B * M * T * (2 if c['dgrad'] else 1)
    out = Guarded(n_out)
    save = Guarded(n_out) if (not c['dgrad'] and opts['save_r']) else None
    kw = dict(ops.kw, out=out.view, shape=shape)
    if not c['dgrad']:
        kw.update(bias=ops.dev['bias'] if opts['bias'] else None, bn_scale=ops.dev['bn_scale'] if opts['bn'] else None,
                  bn_shift=ops.dev['bn_shift'] if opts['bn'] else None, relu=opts['relu'], save_r=save.view if save else None)
    if scratch is not None:
        kw.update(split_slab=scratch.slab.view, split_counters=scratch.counters, ksplit=ksplit)
    K.f16x3_strided_conv(**kw)
    torch.cuda.synchronize()
    out.guards_ok(what + ' out')
    if scratch is not None:
        scratch.check(what, written)
    ratios = {}
    if c['dgrad']:
        dx, bar, _ = _contraction(_key(c), kind)
        got = out.host((B, M, 2 * T))
        ratios['dgrad'] = _compare(got, dx, bar, kind, what + ' dx')
        return (got,), ratios
    pre, ab = _contraction(_key(c), kind)
    want, want_r, bar, bar_r = S.fwd_epilogue(pre, ab, 3 * c['ks'] * c['Cin'], ins['bias'] if opts['bias'] else None,
                                              ins['bn_scale'] if opts['bn'] else None, ins['bn_shift'] if opts['bn'] else None, opts['relu'])
    got = out.host((B, M, T))
    ratios['forward'] = _compare(got, want, bar, kind, what + ' out')
    res = (got,)
    if save:
        save.guards_ok(what + ' save_r')
        got_r = save.host((B, M, T))
        ratios['save_r'] = _compare(got_r, want_r, bar_r, kind, what + ' save_r')
        res = (got, got_r)
    return res, ratios


def _record(record_property, ratios, prefix=''):
    for fam, r in ratios.items():
        record_property('err_over_bar_' + prefix + fam, r)


def _merge(total, ratios):
    for k, v in ratios.items():
        total[k] = max(total.get(k, 0.0), v)


# ---------------------------------------------------------------------------------------------------- the geometry table
TABLE = S.table_cases()


def _option_names(c, si, shape):
    """All five option sets on shape 0 and on the shapes few geometries allow (3, 4); one of them, rotating, on shapes 1, 2, 5."""
    if c['dgrad']:
        return ['none']
    if shape in (0, 3, 4):
        return [o[0] for o in S.OPTION_SETS]
    return [S.OPTION_SETS[(si + c['ks'] + c['pad_left']) % 5][0]]


@pytest.mark.parametrize('c', TABLE, ids=_ids(TABLE))
def test_table_geometry_on_every_block_shape(K, record_property, c):
    """Shape 0 and every forced shape the header allows for M, on both kinds of operands and in both scale modes; the forward pass
    with all five option sets on shape 0 and one of them, rotating, on every forced shape."""
    total, launches = {}, 0
    assert S.path(dict(c, shape=0), _cus())['S'] == 1
    for kind in S.KINDS:
        ins = _inputs(_key(c), kind)
        ops = {m: Operands(K, c, ins, m) for m in S.SCALE_MODES}
        for si, shape in enumerate(S.shapes_for(c['M'])):
            assert S.legality(dict(c, shape=shape)) is None
            names = _option_names(c, si, shape)
            for oi, name in enumerate(names):
                mode = S.SCALE_MODES[(si + oi) % 2]
                what = '%s %s shape %d options %s scales %s' % (c['name'], kind, shape, name, mode)
                _, ratios = _launch(K, c, ops[mode], S.options(name), kind, what, shape=shape)
                _merge(total, ratios)
                launches += 1
    _record(record_property, total)
    record_property('launches', launches)


def test_every_option_set_meets_every_forced_shape():
    seen = {(sh, name) for c in TABLE if not c['dgrad'] for si, sh in enumerate(S.shapes_for(c['M'])) if sh for name in _option_names(c, si, sh)}
    assert seen == {(sh, o[0]) for sh in (1, 2, 3, 4, 5) for o in S.OPTION_SETS}, sorted(seen)


# ---------------------------------------------------------------------------------------------------- split-K
SPLIT = S.split_cases()


@pytest.mark.parametrize('c', SPLIT, ids=_ids(SPLIT))
def test_explicit_split_counts(K, record_property, c):
    """ksplit blocks per tile through an exactly sized slab: every partial tile is written, nothing behind the slab or the
    counters is, two launches agree bit for bit, and the unsplit launch (ksplit = 1) of the same operands holds the same bars."""
    total = {}
    Sn = c['ksplit']
    assert S.legality(c) is None and S.path(c, _cus()) == dict(shape=2, S=Sn, rounds=1 if S.split_tiles(c) * Sn <= _cus() else 2)
    for kind in S.KINDS:
        ops = Operands(K, c, _inputs(_key(c), kind), S.SCALE_MODES[Sn % 2])
        for name in (('all', 'none') if not c['dgrad'] else ('none',)):
            opts = S.options(name)
            what = '%s %s options %s' % (c['name'], kind, name)
            sc = Scratch(S.slab_floats(c, Sn), S.split_tiles(c))
            a, ratios = _launch(K, c, ops, opts, kind, what, shape=c['shape'], scratch=sc, ksplit=Sn, written=S.slab_floats(c, Sn))
            b, _ = _launch(K, c, ops, opts, kind, what + ' again', shape=c['shape'], scratch=sc, ksplit=Sn, written=S.slab_floats(c, Sn))
            for x, y in zip(a, b):
                assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), what + ': split launches differ from launch to launch'
            _merge(total, {'split_' + k: v for k, v in ratios.items()})
            sc1 = Scratch(S.slab_floats(c, Sn), S.split_tiles(c))
            u1, r1 = _launch(K, c, ops, opts, kind, what + ' ksplit 1', shape=c['shape'], scratch=sc1, ksplit=1, written=0)
            u2, _ = _launch(K, c, ops, opts, kind, what + ' no scratch', shape=c['shape'])
            for x, y in zip(u1, u2):
                assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), what + ': ksplit = 1 differs from a launch without scratch'
            _merge(total, r1)
    _record(record_property, total)


IGNORED = S.ignored_split_cases()


@pytest.mark.parametrize('c', IGNORED, ids=_ids(IGNORED))
def test_explicit_split_is_ignored_on_forced_shapes_1_3_4_5(K, record_property, c):
    """128-row blocks only: with a forced shape 1, 3, 4 or 5 an explicit ksplit > 1 runs unsplit -- the slab stays NaN, the bits are
    those of the launch without scratch."""
    total = {}
    assert S.path(c, _cus()) == dict(shape=c['shape'], S=1, rounds=0)
    for kind in S.KINDS:
        ops = Operands(K, c, _inputs(_key(c), kind), 'dev')
        what = '%s %s' % (c['name'], kind)
        sc = Scratch(S.slab_floats(c, c['ksplit']), S.split_tiles(c))
        a, ratios = _launch(K, c, ops, S.options('all'), kind, what, shape=c['shape'], scratch=sc, ksplit=c['ksplit'], written=0)
        b, _ = _launch(K, c, ops, S.options('all'), kind, what + ' no scratch', shape=c['shape'])
        for x, y in zip(a, b):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), what
        _merge(total, ratios)
    _record(record_property, total)


def test_two_tile_counts_share_the_counters_without_zeroing(K):
    """A launch leaves every counter at zero: a second launch with another tile count on the same counters is right too."""
    big, small = next(c for c in S.split_cases() if c['dgrad'] and c['Cin'] == 256), S.split_cases()[0]
    assert S.split_tiles(big) != S.split_tiles(small)
    sc = Scratch(max(S.slab_floats(big, big['ksplit']), S.slab_floats(small, small['ksplit'])), max(S.split_tiles(big), S.split_tiles(small)))
    for c in (big, small, big):
        view = sc.share(S.split_tiles(c))
        ops = Operands(K, c, _inputs(_key(c), 'ints'), 'dev')
        _launch(K, c, ops, S.options('all'), 'ints', c['name'] + ' shared counters', shape=c['shape'], scratch=view, ksplit=c['ksplit'])


def test_automatic_choices_at_this_cu_count(K, record_property):
    """shape = 0 / ksplit = 0 on geometries sized from the device's CU count: path() must name the outcome each case was built
    for (block shapes 5, 2, 4, 3; one round, two rounds, unsplit), and the slab must hold exactly the partial tiles of the split
    count it names."""
    cus = _cus()
    cases = S.auto_cases(cus)
    assert {c['expect']['shape'] for c in cases if not c['slab']} == {2, 3, 4, 5}
    assert {c['expect']['rounds'] for c in cases if c['slab']} == {0, 1, 2}
    total = {}
    for c in cases:
        assert S.legality(c) is None and S.path(c, cus) == c['expect'], (c['name'], S.path(c, cus))
        Sn = c['expect']['S']
        for kind in S.KINDS:
            ops = Operands(K, c, _inputs(_key(c), kind), 'dev')
            sc = Scratch(cus * 65536, S.split_tiles(c)) if c['slab'] else None      # (CUs * 65536 always suffices)
            what = '%s %s' % (c['name'], kind)
            _, ratios = _launch(K, c, ops, S.options('all'), kind, what, scratch=sc, ksplit=0,
                                written=(S.slab_floats(c, Sn) if Sn > 1 else 0) if c['slab'] else None)
            _merge(total, {('auto_split_' if Sn > 1 else 'auto_') + k: v for k, v in ratios.items()})
            del ops, sc
        _contraction.cache_clear()
        _inputs.cache_clear()
    _record(record_property, total)


# ---------------------------------------------------------------------------------------------------- refusals
MATCH = {'Cin32': 'Cin % 32', 'Cin80': 'Cin % 32', 'M192': 'M % 128', 'ks1': '2..8 taps', 'ks9': '2..8 taps', 'pad_left=ks': '2..8 taps',
         'bn_scale without bn_shift': 'bn_scale needs bn_shift', 'w_scale_inv=0': 'w_scale_inv must be positive',
         'shape3 at M384': 'shape is 0', 'shape4 at M256': 'shape is 0', 'shape6': 'shape is 0',
         'ksplit3 at 40 steps': 'do not divide into 3 even parts', 'ksplit8 at 40 steps': 'do not divide into 8 even parts',
         'slab one float short': 'split scratch too small', 'counters one short': 'split scratch too small',
         'slab without counters': 'needs split_counters'}


@pytest.mark.parametrize('name,c', S.refusal_cases(), ids=[n for n, _ in S.refusal_cases()])
def test_refusals_raise_and_launch_nothing(K, name, c):
    import re
    assert S.legality(c) is not None
    B, T, Cin, M, ks = c['B'], c['T'], c['Cin'], c['M'], c['ks']
    xp = torch.zeros(2 * 2 * Cin * B * T, dtype=torch.float16, device=DEV)
    wp = torch.zeros(2 * ks * Cin * M, dtype=torch.float16, device=DEV)
    out, save = Guarded(B * M * T), Guarded(B * M * T)
    vec = torch.ones(M, device=DEV)
    kw = dict(xp=xp, wp=wp, out=out.view, save_r=save.view, B=B, T=T, Cin=Cin, M=M, ks=ks, pad_left=c['pad_left'], bias=vec, relu=True,
              shape=c['shape'], w_scale_inv=c.get('w_scale_inv', 1.0), ksplit=c['ksplit'])
    if c.get('bn_scale'):
        kw.update(bn_scale=vec, bn_shift=vec if c.get('bn_shift', True) else None)
    sc = None
    if c['slab']:
        sc = Scratch(c.get('slab_floats', S.slab_floats(c, max(c['ksplit'], 1))), S.split_tiles(c))
        kw.update(split_slab=sc.slab.view, split_counters=sc.cfull[:c.get('counters_n', S.split_tiles(c))] if c.get('counters', True) else None)
    with pytest.raises((RuntimeError, ValueError), match=re.escape(MATCH[name])):
        K.f16x3_strided_conv(**kw)
    torch.cuda.synchronize()
    out.untouched(name + ' out')
    save.untouched(name + ' save_r')
    if sc is not None:
        sc.slab.untouched(name + ' slab')
        assert int(sc.counters.abs().sum()) == 0 and bool((sc.cfull[sc.tiles:] == ISENT).all())


def test_weight_gradient_refuses_a_length_that_is_no_multiple_of_4(K):
    B, T, Cp = 2, 38, S.WG_C
    p, q = torch.zeros(B, Cp, 2 * T, device=DEV), torch.zeros(B, Cp, T, device=DEV)
    dw = Guarded(5 * Cp * Cp)
    slab = torch.empty(_cus() * 65536, device=DEV)
    with pytest.raises(RuntimeError, match='multiple of 32'):
        K.f16x3_wgrad(p=p, q0=q, dw=dw.view, slab=slab, B=B, T=T, T_p=2 * T, Cp=Cp, Q0=Cp, taps=[-1, 0, 1, 2, 3], p_stride=2, mode=0)
    torch.cuda.synchronize()
    dw.untouched('dw')


# ---------------------------------------------------------------------------------------------------- weight gradient
WGRAD = S.wgrad_cases()


@pytest.fixture(scope='module')
def wg_slab():
    return torch.full((_cus() * 65536,), float('nan'), device=DEV)


@pytest.mark.parametrize('c', WGRAD, ids=_ids(WGRAD))
def test_stride2_weight_gradient(K, record_property, wg_slab, c):
    """Form (a): fp32 operands with p_stride = 2 (Tp = 2T and 2T - 1); form (b), where Tp = 2T: both operands as planes, p as
    space-to-depth planes with p_tap_chunk.  dw is accumulated onto pre-filled values in rows of lddw > Q0 floats; q_total over
    all columns or over a range onto pre-filled values.  (a) and (b) must agree bit for bit."""
    B, T, Tp, ks, pl, C, ld = c['B'], c['T'], c['Tp'], c['ks'], c['pad_left'], S.WG_C, S.WG_LDDW
    taps = S.wgrad_taps(c)
    total = {}
    ranged = bool(WGRAD.index(c) % 2)
    for kind in S.KINDS:
        ins = S.wgrad_inputs(c, kind)
        p, q = _dev(ins['p']), _dev(ins['q'])
        sc = torch.tensor([ins['sp'], ins['sq']], device=DEV)
        rows0 = np.full((ks, C, ld), S.SENTINEL, F32)
        rows0[:, :, :C] = ins['dw0']
        got = {}
        for form in ('a', 'b') if Tp == 2 * T else ('a',):
            cols = S.WG_TOTAL_COLS if ranged == (form == 'a') else None
            dw, tot = Guarded(ks * C * ld, init=rows0), Guarded(C, init=ins['total0'])
            kw = dict(dw=dw.view, slab=wg_slab, B=B, T=T, Cp=C, Q0=C, lddw=ld, p_scale=sc[0:1], q0_scale=sc[1:2], q_total=tot.view,
                      total_cols=cols, mode=0)
            if form == 'a':
                K.f16x3_wgrad(p=p, q0=q, taps=taps, p_stride=2, T_p=Tp, **kw)
            else:
                pp = torch.empty(2 * B * C * Tp, dtype=torch.float16, device=DEV)
                qp = torch.empty(2 * B * C * T, dtype=torch.float16, device=DEV)
                K.f16x3_split_activations(p, pp, B, C, Tp, scale_dev=sc[0:1], mode=K.X3_S2D)
                K.f16x3_split_activations(q, qp, B, C, T, scale_dev=sc[1:2], mode=0)
                K.f16x3_wgrad(p_planes=pp, p_planes_KC=2 * C // 8, p_tap_chunk=[(e & 1) * (C // 8) for e in taps], q_planes=qp,
                              taps=[e >> 1 for e in taps], **kw)
            torch.cuda.synchronize()
            what = '%s %s form (%s)' % (c['name'], kind, form)
            dw.guards_ok(what + ' dw')
            tot.guards_ok(what + ' q_total')
            rows = dw.host((ks, C, ld))
            assert np.array_equal(rows[:, :, C:].view(np.uint32), rows0[:, :, C:].view(np.uint32)), what + ': the columns behind Q0 of an lddw row changed'
            want, want_t, bar, bar_t, _ = S.wgrad_s2(ins['p'], ins['q'], taps, Tp, ins['sp'], ins['sq'], dw0=ins['dw0'], total0=ins['total0'],
                                                     total_cols=cols, q_from_planes=(form == 'b'), full=True)
            got[form] = np.ascontiguousarray(rows[:, :, :C])
            _merge(total, {'wgrad_' + form: _compare(got[form], want, bar, kind, what + ' dw')})
            t = tot.host((C,))
            if cols is not None:
                out = np.r_[0:cols[0], cols[1]:C]
                assert np.array_equal(t[out].view(np.uint32), ins['total0'][out].view(np.uint32)), what + ': q_total outside [total_o0, total_o1) changed'
            _merge(total, {'q_total_' + form: _compare(t, want_t, np.where(bar_t > 0, bar_t, 0.0), kind, what + ' q_total')})
        if 'b' in got:
            assert np.array_equal(got['a'].view(np.uint32), got['b'].view(np.uint32)), c['name'] + ' ' + kind + ': forms (a) and (b) differ'
    _record(record_property, total)


# ---------------------------------------------------------------------------------------------------- the reference on the device
def test_numpy_reference_matches_torch_float64_on_the_device():
    """The float64 statement once more with torch on the device (conv1d and its autograd over the decoded planes' values): the numpy
    reference every case above is held to agrees with it at 1e-12."""
    import torch.nn.functional as Fn
    c = next(t for t in TABLE if t['B'] == 7 and not t['dgrad'])
    ins = S.sconv_inputs(c, 'normal')
    pre, ab = S.fwd_pre(ins['x'], ins['w'], c['pad_left'], 1.0, 1.0, split=S.unsplit)
    x = _dev(ins['x']).double().requires_grad_(True)
    w = _dev(ins['w']).double()
    y = Fn.conv1d(Fn.pad(x, (c['pad_left'], c['ks'] - 2 - c['pad_left'])), w.permute(2, 1, 0), None, stride=2)
    assert np.abs(y.detach().cpu().numpy() - pre).max() <= 1e-12 * max(1.0, ab.max())
    dy = _dev(np.random.default_rng(3).standard_normal(pre.shape).astype(F32))
    want, = torch.autograd.grad(y, x, dy.double())
    dx, _, ab = S.sconv_dgrad(dy.cpu().numpy(), np.ascontiguousarray(ins['w'].transpose(0, 2, 1)), c['pad_left'], split=S.unsplit, full=True)
    assert np.abs(want.cpu().numpy() - dx).max() <= 1e-12 * max(1.0, ab.max())
