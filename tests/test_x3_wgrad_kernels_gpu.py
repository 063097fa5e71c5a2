"""vqw_f16x3_wgrad / vqw_f16x3_wgrad_batch with p_stride 1 against the plane-exact float64 reference of tests/x3_wgrad_ref.py, through
kernels.py (f16x3_wgrad, f16x3_wgrad_batch), at the smallest shapes at which each mechanism exists: one, two, three and six pairs
of 16-step stages per batch row, one and two row tiles, one to three column tiles, 1 .. 17 K splits, 1 .. 32 problems.

Every dw (with its lddw slack, its tap-stride gap and the columns in front of a column block), q_total and q_seg (with its
seg_bstride slack) is a view into a sentinel-filled buffer; the slab is a NaN-filled view of exactly tiles * nsplit * 65536 floats
inside a sentinel buffer, nsplit being what path(case, CUs) names: afterwards no NaN is left in it, and whatever a launch does not
own keeps its bits.  Operands that come as planes are the exact uint16 images of tests/x3_ref.act_planes, inside wider tensors
where the case says so.  Integer cases must equal the reference bit for bit in dw, q_total and q_seg, standard-normal cases stay
within the elementwise bars, and a refusal must raise with the launcher's own message and leave every output's bits alone.

Every test records err / bar of its case (record_property 'err_over_bar_<output>') and prints it; DESIGN 6 lists the maxima per
family.  (Nine taps cannot be asked for through kernels.py: the descriptor has eight slots.)"""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import x3_wgrad_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F32 = np.float32
G = R.GUARD
SENT = float(R.SENTINEL)
WORST = {}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def _bits(t):
    return t.view(torch.int32)


class Guarded:
    """n floats between two guard bands of sentinels; `view` is what the kernel gets (16-byte aligned).  img: the view's contents
    before the launch (default: sentinels); fill: one value for all of it."""

    def __init__(self, n, img=None, fill=None, tail=G):
        self.n = n
        self.full = torch.full((G + n + tail,), SENT, device=DEV)
        self.view = self.full[G:G + n]
        if img is not None:
            self.view.copy_(_dev(np.asarray(img, F32).reshape(-1)))
        elif fill is not None:
            self.view.fill_(fill)
        self.before = self.full.clone() if fill is None else None
        assert self.view.data_ptr() % 16 == 0

    def guards_ok(self, what):
        edge = torch.cat([self.full[:G], self.full[G + self.n:]])
        assert bool((_bits(edge) == _bits(torch.tensor([SENT], device=DEV))).all()), what + ': a guard band changed'

    def untouched(self, what):
        if self.before is None:
            self.guards_ok(what)
            assert bool(torch.isnan(self.view).all()), what + ': written'
        else:
            assert torch.equal(_bits(self.full), _bits(self.before)), what + ': changed'

    def host(self):
        return self.view.cpu().numpy()


def dw_layout(c, nt):
    """(row length, tap stride, floats, flat index of dw[j][c][o]) of a case's dw buffer: rows of lddw floats (a column block starts
    at column col0 of them), taps tap_gap floats further apart than Cp rows."""
    Q = c['Q0'] + c['Q1']
    ld = (c['lddw'] or Q) + c['col0']
    ts = c['Cp'] * ld + c['tap_gap']
    cells = (np.arange(nt)[:, None, None] * ts + np.arange(c['Cp'])[None, :, None] * ld + c['col0'] + np.arange(Q)[None, None, :])
    return ld, ts, (max(nt, 1) - 1) * ts + c['Cp'] * ld + max(0, c['col0'] + Q - ld), cells      # (a refused lddw below Q0 + Q1: rows overlap)


def seg_layout(c):
    Q = c['Q0'] + c['Q1']
    bs = c['seg_bstride'] or Q * c['seg_T']
    cells = np.arange(c['B'])[:, None, None] * bs + np.arange(Q)[None, :, None] * c['seg_T'] + np.arange(c['seg_T'])[None, None, :]
    return bs, c['B'] * max(bs, Q * c['seg_T']), cells


def _planes_tensor(img):
    return None if img is None else _dev(img.view(np.int16)).view(torch.float16).reshape(-1)


class Launch:
    """The buffers and keyword arguments of one launch of a case (n problems), on operands of one kind."""

    def __init__(self, c, kind, slab_floats):
        self.c, self.kind = c, kind
        n, Q = c['n'], c['Q0'] + c['Q1']
        pp, qp = R._is_pp(c), R._is_qp(c)
        taps = R.all_taps(c)
        self.taps = [taps[i % len(taps)] for i in range(n)]
        nt = len(self.taps[0])
        self.ld, self.ts, dw_floats, self.cells = dw_layout(c, nt)
        self.slab = Guarded(slab_floats, fill=float('nan'), tail=4096)
        self.ins, self.dw, self.tot, self.seg, self.problems, self.keep = [], [], [], [], [], []
        for i in range(n):
            ins = R.inputs(c, kind, i) if i < R.MAX_BATCH else self.ins[0]
            self.ins.append(ins)
            img = np.full(dw_floats, R.SENTINEL, F32)
            if nt:
                img[self.cells.reshape(-1)] = ins['dw0'].reshape(-1)
            dw = Guarded(dw_floats + (1 if c.get('dw_misaligned') else 0), img=np.r_[img, [R.SENTINEL] * (1 if c.get('dw_misaligned') else 0)])
            sc = torch.tensor([ins['sp'], ins['sq0'], ins['sq1']], device=DEV)
            pr = dict(dw=dw.view[c['col0'] + (1 if c.get('dw_misaligned') else 0):], taps=self.taps[i], p_scale=sc[0:1], q0_scale=sc[1:2])
            pimg, qimg = R.plane_images(c, ins)
            if pp:
                pr['p_planes'] = _planes_tensor(pimg)
            else:
                pr['p'] = _dev(ins['p'])
            if qp and not (c.get('planes_in_one_problem') and i == 1):
                pr['q_planes'] = _planes_tensor(qimg)
            else:
                pr['q0'] = _dev(ins['q0'][:, :c['Q0']])
            if c['Q1']:
                pr.update(q1=_dev(ins['q1']), q1_scale=sc[2:3])
            if c['total']:
                self.tot.append(Guarded(Q, img=ins['total0']))
                pr['q_total'] = self.tot[-1].view
            if c['seg_T']:
                bs, floats, cells = seg_layout(c)
                simg = np.full(floats, R.SENTINEL, F32)
                simg[cells.reshape(-1)] = 0.0
                self.seg.append(Guarded(floats, img=simg))
                pr['q_seg'] = self.seg[-1].view
            if c.get('shape_differs') and i == 1:
                pr['p_relu'] = True
            self.dw.append(dw)
            self.problems.append(pr)
            self.keep.append(sc)
        self.common = dict(slab=self.slab.view, B=c['B'], T=c['T'], Cp=c['Cp'], Q0=c['Q0'], Q1=c['Q1'], nsplit=c['nsplit'], mode=c['mode'],
                           p_relu=c['p_relu'])
        if c['lddw'] or c['col0'] or c['tap_gap']:
            self.common.update(lddw=self.ld, dw_tap_stride=self.ts)
        if c['total']:
            self.common['total_cols'] = c['total_cols']
        if c['seg_T']:
            self.common.update(seg_T=c['seg_T'], seg_bstride=c['seg_bstride'])
        if pp:
            self.common.update(p_planes_KC=c['p_KC'], p_planes_kc0=c['p_kc0'], p_tap_chunk=c['p_tap_chunk'],
                               p_planes_scale=0.0 if c['p_hscale'] == 1.0 else c['p_hscale'])
        if qp:
            self.common.update(q_planes_KC=c['q_KC'], q_planes_kc0=c['q_kc0'], q_planes_scale=0.0 if c['q_hscale'] == 1.0 else c['q_hscale'])
        if 'p_stride' in c:
            self.common['p_stride'] = c['p_stride']

    def run(self, K):
        if self.c['n'] == 1:
            K.f16x3_wgrad(**dict(self.common, **self.problems[0]))
        else:
            K.f16x3_wgrad_batch(self.problems, **self.common)
        torch.cuda.synchronize()

    def outputs(self):
        return [dict(dw=d.host(), tot=self.tot[i].host() if self.tot else None, seg=self.seg[i].host() if self.seg else None)
                for i, d in enumerate(self.dw)]

    def untouched(self, what):
        for bufs, name in ((self.dw, 'dw'), (self.tot, 'q_total'), (self.seg, 'q_seg')):
            for i, b in enumerate(bufs[:R.MAX_BATCH]):
                b.untouched('%s: %s of problem %d' % (what, name, i))
        self.slab.untouched(what + ': slab')


def _compare(got, want, bar, kind, what):
    """err / bar (0 for a bit-exact kind)."""
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


def _same_elsewhere(img, before, cells, what):
    """Everything of a buffer but its cells kept its bits."""
    mask = np.ones(img.size, bool)
    mask[cells.reshape(-1)] = False
    assert np.array_equal(img[mask].view(np.uint32), before[mask].view(np.uint32)), what + ' changed'


def run_case(K, c, kind, again=False):
    """Launch a case, check guards, slack and slab, compare every problem to the reference.  Returns ({output: err / bar}, the raw
    outputs)."""
    pth = R.path(c, _cus())
    ns, tl = pth['nsplit'], pth['tiles']
    L = Launch(c, kind, tl * ns * R.TILE_FLOATS)
    before = [d.host().copy() for d in L.dw]
    seg_before = [s.host().copy() for s in L.seg]
    L.run(K)
    if again:
        first = L.outputs()
        for d, b in zip(L.dw, before):
            d.view.copy_(_dev(b))
        for i, t in enumerate(L.tot):
            t.view.copy_(_dev(L.ins[i]['total0']))
        for s, b in zip(L.seg, seg_before):
            s.view.copy_(_dev(b))
        L.slab.view.fill_(float('nan'))
        L.run(K)
    what = '%s %s (%s, %d splits)' % (c['name'], kind, '/'.join(str(x) for x in R.instantiation(pth)), ns)
    L.slab.guards_ok(what + ' slab')
    left = int(torch.isnan(L.slab.view).sum())
    assert left == 0, '%s: %d floats of the slab of %d tiles x %d splits were not written' % (what, left, tl, ns)
    outs = L.outputs()
    ratios = {}
    Q = c['Q0'] + c['Q1']
    for i, o in enumerate(outs):
        w = '%s problem %d' % (what, i)
        L.dw[i].guards_ok(w + ' dw')
        _same_elsewhere(o['dw'], before[i], L.cells, w + ': lddw slack, tap-stride gap or columns outside the block')
        dw, tot, seg, bar, bar_t, bar_s, _ = R.reference(c, L.ins[i], i, nsplit=ns)
        ratios['dw'] = max(ratios.get('dw', 0.0), _compare(o['dw'][L.cells], dw, bar, kind, w + ' dw'))
        if c['total']:
            L.tot[i].guards_ok(w + ' q_total')
            if c['total_cols']:
                out = np.r_[0:c['total_cols'][0], c['total_cols'][1]:Q]
                assert np.array_equal(o['tot'][out].view(np.uint32), L.ins[i]['total0'][out].view(np.uint32)), w + ': q_total outside [total_o0, total_o1) changed'
            ratios['q_total'] = max(ratios.get('q_total', 0.0), _compare(o['tot'], tot, bar_t, kind, w + ' q_total'))
        if c['seg_T']:
            L.seg[i].guards_ok(w + ' q_seg')
            cells = seg_layout(c)[2]
            _same_elsewhere(o['seg'], seg_before[i], cells, w + ': seg_bstride slack')
            ratios['q_seg'] = max(ratios.get('q_seg', 0.0), _compare(o['seg'][cells], seg, bar_s, kind, w + ' q_seg'))
        if again:
            for k in ('dw', 'tot', 'seg'):
                assert o[k] is None or (k != 'dw' and kind == 'normal') or np.array_equal(o[k].view(np.uint32), first[i][k].view(np.uint32)), \
                    w + ': %s differs between two launches' % k
    return ratios, outs, L


def _note(record_property, c, ratios):
    fam = WORST.setdefault(c['family'], {})
    for k, v in ratios.items():
        fam[k] = max(fam.get(k, 0.0), v)
        record_property('err_over_bar_' + k, v)
    print('%s: err / bar %s' % (c['name'], ', '.join('%s %.4f' % kv for kv in sorted(ratios.items()))))


def _both_kinds(K, record_property, c, again=False):
    total = {}
    for kind in R.KINDS:
        ratios, _, _ = run_case(K, c, kind, again)
        for k, v in ratios.items():
            total[k] = max(total.get(k, 0.0), v)
    _note(record_property, c, total)


def _ids(cases):
    return [c['name'] for c in cases]


FORM_CASES = R.form_cases()


@pytest.mark.parametrize('c', FORM_CASES, ids=_ids(FORM_CASES))
def test_operand_forms(K, record_property, c):
    """Every operand form against the reference; on top of that, a form with planes gives the bits of the fp32-operand launch on the
    same operands (the planes are the images of what that launch splits itself)."""
    total = {}
    for kind in R.KINDS:
        ratios, outs, _ = run_case(K, c, kind)
        total.update({k: max(total.get(k, 0.0), v) for k, v in ratios.items()})
        if c['form'] != 'ff':
            twin = dict(c, form='ff', total=False)
            _, ref, _ = run_case(K, twin, kind)
            assert np.array_equal(outs[0]['dw'].view(np.uint32), ref[0]['dw'].view(np.uint32)), '%s %s: dw differs from the fp32-operand launch' % (c['name'], kind)
    _note(record_property, c, total)


def test_the_forms_reach_all_twelve_stride1_instantiations():
    assert {R.instantiation(R.path(c, _cus())) for c in R.all_cases()} == set(R.stride1_instantiations())
    assert {R.instantiation(R.path(c, _cus())) for c in FORM_CASES} == set(R.stride1_instantiations())


OTHER = R.tap_cases() + R.rowcol_cases() + R.split_cases() + R.auto_cases() + R.sums_cases() + R.relu_cases() + R.wide_cases()


@pytest.mark.parametrize('c', OTHER, ids=_ids(OTHER))
def test_taps_tiles_splits_sums_relu_and_wider_planes(K, record_property, c):
    _both_kinds(K, record_property, c)


def test_a_tap_in_the_padding_adds_exact_zeros(K):
    """dw of a tap that lies in the padding throughout keeps the bits it held, on standard-normal operands too."""
    for name in ('taps/ff-T64-padding', 'taps/pq-T96-padding', 'taps/fq-padding'):
        c = next(x for x in OTHER if x['name'] == name)
        _, outs, L = run_case(K, c, 'normal')
        for j, sh in enumerate(c['taps']):
            if -sh >= c['T']:
                assert np.array_equal(outs[0]['dw'][L.cells[j]].view(np.uint32), L.ins[0]['dw0'][j].view(np.uint32)), '%s: tap %d changed dw' % (name, sh)


def test_the_automatic_split_is_the_one_path_names(K):
    """nsplit = 0 at 48 tiles: CUs / 48 partial tiles each, unclamped wherever the device has 96 .. 335 CUs; run_case sized the slab by
    it -- one split more is refused, one less leaves NaNs."""
    c = R.auto_cases()[0]
    pth = R.path(c, _cus())
    assert pth['tiles'] == 48 and pth['nsplit'] == max(1, min(_cus() // 48, 6))
    assert not 96 <= _cus() < 288 or 1 < pth['nsplit'] < 6
    run_case(K, c, 'ints')


BATCHES = R.batch_cases()


@pytest.mark.parametrize('c', BATCHES, ids=_ids(BATCHES))
def test_batches(K, record_property, c):
    """Each problem against the reference on its own operands, taps, scales and sums; two launches give the same dw bits."""
    _both_kinds(K, record_property, c, again=True)


def test_slab_one_tile_short_is_refused_and_nothing_written(K):
    c = R._case('refusals/slab', taps=(-2, -1, 0), nsplit=3, total=True, seg_T=1)
    L = Launch(c, 'ints', (3 * 3 - 1) * R.TILE_FLOATS)
    with pytest.raises(RuntimeError, match=re.escape('slab too small (3 tiles x 3 splits x 65536 floats)')):
        L.run(K)
    torch.cuda.synchronize()
    L.untouched(c['name'])


REFUSALS = R.refusal_cases()


@pytest.mark.parametrize('name,c,msg', REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_raise_and_write_nothing(K, name, c, msg):
    assert R.legality(c) is not None
    floats = 16 * R.TILE_FLOATS                 # enough for every case here: the rule under test is the one that refuses
    if c.get('slab_short'):
        pth = R.path(c, _cus())
        floats = (pth['tiles'] * pth['nsplit'] - 1) * R.TILE_FLOATS
    L = Launch(c, 'ints', floats)
    with pytest.raises((RuntimeError, ValueError), match=re.escape(msg)):
        L.run(K)
    torch.cuda.synchronize()
    L.untouched(name)


def test_print_the_worst_ratios_per_family():
    for fam in sorted(WORST):
        print('%-8s %s' % (fam, ', '.join('%s %.4f' % kv for kv in sorted(WORST[fam].items()))))
