"""The LDS-DMA weight-gradient kernel (both operands as planes) tiles its 256 x 256 block 2 x 2 over the four waves -- wave
(wr, wc) owns rows 128 wr .., columns 128 wc .. -- and forms the q sums only in the blocks that use them, in a loop body chosen
in front of the loop.  Neither changes a bit of dW: per accumulator the K steps and the three terms come in the order they had.
What can go wrong is the read map (a wave multiplying another wave's fragments), the slab index, the owner of a q sum and the
choice of the loop body; so, at Cp = 256 and small T:
  * one and two column tiles (Q0 = 256, 512: with two, every (wr, wc) owns different data in both operands),
  * T = 256 (whole 32-step pairs, a K range that crosses the batch row) and T = 40, 72 (steps behind the row's end read as zero),
  * one tap, three causal taps of dilation 1 (unaligned shifts), 4, and 32 at T = 40 (a whole tap in the padding),
  * launches whose blocks partly sum (q_seg: tap 0 only; q_total over a column range that ends inside the first column tile) and
    one that sums nowhere, beside buffers that must stay as they are,
  * a batch of two problems with different scales.
Bars, all the project's: dW torch.equal to the fp32-operand launch (the register kernel) where that launch is legal, inside
2e-6 max |dW| of the float64 sum over the plane values (tests/x3_ref.py) at T = 40 / 72; column totals inside 1e-5 sum |q|,
segment sums inside 1e-5 max |q| 32 (T // Tz // 32) (test_q_sums_from_the_fragments)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wgrad_dma_cases as W  # noqa: E402
import x3_ref as X  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = W.DEV
B, TZ = 2, 2
PART = (64, 224)          # q_total over these columns only: the second column tile of Q0 = 512 has nothing to sum
ONE, D1, D4, D32 = [0], [-2, -1, 0], [-8, -4, 0], [-64, -32, 0]


def _c(name, T, Q0, taps, nsplit, sums, mode=0):
    return name, dict(T=T, Q0=Q0, taps=taps, nsplit=nsplit, sums=sums, mode=mode)


CASES = [
    # whole pairs: against the fp32-operand launch
    _c('T=256/Q0=256/1x1/seg', 256, 256, [ONE], 3, 'seg'),
    _c('T=256/Q0=512/d=1/seg+total', 256, 512, [D1], 3, 'seg+total'),
    _c('T=256/Q0=512/d=4/total-part', 256, 512, [D4], 2, 'total-part'),
    _c('T=256/Q0=256/d=4/none', 256, 256, [D4], 1, 'none'),
    _c('T=256/Q0=512/d=1/none', 256, 512, [D1], 3, 'none'),
    _c('T=256/Q0=512/batch/seg+total', 256, 512, [D1, D4], 3, 'seg+total'),
    _c('T=256/Q0=512/batch/bf16/seg', 256, 512, [D4, D1], 2, 'seg', W.X3_BF16),
    # rows that are no whole pairs: against float64 (q_seg needs whole pairs)
    _c('T=40/Q0=512/1x1/none', 40, 512, [ONE], 2, 'none'),
    _c('T=40/Q0=512/d=1/total-part', 40, 512, [D1], 1, 'total-part'),
    _c('T=40/Q0=256/d=4/total', 40, 256, [D4], 2, 'total'),
    _c('T=40/Q0=512/d=32/total', 40, 512, [D32], 2, 'total'),
    _c('T=72/Q0=256/1x1/total', 72, 256, [ONE], 3, 'total'),
    _c('T=72/Q0=512/d=1/none', 72, 512, [D1], 2, 'none'),
    _c('T=72/Q0=512/d=4/total-part', 72, 512, [D4], 3, 'total-part'),
    _c('T=72/Q0=256/batch/total', 72, 256, [D1, D4], 2, 'total'),
]


def _launch(K, form, *, T, Q0, taps, nsplit, sums, mode):
    """One launch of the batch; problem i: operands of seed 70 + i, its own scales.  -> [(dw, q_seg or None, q_total or None)]"""
    probs, outs = [], []
    for i, tp in enumerate(taps):
        p, q = W.operands(B, T, Q0, 70 + i)
        spd, sqd, _, _ = W.problem_scales(i)
        pd, qd = torch.from_numpy(p).to(DEV), torch.from_numpy(q).to(DEV)
        dw = torch.zeros(len(tp), W.CP, Q0, device=DEV)
        seg = torch.zeros(B, Q0, TZ, device=DEV) if 'seg' in sums else None
        tot = torch.zeros(Q0, device=DEV) if 'total' in sums else None
        pr = dict(dw=dw, taps=list(tp), p_scale=spd, q0_scale=sqd, q_seg=seg, q_total=tot)
        if form == 'planes':
            pr.update(p_planes=W._planes(K, pd, B, W.CP, T, spd, mode), q_planes=W._planes(K, qd, B, Q0, T, sqd, mode))
        else:
            pr.update(p=pd, q0=qd)
        probs.append(pr)
        outs.append((dw, seg, tot))
    common = dict(slab=W.slab(), B=B, T=T, Cp=W.CP, Q0=Q0, nsplit=nsplit, mode=mode)
    if 'seg' in sums:
        common.update(seg_T=TZ)
    if sums.endswith('total-part'):
        common.update(total_cols=PART)
    K.f16x3_wgrad_batch(probs, **common)
    return outs


def _shift64(x, sh):
    """x [B][C][T] (float64) read at t + sh (sh <= 0), zero before the batch row's first step."""
    out = torch.zeros_like(x)
    if -sh < x.shape[2]:
        out[:, :, -sh:] = x[:, :, :x.shape[2] + sh]
    return out


def _dw64(T, Q0, taps, i):
    """float64 dW of problem i over the values the two fp16 planes hold (a1 b1 + a1 b2 + a2 b1), descaled."""
    p, q = W.operands(B, T, Q0, 70 + i)
    _, _, sp, sq = W.problem_scales(i)
    pp = [torch.from_numpy(h.astype(np.float64)).to(DEV) for h in X.split(X.scaled(p, 1.0, sp))]
    qq = [torch.from_numpy(h.astype(np.float64)).to(DEV) for h in X.split(X.scaled(q, 1.0, sq))]
    dw = [sum(torch.einsum('bct,bot->co', _shift64(pp[a], sh), qq[b]) for a, b in ((0, 0), (0, 1), (1, 0))) for sh in taps]
    return torch.stack(dw) / (sp * sq)


@pytest.mark.parametrize('name,kw', CASES, ids=[n for n, _ in CASES])
def test_tiled_loop_matches_the_register_path_and_sums_where_asked(K, name, kw):
    T, Q0, sums, mode = kw['T'], kw['Q0'], kw['sums'], kw['mode']
    # buffers of a neighbouring problem, beside the launch's own: a block that sums without being asked has nowhere else to write
    guard_seg, guard_tot = torch.full((B, Q0, TZ), 3.25, device=DEV), torch.full((Q0,), -1.5, device=DEV)
    got = _launch(K, 'planes', **kw)
    ref = _launch(K, 'fp32', **kw) if T % 32 == 0 else None
    torch.cuda.synchronize()
    assert len(got) == len(kw['taps'])
    for i, (dw, seg, tot) in enumerate(got):
        assert bool(torch.isfinite(dw).all()) and float(dw.abs().max()) > 0.0, '%s: dw of problem %d is empty or not finite' % (name, i)
        if ref is not None:
            assert torch.equal(dw, ref[i][0]), '%s: dw of problem %d differs from the fp32-operand launch' % (name, i)
        else:
            assert mode == 0
            w64 = _dw64(T, Q0, kw['taps'][i], i)
            err, top = float((dw.double() - w64).abs().max()), float(w64.abs().max())
            print('%s problem %d: max err %.3e, bar %.3e' % (name, i, err, 2e-6 * top))
            assert err <= 2e-6 * top, '%s: dw of problem %d is %.3e from float64 of the plane values (bar %.3e)' % (name, i, err, 2e-6 * top)
        q = W.operands(B, T, Q0, 70 + i)[1]
        _, _, _, sq = W.problem_scales(i)
        # (the sums are formed from the planes: of the ROUNDED q where there is one bf16 plane)
        q = torch.from_numpy(X.bf16_round(X.scaled(q, 1.0, sq)) / sq if mode else q.astype(np.float64)).to(DEV)
        assert (seg is not None) == ('seg' in sums) and (tot is not None) == ('total' in sums)
        if tot is not None:
            lo, hi = PART if sums.endswith('total-part') else (0, Q0)
            assert float(tot[:lo].abs().max() if lo else 0.0) == 0.0 and float(tot[hi:].abs().max() if hi < Q0 else 0.0) == 0.0, \
                '%s: q_total outside its columns was written (problem %d)' % (name, i)
            bad = (tot.double() - q.sum((0, 2)))[lo:hi].abs() > 1e-5 * q.abs().sum((0, 2))[lo:hi]
            assert not bool(bad.any()), '%s: %d column totals of problem %d outside 1e-5 sum |q|' % (name, int(bad.sum()), i)
        if seg is not None:
            err = float((seg.double() - q.reshape(B, Q0, TZ, T // TZ).sum(-1)).abs().max())
            bar = 1e-5 * float(q.abs().max()) * 32 * (T // TZ // 32)
            print('%s problem %d: segment sums off by %.3e, bar %.3e' % (name, i, err, bar))
            assert err <= bar, '%s: segment sums of problem %d off by %.3e (bar %.3e)' % (name, i, err, bar)
    assert bool((guard_seg == 3.25).all()) and bool((guard_tot == -1.5).all()), '%s: buffers that were not passed were written' % name
