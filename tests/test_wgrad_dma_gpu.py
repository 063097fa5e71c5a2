"""The weight gradients with both operands as planes stage them by LDS-DMA into a ring of 16-step stages; that only changes HOW
the plane entries reach LDS.  Every dW of tests/wgrad_dma_cases.py is therefore
  * bit for bit what tests/golden/wgrad_dma_digests.json recorded at the commit before (the register ring),
  * bit for bit the fp32-operand launch (the register path, which converts the same fp16 pieces itself) wherever that launch
    is legal (T % 32 == 0, or T % 4 == 0 with p_stride 2),
  * inside 2e-6 max |dW| of the float64 sum over the plane values (tests/x3_ref.py) where it is not (T = 40, 72) and for the
    bf16 plane (rounded operands),
  * the same from one run to the next.
On top of that every unstrided dW, and the sums, are held elementwise to the plane-exact reference and bars of tests/x3_wgrad_ref.py.
A differing digest means a stage reached the MFMAs with other bytes: a step behind the row's end or before the batch row that
did not read zero, a stage read before it had landed, a ring slot refilled too early, a request past the block's K range that
was read after all.  q_total / q_seg are sums by atomics: held at the bounds of test_wgrad_f16x3_matches_fp64."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wgrad_dma_cases as W  # noqa: E402
import x3_ref as X  # noqa: E402
import x3_wgrad_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'wgrad_dma_digests.json')
CASES = W.cases()
DEV = W.DEV


@pytest.fixture(scope='module')
def want():
    with open(GOLDEN) as f:
        return json.load(f)


def _shift64(x, sh):
    """x [B][C][T] (float64) read at t + sh, either sign, zero outside [0, T) of the batch row."""
    T = x.shape[2]
    out = torch.zeros_like(x)
    if sh <= -T or sh >= T:
        return out
    if sh >= 0:
        out[:, :, :T - sh] = x[:, :, sh:]
    else:
        out[:, :, -sh:] = x[:, :, :T + sh]
    return out


def _dw64(kw, i, bf16):
    """float64 dW of problem i over the values the planes hold: a1 b1 + a1 b2 + a2 b1 of the two fp16 pieces, or the product of the
    bf16-rounded operands; divided by the two scales."""
    p, q = W.operands(kw['B'], kw['T'], kw['Q0'], kw.get('seed', 0) + i)
    _, _, sp, sq = W.problem_scales(i)
    if bf16:
        pp = [torch.from_numpy(X.bf16_round(X.scaled(p, 1.0, sp))).to(DEV)]
        qq = [torch.from_numpy(X.bf16_round(X.scaled(q, 1.0, sq))).to(DEV)]
        terms = ((0, 0),)
    else:
        pp = [torch.from_numpy(h.astype(np.float64)).to(DEV) for h in X.split(X.scaled(p, 1.0, sp))]
        qq = [torch.from_numpy(h.astype(np.float64)).to(DEV) for h in X.split(X.scaled(q, 1.0, sq))]
        terms = ((0, 0), (0, 1), (1, 0))
    dw = []
    for sh in kw['taps'][i]:
        dw.append(sum(torch.einsum('bct,bot->co', _shift64(pp[a], sh), qq[b]) for a, b in terms))
    return torch.stack(dw) / (sp * sq)


def test_table_is_the_recorded_one(want):
    assert sorted(n for n, _ in CASES) == sorted(want) and len(CASES) == len(set(n for n, _ in CASES)) == 30


@pytest.mark.parametrize('name,kw', CASES, ids=[n for n, _ in CASES])
def test_planes_both_matches_the_parent_and_the_register_path(K, want, name, kw):
    got = W.run(K, **kw)
    again = W.run(K, **kw)
    torch.cuda.synchronize()
    dws = sorted(k for k in got if k.startswith('dw'))
    assert len(dws) == len(kw['taps'])
    for k in dws:
        assert bool(torch.isfinite(got[k]).all()) and float(got[k].abs().max()) > 0.0, '%s: %s is empty or not finite' % (name, k)
        assert torch.equal(got[k], again[k]), '%s: %s differs between two runs' % (name, k)
    assert W.digest(got) == want[name], '%s: dW is not the parent commit\'s' % name
    if W.has_fp32_twin(kw):
        ref = W.run(K, form='fp32', **kw)
        for k in dws:
            assert torch.equal(got[k], ref[k]), '%s: %s differs from the fp32-operand launch' % (name, k)
    bf16 = bool(kw.get('mode', 0) & W.X3_BF16)
    if (not W.has_fp32_twin(kw) or bf16) and not kw.get('strided', False):
        for i, k in enumerate(dws):
            w64 = _dw64(kw, i, bf16)
            err, top = float((got[k].double() - w64).abs().max()), float(w64.abs().max())
            print('%s %s: max err %.3e, bar %.3e' % (name, k, err, 2e-6 * top))
            assert err <= 2e-6 * top, '%s: %s is %.3e from float64 of the plane values (bar %.3e)' % (name, k, err, 2e-6 * top)
    if not kw.get('strided', False):
        block = kw.get('dw_form') == 'block'
        for i, k in enumerate(dws):
            p, q = W.operands(kw['B'], kw['T'], kw['Q0'], kw.get('seed', 0) + i)
            _, _, sp, sq = W.problem_scales(i)
            ns = min(kw['nsplit'], R.pairs(kw['B'], kw['T'])[1])
            w64, t64, _, bar, bar_t, _, _ = R.wgrad(p, q, None, kw['taps'][i], sp, sq, mode=kw.get('mode', 0), p_planes=True, q_planes=True, nsplit=ns,
                                                    total=block, total_cols=(64, kw['Q0'] - 32) if block else None, full=True)
            dev = got[k].cpu().numpy().astype(np.float64)
            dev = dev[None, :, 512:] if block else dev
            over = np.abs(dev - w64) > bar
            assert not over.any(), '%s: %d elements of %s outside the elementwise bars of x3_wgrad_ref (worst %.3f of its bar)' % (
                name, int(over.sum()), k, float((np.abs(dev - w64) / bar).max()))
            if block:
                assert not (np.abs(got['tot%d' % i].cpu().numpy().astype(np.float64) - t64) > bar_t).any(), '%s: bias sums outside the bars of x3_wgrad_ref' % name
    if kw.get('dw_form') == 'block':
        lo, hi = 64, kw['Q0'] - 32
        for i, k in enumerate(dws):
            assert float(got[k][:, :512].abs().max()) == 0.0, '%s: columns in front of the block were written' % name
            q = torch.from_numpy(W.operands(kw['B'], kw['T'], kw['Q0'], kw.get('seed', 0) + i)[1]).to(DEV).double()
            tot = got['tot%d' % i].double()
            assert float(tot[:lo].abs().max()) == 0.0 and float(tot[hi:].abs().max()) == 0.0, '%s: q_total outside total_cols was written' % name
            bad = (tot[lo:hi] - q.sum((0, 2))[lo:hi]).abs() > 1e-5 * q.abs().sum((0, 2))[lo:hi]
            assert not bool(bad.any()), '%s: %d bias sums outside 1e-5 sum |q|' % (name, int(bad.sum()))


@pytest.mark.parametrize('mode', [0, W.X3_BF16], ids=['f16x3', 'bf16'])
def test_q_sums_from_the_fragments(K, mode):
    """q_seg / q_total of a batch of two problems, formed from the B fragments of the stages (flushed behind each pair's second
    stage): pairs that start a condition frame, end one and cross a batch row, over K splits that cut inside a frame."""
    B, T, Q0, Tz = 2, 192, 512, 2
    probs, segs, tots, qs = [], [], [], []
    for i, taps in enumerate(([-4, -2, 0], [-192, -96, 0])):
        p, q = W.operands(B, T, Q0, 50 + i)
        spd, sqd, sp, sq = W.problem_scales(i)
        seg, tot = torch.zeros(B, Q0 + 3, Tz, device=DEV), torch.zeros(Q0, device=DEV)
        pd, qd = torch.from_numpy(p).to(DEV), torch.from_numpy(q).to(DEV)
        probs.append(dict(p_planes=W._planes(K, pd, B, W.CP, T, spd, mode), q_planes=W._planes(K, qd, B, Q0, T, sqd, mode), taps=taps,
                          p_scale=spd, q0_scale=sqd, dw=torch.zeros(3, W.CP, Q0, device=DEV), q_seg=seg, q_total=tot))
        segs.append(seg)
        tots.append(tot)
        # (the sums are formed from the planes: of the ROUNDED q where there is one bf16 plane)
        qs.append(torch.from_numpy(X.bf16_round(X.scaled(q, 1.0, sq)) / sq).to(DEV) if mode else qd.double())
    K.f16x3_wgrad_batch(probs, slab=W.slab(), B=B, T=T, Cp=W.CP, Q0=Q0, nsplit=5, seg_T=Tz, seg_bstride=(Q0 + 3) * Tz, mode=mode)
    for i in range(2):
        q = qs[i]
        bad = (tots[i].double() - q.sum((0, 2))).abs() > 1e-5 * q.abs().sum((0, 2))
        assert not bool(bad.any()), 'problem %d: %d column totals outside 1e-5 sum |q|' % (i, int(bad.sum()))
        err = float((segs[i][:, :Q0].double() - q.reshape(B, Q0, Tz, T // Tz).sum(-1)).abs().max())
        assert err <= 1e-5 * float(q.abs().max()) * 32 * (T // Tz // 32), 'problem %d: segment sums off by %.3e' % (i, err)
        assert float(segs[i][:, Q0:].abs().max()) == 0.0, 'the slack between the batch rows was written'
        # and elementwise against the reference: (terms + 3) u sum |q| per sum, of what the planes hold
        p, q32 = W.operands(B, T, Q0, 50 + i)
        _, _, sp, sq = W.problem_scales(i)
        _, t64, s64, _, bar_t, bar_s, _ = R.wgrad(p, q32, None, probs[i]['taps'], sp, sq, mode=mode, p_planes=True, q_planes=True, nsplit=5, total=True, seg_T=Tz,
                                                  csel=np.arange(8), full=True)
        assert not (np.abs(tots[i].cpu().numpy().astype(np.float64) - t64) > bar_t).any(), 'problem %d: column totals outside the bars of x3_wgrad_ref' % i
        assert not (np.abs(segs[i][:, :Q0].cpu().numpy().astype(np.float64) - s64) > bar_s).any(), 'problem %d: segment sums outside the bars of x3_wgrad_ref' % i
