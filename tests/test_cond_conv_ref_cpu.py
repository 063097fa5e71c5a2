"""CPU tests of tests/cond_conv_ref.py: the float64 restatement of the conditioning conv against torch's conv1d and autograd in
float64, and that the GPU cases (tests/test_cond_conv_kernels_gpu.py) at their bars would catch the wrong kernels of CR.FLAWS."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cond_conv_ref as CR  # noqa: E402


def close(got, want, what):
    err = np.abs(np.asarray(got) - np.asarray(want)).max()
    assert err <= 1e-12 * max(np.abs(want).max(), 1e-300), '%s: %.3e' % (what, err)


@pytest.mark.parametrize('case', CR.CASES, ids=CR.case_id)
def test_reference_matches_torch_float64(case):
    B, D, C, Tz, k = case
    z, w, bias, dout, dw0, db0 = (torch.from_numpy(a).double() for a in CR.operands(case, 'random'))
    z.requires_grad_(True)
    w.requires_grad_(True)
    bias.requires_grad_(True)
    # torch's kernel is [C][D][k], cross-correlation: out[o][t] = sum w[o][d][j] z[d][t + j - pl]
    out = torch.nn.functional.conv1d(z, w.permute(2, 1, 0), bias, padding=(k - 1) // 2)
    out.backward(dout)
    zn, wn, bn, gn = z.detach().numpy(), w.detach().numpy(), bias.detach().numpy(), dout.numpy()
    close(CR.fwd(zn, wn, bn), out.detach().numpy(), 'fwd')
    close(CR.dgrad(wn, gn), z.grad.numpy(), 'dgrad')
    dw, db = CR.wgrad(zn, gn, k)
    close(dw, w.grad.numpy(), 'wgrad')
    close(db, bias.grad.numpy(), 'bias gradient')


def test_shifted_pads_with_zeros_per_row():
    z = np.arange(1.0, 7.0).reshape(2, 1, 3)
    assert CR.shifted(z, 1).tolist() == [[[2, 3, 0]], [[5, 6, 0]]]
    assert CR.shifted(z, -1).tolist() == [[[0, 1, 2]], [[0, 4, 5]]]
    assert CR.shifted(z, 3).tolist() == [[[0, 0, 0]], [[0, 0, 0]]] and CR.shifted(z, 0).tolist() == z.tolist()


def test_exact_operands_stay_exact_in_fp32():
    """Every sum of absolute terms of every exact case stays below 2^24: fp32 holds each partial sum, in any order."""
    for case in CR.CASES:
        ops = CR.operands(case, 'exact')
        assert all(np.abs(a).max() <= 8 and np.array_equal(a, np.round(a)) for a in ops)
        mag = CR.results(*(np.abs(a) for a in ops))
        assert max(v.max() for v in mag.values()) < 2.0 ** 24, case


@pytest.mark.parametrize('flaw', CR.FLAWS)
def test_cases_catch_wrong_kernels(flaw):
    """A kernel with the flaw fails at least one GPU case: its exact outputs differ from the reference's somewhere, AND its
    random outputs leave the bars somewhere."""
    caught_exact, caught_random = [], []
    for case in CR.CASES:
        ops = CR.operands(case, 'exact')
        good, bad = CR.results(*ops), CR.results(*ops, flaw=flaw)
        if any(not np.array_equal(good[n], bad[n]) for n in good):
            caught_exact.append(case)
        ops = CR.operands(case, 'random')
        good, bad, bar = CR.results(*ops), CR.results(*ops, flaw=flaw), CR.bars(case, *ops)
        if any((np.abs(good[n] - bad[n]) > bar[n]).any() for n in good):
            caught_random.append(case)
    assert caught_exact and caught_random, (flaw, caught_exact, caught_random)


def test_bars_are_tight_enough_to_matter():
    """The bars are a rounding bound, not a tolerance: far below the outputs' own size at every case."""
    for case in CR.CASES:
        ops = CR.operands(case, 'random')
        good, bar = CR.results(*ops), CR.bars(case, *ops)
        for n in good:
            assert bar[n].max() < 1e-3 * max(np.abs(good[n]).max(), 1.0), (case, n)
