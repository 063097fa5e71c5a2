"""Pins tests/x3_ref.py, the CPU statement of the fp16x3 number format that test_x3_range_gpu.py holds the kernels to (and of
the bf16 engine's one-plane format, test_bf16_kernels_gpu.py): if one of these fails, a GPU failure of those modules says nothing
about the kernels.  No GPU, numpy only (torch.bfloat16 once, as a witness)."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import x3_ref as X  # noqa: E402


def spread(rng, shape, lo=-40, hi=0):
    """randn times per-element powers of two 2^lo..2^hi."""
    return (rng.standard_normal(shape) * np.exp2(rng.randint(lo, hi + 1, shape))).astype(np.float32)


def working_scale(x, target_exp=14):
    """The engine's choice: the power of two that puts max |x| into [2^(target_exp-1), 2^target_exp)."""
    s, flag = X.update_scales([X.amax_bits(x)], [1.0], target_exp)
    assert flag == 0
    return float(s[0])


def row_scaled_problem(seed=0, K=768, N=256, reps=3, kmax=40):
    """The issue's problem: a [rows][K] with row r multiplied by 2^-(r % (kmax+1)), b [K][N] plain randn."""
    rng = np.random.RandomState(seed)
    ks = np.arange(reps * (kmax + 1)) % (kmax + 1)
    a = (rng.standard_normal((len(ks), K)) * np.exp2(-ks)[:, None]).astype(np.float32)
    b = rng.standard_normal((K, N)).astype(np.float32)
    return ks, a, b


def curve_by_k(ks, err):
    return np.array([err[ks == k].mean() for k in range(ks.max() + 1)])


def test_split_reproduces_the_scaled_value():
    """h1 + h2 = x to 2^-22 relative where |x| >= 2^-3 (h1 is x to 2^-11, the residual is normal in fp16 or its absolute
    error 2^-25 is below that bar), and to 2^-25 absolute below (the residual is an fp16 subnormal: spacing 2^-24)."""
    rng = np.random.RandomState(1)
    x = np.concatenate([spread(rng, 200000, -40, 15), np.float32([65504, -65504, 65519.996, 2.0 ** -14, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25,
                                                                  0.0, -0.0, 2.0 ** -126, 1e-40, 0.125, np.nextafter(np.float32(0.125), 0)])])
    x = x[np.abs(x) < 65520]
    h1, h2 = X.split(x)
    assert np.isfinite(h1.astype(np.float64)).all() and np.isfinite(h2.astype(np.float64)).all()
    err = np.abs(h1.astype(np.float64) + h2.astype(np.float64) - x.astype(np.float64))
    big = np.abs(x) >= 2.0 ** -3
    assert big.sum() > 1000 and (~big).sum() > 1000
    assert (err[big] <= 2.0 ** -22 * np.abs(x[big].astype(np.float64))).all()
    assert (err[~big] <= 2.0 ** -25).all()
    # the planted roundings, bit for bit: ties go to even, the sign of a vanished piece is kept
    bits = lambda v: tuple(int(h.view(np.uint16)[0]) for h in X.split(np.float32([v])))
    assert bits(2.0 ** -25) == (0x0000, 0x0000)
    assert bits(3 * 2.0 ** -25) == (0x0002, 0x8000)
    assert bits(-0.0) == (0x8000, 0x0000)                      # -0 - (-0) = +0
    assert bits(65519.996) == (0x7bff, 0x4bff + 1)             # 65504 + fp16(15.996) = 16
    assert bits(2.0 ** -14) == (0x0400, 0x0000) and bits(2.0 ** -24) == (0x0001, 0x0000)
    f1, f2 = X.split(np.float32([2.0 ** -14, 2.0 ** -15, 1.0 + 2.0 ** -13 + 2.0 ** -26]), flush=True)
    assert f1.tolist() == [2.0 ** -14, 0.0, 1.0] and f2.tolist() == [0.0, 0.0, 2.0 ** -13]
    assert X.bf16_bits(np.float32([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -2.5])).tolist() == [0x3f80, 0x3f80, 0x3f82, 0xc020]


def test_contract_curves_by_distance_from_the_tensor_max():
    """Per-row relative L2 error of the three-term product against fp64, rows 2^-k below the tensor max (K = 768, operand
    max at [2^13, 2^14)).  While a row's residual plane is normal in fp16 (k <= 12: the residual is 2^-11 of the row, the
    row 2^(13-k)) nothing is lost: the curve is flat, within 2x of k = 0.  After that it can only grow (0.9: the curve is a
    mean over three rows per k).  With subnormals flushed the residual plane of such a row is gone entirely, which leaves
    2^-11 per element instead of 2^-22 -- by k = 14 the two curves are at least 100x apart, so a test can tell which one a
    device is on."""
    ks, a, b = row_scaled_problem()
    sa, sb = working_scale(a), working_scale(b)
    assert 2.0 ** 13 <= np.abs(a).max() * sa < 2.0 ** 14 and 2.0 ** 13 <= np.abs(b).max() * sb < 2.0 ** 14
    want = a.astype(np.float64) @ b.astype(np.float64)
    keep = curve_by_k(ks, X.row_rel_l2(X.contract(a, b, sa, sb), want))
    flush = curve_by_k(ks, X.row_rel_l2(X.contract(a, b, sa, sb, flush=True), want))
    print('k       ', ' '.join('%8d' % k for k in range(0, 41, 2)))
    print('kept    ', ' '.join('%8.1e' % v for v in keep[::2]))
    print('flushed ', ' '.join('%8.1e' % v for v in flush[::2]))
    assert keep[0] < 2.0 ** -22                                # the dropped a2 b2 term and two roundings of 2^-22, averaged over K
    assert (keep[:13] <= 2 * keep[0]).all() and (keep[:13] >= keep[0] / 2).all()
    assert (keep[13:] >= 0.9 * keep[12:-1]).all()
    assert flush[14] >= 100 * keep[14]
    assert (flush >= 0.9 * keep).all()
    assert (keep[:31] < 0.25).all()                            # every row the GPU test must assert carries information
    # the scales are undone: exact operands give the exact product at any scale
    e = np.float32([[1.0, 2.0, -0.5, 3.0]])
    assert X.contract(e, e.T, 2.0 ** 10, 2.0 ** -4).tolist() == [[14.25]]


def test_activation_planes_match_a_triple_loop():
    rng = np.random.RandomState(2)
    B, C, T, kc0, KC = 2, 16, 6, 1, 4
    x = spread(rng, (B, C, T), -30, 0)
    v = X.scaled(x, 8.0, 0.25)
    assert np.array_equal(v, x * np.float32(2.0))
    h = X.split(v)
    before = rng.randint(0, 65536, (2, KC, B * T, 8)).astype(np.uint16)
    want = before.copy()
    for p in range(2):
        for b in range(B):
            for c in range(C):
                for t in range(T):
                    want[p, kc0 + c // 8, b * T + t, c % 8] = h[p][b, c, t].view(np.uint16)
    got = X.act_planes(x, 8.0, 0.25, kc0, KC, into=before)
    assert np.array_equal(got, want)
    assert np.array_equal(X.act_planes(x, 2.0)[:, :, :, :], want[:, kc0:kc0 + C // 8])
    # space to depth: [plane][parity block of C/8 chunks][b T/2 + t'][8]
    want = np.zeros((2, 2 * C // 8, B * T // 2, 8), np.uint16)
    for p in range(2):
        for b in range(B):
            for c in range(C):
                for t in range(T):
                    want[p, (t % 2) * (C // 8) + c // 8, b * (T // 2) + t // 2, c % 8] = h[p][b, c, t].view(np.uint16)
    assert np.array_equal(X.act_planes(x, 8.0, 0.25, mode=X.X3_S2D), want)
    # bf16: one plane
    got = X.act_planes(x, 8.0, 0.25, mode=X.X3_BF16)
    assert got.shape == (1, C // 8, B * T, 8)
    for b in range(B):
        for c in range(C):
            for t in range(T):
                assert got[0, c // 8, b * T + t, c % 8] == X.bf16_bits(v[b, c, t:t + 1])[0]


def test_weight_planes_match_a_triple_loop():
    rng = np.random.RandomState(3)
    K, M, ldw, cnt = 16, 5, 7, 2
    w = spread(rng, (cnt, K, ldw), -30, 0)
    h = X.split(X.scaled(w, 4.0, 0.5))
    want = np.zeros((cnt, 2, K // 8, M, 8), np.uint16)
    for i in range(cnt):
        for p in range(2):
            for k in range(K):
                for m in range(M):
                    want[i, p, k // 8, m, k % 8] = h[p][i, k, m].view(np.uint16)
    assert np.array_equal(X.pack_weights(w, K, M, 4.0, 0.5), want)
    # transposed storage: k = jb * k_inner + ko is src[i * (K / k_inner) * blk_stride + jb * blk_stride + m * ld_src + ko]
    k_inner, ld_src, blk = 8, 12, 40
    M = 3
    src = spread(rng, cnt * (K // k_inner) * blk, -30, 0)
    h = X.split(X.scaled(src, 4.0, 0.5))
    want = np.zeros((cnt, 2, K // 8, M, 8), np.uint16)
    for i in range(cnt):
        for p in range(2):
            for k in range(K):
                for m in range(M):
                    j = i * (K // k_inner) * blk + (k // k_inner) * blk + m * ld_src + k % k_inner
                    want[i, p, k // 8, m, k % 8] = h[p][j].view(np.uint16)
    assert np.array_equal(X.pack_weights_t(src, K, M, k_inner, ld_src, blk, 4.0, cnt, 0.5), want)


@pytest.mark.parametrize('mode,hb', [(0, 256), (X.X3_HALF_BLOCKS, 128)])
def test_gate_weight_planes_match_a_triple_loop(mode, hb):
    """Rows in block order: every block of hb rows holds hb/2 filter channels, then the hb/2 matching gate channels."""
    rng = np.random.RandomState(4)
    ks, R, ldw, cnt = 2, 128, 2 * 128 + 4, 2
    w = spread(rng, (cnt, ks, R, ldw), -30, 0)
    order = []
    for blk in range(2 * R // hb):
        chans = range(blk * hb // 2, (blk + 1) * hb // 2)
        order += [c for c in chans] + [R + c for c in chans]
    assert sorted(order) == list(range(2 * R)) and order == X.gate_row_order(R, mode).tolist()
    h = X.split(X.scaled(w, 256.0, 2.0))
    want = np.zeros((cnt, 2, ks * R // 8, 2 * R, 8), np.uint16)
    for i in range(cnt):
        for p in range(2):
            for j in range(ks):
                for c in range(R):
                    k = j * R + c
                    want[i, p, k // 8, :, k % 8] = h[p][i, j, c, order].view(np.uint16)
    assert np.array_equal(X.pack_gate_weights(w, ks, R, 256.0, 2.0, mode), want)


def test_update_scales_every_exponent_and_target():
    amax = X.exponent_sweep()
    f = amax.view(np.float32).astype(np.float64)
    assert f.min() == 2.0 ** -149 and np.isfinite(f).all()
    for te in range(1, 16):
        s, flag = X.update_scales(amax, np.full(len(amax), 3.0, np.float32), te)
        assert flag == 0
        s64 = s.astype(np.float64)
        man, ex = np.frexp(s64)
        assert (man == 0.5).all(), 'a scale that is not a power of two'
        k = ex - 1
        assert (np.abs(k) <= X.SCALE_EXP_CLAMP).all()
        inside = (f * s64 >= 2.0 ** (te - 1)) & (f * s64 < 2.0 ** te)
        free = (f >= 2.0 ** (te - 101)) & (f < 2.0 ** (te + 100))      # the header's clamp at 2^+-100
        assert inside[free].all() and free.sum() > 700
        assert (k[f < 2.0 ** (te - 101)] == 100).all() and (k[f >= 2.0 ** (te + 100)] == -100).all()
        assert not inside[~free].any()
    s, flag = X.update_scales([0, 0, 0x7f800000, 0x7fc00000, 0x3f800000], np.float32([5.0, 0.0, 7.0, 7.0, 7.0]), 14)
    assert s.tolist() == [5.0, 1.0, 7.0, 7.0, 8192.0] and flag == 1
    assert X.amax_bits(np.float32([[0.5, -3.0], [2.0, -0.0]])) == 0x40400000
    assert math.ldexp(1.0, 13) * 1.0 == 8192.0


# ----------------------------------------------------------------------------- the bf16 engine's reference
def test_bf16_round_is_the_value_of_bf16_bits():
    """bf16_round against bf16_bits bit for bit, planted ties (to even, both ways), negative values, values that round up
    across a power of two, and torch.bfloat16 as a witness that shares no code with either."""
    import torch
    rng = np.random.RandomState(5)
    one = np.float32(1.0)
    planted = np.float32([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), -(1.0 + 3 * 2.0 ** -8),       # ties: down to even, up to even
                          2.0 - 2.0 ** -8, -(2.0 - 2.0 ** -8), 2.0 - 2.0 ** -9, np.nextafter(np.float32(2.0), one),  # up across a power of two
                          1.0 + 2.0 ** -8 + 2.0 ** -23, 1.0 + 2.0 ** -8 - 2.0 ** -16, 0.0, -0.0, 2.0 ** -126, -2.5, 3.0e38, 2.0 ** -130])
    want = np.float64([1.0, 1.0 + 2.0 ** -6, -1.0, -(1.0 + 2.0 ** -6), 2.0, -2.0, 2.0, 2.0,
                       1.0 + 2.0 ** -7, 1.0, 0.0, -0.0, 2.0 ** -126, -2.5, 0, 2.0 ** -130])
    got = X.bf16_round(planted)
    keep = np.arange(len(planted)) != 14
    assert np.array_equal(got[keep], want[keep]) and np.array_equal(np.signbit(got), np.signbit(planted))
    x = np.concatenate([spread(rng, 300000, -60, 60), planted])
    r = X.bf16_round(x)
    assert r.dtype == np.float64 and r.shape == x.shape
    r32 = r.astype(np.float32)
    assert np.array_equal(r32.astype(np.float64), r), 'a bf16 value that is no float32'
    assert np.array_equal(r32.view(np.uint32), X.bf16_bits(x).astype(np.uint32) << 16)
    assert (np.abs(r - x.astype(np.float64)) <= 2.0 ** -8 * np.abs(x.astype(np.float64))).all()      # half an ulp (2^-7) of 8 significand bits
    assert np.array_equal(X.bf16_round(r32), r), 'rounding is not idempotent'
    witness = torch.from_numpy(x).to(torch.bfloat16).to(torch.float64).numpy()
    assert np.array_equal(witness, r)
    assert X.bf16_round(x.reshape(4, -1)).shape == (4, x.size // 4)
    # truncation (the wrong conversion the GPU tests must catch) differs from it exactly where the dropped bits are more than half
    t = X.bf16_truncate(x)
    assert (np.abs(t) <= np.abs(x.astype(np.float64))).all() and 0.4 < (t != r).mean() < 0.6
    # exact operands give the exact product at any scale, and rounding happens AFTER the scale
    e = np.float32([[1.0, 2.0, -0.5, 3.0]])
    assert X.contract_bf16(e, e.T, 2.0 ** 10, 2.0 ** -4).tolist() == [[14.25]]
    a = np.float32([[1.0 + 2.0 ** -8 + 2.0 ** -20]])
    assert X.contract_bf16(a, np.float32([[3.0]])).tolist() == [[3.0 * (1.0 + 2.0 ** -7)]]


def _wrong_variants():
    return (('operands truncated, not rounded to nearest even', dict(rnd=X.bf16_truncate)),
            ('tap 0 not zeroed before the start of the batch row', dict(leak_tap=0)),
            ('operands left unrounded', dict(rnd=X.unrounded)))


def test_gate_bar_tells_a_wrong_bf16_kernel_from_a_right_one():
    """The gate conv's bar in test_bf16_kernels_gpu.py (2e-5 absolute on tanh * sigmoid, tanh and sigmoid) at its case
    (B=2, T=512, R=128, ks=3, d=7): every deliberately wrong evaluation lies at least 10 bars from the reference in the output
    the GPU test compares, so a kernel inside the bar made none of these mistakes."""
    B, T, R, ks, d = 2, 512, 128, 3, 7
    bar = 2e-5
    x, w, bias, cond = X.gate_case(B, T, R, ks, d)
    taps = [-(ks - 1 - j) * d for j in range(ks)]
    want = X.gate_outputs(X.conv_bf16(x, w, taps, 1.0, 256.0), bias, cond, T)
    for what, kw in _wrong_variants():
        got = X.gate_outputs(X.conv_bf16(x, w, taps, 1.0, 256.0, **kw), bias, cond, T)
        dist = [float(np.abs(g_ - w_).max()) for g_, w_ in zip(got, want)]
        print('%-52s gated %.2e tanh %.2e sigmoid %.2e (bar %.0e)' % (what, dist[0], dist[1], dist[2], bar))
        assert min(dist) >= 10 * bar, (what, dist)
    # the leaked tap is wrong ONLY in the first 2 d steps of the rows behind the first: a test that samples must sample there
    got = X.gate_outputs(X.conv_bf16(x, w, taps, 1.0, 256.0, leak_tap=0), bias, cond, T)[0]
    assert np.array_equal(got[0], want[0][0]) and np.array_equal(got[1][:, 2 * d:], want[0][1][:, 2 * d:])


def test_wgrad_bar_tells_a_wrong_bf16_kernel_from_a_right_one():
    """The weight gradient's bar (2e-6 of the largest update + 1e-6 of the largest dw accumulated into) at its case
    (B=2, T=512, d=1, Cp=256, Q=512+256): each wrong evaluation is at least 10 bars away."""
    B, T, d, Q1 = 2, 512, 1, 256
    p, q0, q1, dw0, sc = X.wgrad_case(B, T, d, Q1, False)
    q = np.concatenate([q0, q1], 1)
    taps = [-2 * d, -d, 0]
    want = X.wgrad_bf16(p, q, taps)
    bar = 2e-6 * float(np.abs(want).max()) + 1e-6 * float(np.abs(dw0).max())
    for what, kw in _wrong_variants():
        dist = float(np.abs(X.wgrad_bf16(p, q, taps, **kw) - want).max())
        print('%-52s %.2e (bar %.2e)' % (what, dist, bar))
        assert dist >= 10 * bar, (what, dist, bar)
    leak = X.wgrad_bf16(p, q, taps, leak_tap=0)
    assert np.array_equal(leak[1:], want[1:]) and not np.array_equal(leak[0], want[0])
