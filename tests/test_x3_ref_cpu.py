"""Pins tests/x3_ref.py, the CPU statement of the fp16x3 number format that test_x3_range_gpu.py holds the kernels to: if
one of these fails, a GPU failure of that module says nothing about the kernels.  No GPU, numpy only."""
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
