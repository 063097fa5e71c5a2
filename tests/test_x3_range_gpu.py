"""The fp16x3 engine's planes, range guards and dynamic range on the GPU against tests/x3_ref.py (pinned by test_x3_ref_cpu.py).

(a) the plane images the split / pack kernels write, bit for bit against the header's statement of the format, on operands that
    span 2^-40..2^0 per element with the edges of fp16 planted;
(b) the guards: max-abs slots, the range flag at its exact edge, the scale update over every exponent, the skip guards;
(c) the per-row relative error of every contraction kernel when the rows of one operand lie 2^-k below the tensor max, held to
    the best the two-plane format can do (x3_ref.contract, fp64 sums) plus the cost of fp32 accumulation.

No bar in this module comes from a kernel's output: they are bit equality, the CPU model and a CPU float32 evaluation."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import x3_ref as X  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BF, HALF, S2D = X.X3_BF16, X.X3_HALF_BLOCKS, X.X3_S2D
KMAX = 40


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def slot(v):
    return torch.tensor([v], dtype=torch.float32, device=DEV)


def izeros(n=1, v=0):
    return torch.full((n,), v, dtype=torch.int32, device=DEV)


def halves(n=None, image=None):
    """A float16 device buffer: n halves of a poison pattern, or the given uint16 image."""
    if image is None:
        image = np.full(n, 0x7e55, np.uint16)
    return dev(image.reshape(-1).view(np.int16)).view(torch.float16)


def image_of(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def f32_bits(v):
    return int(np.float32(v).view(np.uint32))


# the edges of the plane format, as values of scale * x
EDGES = np.float32([65504.0, -65504.0, np.nextafter(np.float32(65520.0), np.float32(0)), 0.0, -0.0, 2.0 ** -14, -2.0 ** -14, 2.0 ** -24,
                    2.0 ** -25, 3 * 2.0 ** -25, -3 * 2.0 ** -25, 2.0 ** -126, 2.0 ** -140, -2.0 ** -140])


def ranged(rng, shape, sc):
    """randn times per-element powers of two 2^-40..2^0, with EDGES / sc planted (sc a power of two: exact) at random places."""
    x = (rng.standard_normal(shape) * np.exp2(rng.randint(-40, 1, shape))).astype(np.float32)
    flat = x.reshape(-1)
    pos = rng.choice(flat.size, 3 * len(EDGES), replace=False)
    planted = (np.tile(EDGES, 3).astype(np.float64) / sc).astype(np.float32)
    assert np.array_equal(planted.astype(np.float64) * sc, np.tile(EDGES, 3).astype(np.float64))
    flat[pos] = planted
    return x


# ----------------------------------------------------------------------------- (a) plane bytes
@pytest.mark.parametrize('mode', [0, BF, S2D, S2D | BF], ids=['f16', 'bf16', 's2d', 's2d_bf16'])
def test_split_activations_plane_bytes(K, mode):
    """vqw_f16x3_split_activations: the whole device buffer equals the reference image (halves beyond the planes written stay as they were)."""
    rng = np.random.RandomState(10 + mode)
    B, C, T = 3, 40, 130
    scale, sdev = 8.0, 0.25
    x = ranged(rng, (B, C, T), scale * sdev)
    buf = halves(2 * B * C * T + 64)
    K.f16x3_split_activations(dev(x), buf, B, C, T, scale=scale, scale_dev=slot(sdev), mode=mode)
    want = X.act_planes(x, scale, sdev, mode=mode).reshape(-1)
    got = image_of(buf)
    assert np.array_equal(got[:want.size], want), '%d halves differ' % int((got[:want.size] != want).sum())
    assert (got[want.size:] == 0x7e55).all(), 'wrote past the planes'


@pytest.mark.parametrize('mode', [0, BF], ids=['f16', 'bf16'])
def test_split_activations_into_a_wider_buffer(K, mode):
    """kc0 / KC: this tensor's chunks land at kc0.. of both planes of a buffer of KC chunks; every other chunk keeps its bits."""
    rng = np.random.RandomState(20 + mode)
    B, C, T, kc0, KC = 2, 24, 100, 2, 7
    scale, sdev = 0.5, 4.0
    x = ranged(rng, (B, C, T), scale * sdev)
    before = rng.randint(0, 65536, (2, KC, B * T, 8)).astype(np.uint16)
    buf = halves(image=before)
    K.f16x3_split_activations(dev(x), buf, B, C, T, scale=scale, kc0=kc0, KC=KC, scale_dev=slot(sdev), mode=mode)
    P = 1 if mode & BF else 2
    want = before.copy()
    want[:P] = X.act_planes(x, scale, sdev, kc0, KC, mode=mode, into=before[:P])
    assert np.array_equal(image_of(buf).reshape(want.shape), want)


@pytest.mark.parametrize('mode', [0, BF], ids=['f16', 'bf16'])
def test_pack_weights_plane_bytes(K, mode):
    rng = np.random.RandomState(30 + mode)
    Kd, M, ldw, cnt = 40, 37, 45, 3
    scale, sdev = 4.0, 0.5
    w = ranged(rng, (cnt, Kd, ldw), scale * sdev)
    buf = halves(cnt * 2 * Kd * M + 64)
    K.f16x3_pack_weights(dev(w), buf, Kd, M, ldw, scale, count=cnt, scale_dev=slot(sdev), mode=mode)
    want = X.pack_weights(w, Kd, M, scale, sdev, mode)
    got = image_of(buf)[:cnt * 2 * Kd * M].reshape(cnt, 2, Kd // 8, M, 8)
    P = want.shape[1]
    assert np.array_equal(got[:, :P], want)
    if P == 1:
        assert (got[:, 1] == 0x7e55).all()
    assert (image_of(buf)[cnt * 2 * Kd * M:] == 0x7e55).all()


@pytest.mark.parametrize('mode', [0, BF], ids=['f16', 'bf16'])
@pytest.mark.parametrize('Kd,M,k_inner,ld_src,pad', [(80, 72, 40, 44, 8), (128, 72, 64, 68, 4), (192, 130, 64, 64, 0)],
                         ids=['direct', 'tile', 'tile_dense'])
def test_pack_weights_t_plane_bytes(K, mode, Kd, M, k_inner, ld_src, pad):
    """vqw_f16x3_pack_weights_t: the direct kernel (k_inner % 64 != 0) and the LDS-transposing one (k_inner % 64 == 0) with
    M % 64 != 0, ld_src > k_inner, blocks further apart than they are long, two matrices per launch."""
    rng = np.random.RandomState(40 + mode + Kd)
    cnt, blk = 2, M * ld_src + pad
    scale, sdev = 2.0, 4.0
    src = ranged(rng, cnt * (Kd // k_inner) * blk, scale * sdev)
    buf = halves(cnt * 2 * Kd * M + 64)
    K.f16x3_pack_weights_t(dev(src), buf, Kd, M, k_inner, ld_src, blk, scale, count=cnt, scale_dev=slot(sdev), mode=mode)
    want = X.pack_weights_t(src, Kd, M, k_inner, ld_src, blk, scale, cnt, sdev, mode)
    got = image_of(buf)[:cnt * 2 * Kd * M].reshape(cnt, 2, Kd // 8, M, 8)
    P = want.shape[1]
    assert np.array_equal(got[:, :P], want), '%d halves differ' % int((got[:, :P] != want).sum())
    if P == 1:
        assert (got[:, 1] == 0x7e55).all()
    assert (image_of(buf)[cnt * 2 * Kd * M:] == 0x7e55).all()


@pytest.mark.parametrize('mode', [0, HALF, BF, HALF | BF], ids=['blocks256', 'blocks128', 'blocks256_bf16', 'blocks128_bf16'])
def test_pack_gate_weights_plane_bytes(K, mode):
    rng = np.random.RandomState(50 + mode)
    ks, R, cnt = 2, 256, 2
    ldw = 2 * R + 4
    scale, sdev = 256.0, 2.0 ** -5
    w = ranged(rng, (cnt, ks, R, ldw), scale * sdev)
    n = cnt * 2 * ks * R * 2 * R
    buf = halves(n + 64)
    K.f16x3_pack_gate_weights(dev(w), buf, ks, R, ldw, scale, count=cnt, scale_dev=slot(sdev), mode=mode)
    want = X.pack_gate_weights(w, ks, R, scale, sdev, mode)
    got = image_of(buf)[:n].reshape(cnt, 2, ks * R // 8, 2 * R, 8)
    P = want.shape[1]
    assert np.array_equal(got[:, :P], want), '%d halves differ' % int((got[:, :P] != want).sum())
    assert (image_of(buf)[n:] == 0x7e55).all()


# ----------------------------------------------------------------------------- (b) guards
@pytest.mark.parametrize('where', ['first_block', 'last_block'])
def test_split_activations_amax_and_range_flag(K, where):
    """amax is the running max of the UNSCALED |x|, exactly; the flag stays 0 with the max exactly at 65504 / s and rises with
    one element at the next fp32 above it, with one inf, with one NaN, in the first and in the last block of the grid; the other bits of
    the flag word are kept."""
    rng = np.random.RandomState(60)
    B, C, T = 2, 16, 4096                                   # 16384 threads: 64 blocks of 256
    scale, sdev = 8.0, 0.25
    s = scale * sdev
    x = (rng.standard_normal((B, C, T)) * 100).astype(np.float32)
    idx = (0, 0, 0) if where == 'first_block' else (B - 1, C - 1, T - 1)
    edge = np.float32(65504.0 / s)
    buf = halves(2 * B * C * T)

    def run(v, amax0=0, flag0=0):
        xx = x.copy()
        xx[idx] = v
        amax, flag = izeros(1, amax0), izeros(1, flag0)
        K.f16x3_split_activations(dev(xx), buf, B, C, T, scale=scale, scale_dev=slot(sdev), amax=amax, flag=flag)
        return xx, int(amax.item()), int(flag.item())

    for v in (edge, -edge):
        xx, a, f = run(v)
        assert a == X.amax_bits(xx) == f32_bits(edge) and f == 0
    xx, a, f = run(edge, amax0=f32_bits(1.0), flag0=6)
    assert a == f32_bits(edge) and f == 6
    xx, a, f = run(edge, amax0=f32_bits(1.0e6))
    assert a == f32_bits(1.0e6) and f == 0, 'amax is not a running max'
    over = np.nextafter(edge, np.float32(np.inf))
    for v in (over, -over):
        xx, a, f = run(v, flag0=6)
        assert a == f32_bits(over) and f == 7
    assert run(np.float32(np.inf))[2] == 1 and run(np.float32(-np.inf), flag0=4)[2] == 5
    assert run(np.float32(np.nan))[2] == 1
    xx, a, f = run(np.float32(1.0))                          # nothing planted: the plain max of the tensor
    assert a == X.amax_bits(xx) and f == 0


def test_amax_every_path(K):
    """vqw_f16x3_amax: the 16-byte path with its unrolled loop and its tail (more than 8 * 512 * 256 * 4 floats), the scalar path
    (n % 4 != 0, a base pointer off by one float, ld > cols, a matrix stride that is not a multiple of 4); the maximum at the first,
    the last, an unrolled-loop and a tail element, of either sign; padding between rows and matrices is not read; inf / NaN."""
    rng = np.random.RandomState(70)
    nthr = 512 * 256
    n = 8 * nthr * 4 + 4 * 12345
    base = rng.standard_normal(n).astype(np.float32)
    bd = dev(base)
    top = X.amax_bits(base)
    amax, flag = izeros(), izeros()
    K.f16x3_amax(bd, amax, flag=flag)
    assert int(amax.item()) == top and int(flag.item()) == 0
    for pos in (0, n - 1, 4 * (3 * nthr + 77) + 1, 4 * (8 * nthr + 5000) + 2, 4 * (8 * nthr) + 3):
        for v in (1234.5, -4321.0):
            xd = bd.clone()
            xd[pos] = v
            amax = izeros(1, f32_bits(2.0))
            K.f16x3_amax(xd, amax, flag=flag)
            assert int(amax.item()) == f32_bits(abs(v)), 'maximum %g at %d missed' % (v, pos)
    assert int(flag.item()) == 0
    amax = izeros(1, f32_bits(1.0e6))
    K.f16x3_amax(bd, amax)
    assert int(amax.item()) == f32_bits(1.0e6), 'amax is not a running max'
    # scalar paths
    for off, ln in ((0, 1000003), (1, 1000000)):
        for pos in (0, ln - 1, 500001):
            v = bd.clone()[off:off + ln]
            v[pos] = -777.25
            amax = izeros()
            K.f16x3_amax(v, amax, flag=flag)
            assert int(amax.item()) == f32_bits(777.25)
        amax = izeros()
        K.f16x3_amax(bd.clone()[off:off + ln], amax)
        assert int(amax.item()) == X.amax_bits(base[off:off + ln])
    # ld > cols: what lies between the rows is not read
    rows, cols, ld = 37, 50, 64
    m = np.full((rows, ld), 1.0e9, np.float32)
    m[:, :cols] = rng.standard_normal((rows, cols))
    m[rows - 1, cols - 1] = -9.5
    amax = izeros()
    K.f16x3_amax(dev(m), amax, rows=rows, cols=cols, ld=ld, flag=flag)
    assert int(amax.item()) == f32_bits(9.5) == X.amax_bits(m[:, :cols])
    # three matrices 131 floats apart: the first on the 16-byte path, the others not
    rows, cols, mstride, cnt = 8, 16, 131, 3
    m = np.full(cnt * mstride, 1.0e9, np.float32)
    want = []
    for i in range(cnt):
        blk = rng.standard_normal(rows * cols).astype(np.float32) * (i + 1)
        blk[(rows * cols - 1) if i != 1 else 0] = -(20.0 + i)
        m[i * mstride:i * mstride + rows * cols] = blk
        want.append(X.amax_bits(blk))
    amax = izeros(cnt)
    K.f16x3_amax(dev(m), amax, rows=rows, cols=cols, ld=cols, mstride=mstride, count=cnt, flag=flag)
    assert amax.tolist() == want == [f32_bits(20.0 + i) for i in range(cnt)]
    assert int(flag.item()) == 0
    # inf / NaN on both paths; the other bits of the flag word are kept
    for off in (0, 1):
        for bad in (np.inf, -np.inf, np.nan):
            for pos in (0, 4095 - off):
                xd = bd[:4096].clone()[off:]
                xd[pos] = bad
                fl = izeros(1, 4)
                K.f16x3_amax(xd, izeros(), flag=fl)
                assert int(fl.item()) == 5, '%r at %d raised no flag' % (bad, pos)
    xd = bd.clone()
    xd[4 * (8 * nthr + 100)] = np.nan
    fl = izeros()
    K.f16x3_amax(xd, izeros(), flag=fl)
    assert int(fl.item()) == 1


def test_update_scales_every_exponent_skip_and_reset(K):
    """vqw_f16x3_update_scales(_guarded) equals x3_ref.update_scales for every fp32 exponent of amax and every target exponent;
    reset zeroes amax (and only then); with *skip != 0 scale, amax and flag keep their bits."""
    sweep = X.exponent_sweep()
    amax_np = np.concatenate([sweep, np.uint32([0, 0])])
    scale0 = np.full(len(amax_np), 3.0, np.float32)
    scale0[-1] = 0.0
    for te in range(1, 16):
        amax, scale, flag = dev(amax_np.view(np.int32)), dev(scale0), izeros(1, 4)
        K.f16x3_update_scales(amax, scale, target_exp=te, reset=(te % 2 == 1), flag=flag)
        want, wflag = X.update_scales(amax_np, scale0, te)
        assert wflag == 0 and int(flag.item()) == 4
        assert np.array_equal(scale.cpu().numpy().view(np.uint32), want.view(np.uint32)), 'target_exp %d' % te
        assert np.array_equal(amax.cpu().numpy().view(np.uint32), amax_np * np.uint32(te % 2 == 0))
    bad = np.uint32([0x7f800000, 0x7fc00000, 0x3f800000, 0x7f800001])
    for i in (0, 1, 3):
        amax, scale, flag = dev(bad[[2, i]].view(np.int32)), dev(np.float32([5.0, 7.0])), izeros(1, 2)
        K.f16x3_update_scales(amax, scale, target_exp=14, reset=False, flag=flag)
        want, wflag = X.update_scales(bad[[2, i]], np.float32([5.0, 7.0]), 14)
        assert wflag == 1 and int(flag.item()) == 3 and scale.tolist() == want.tolist() == [8192.0, 7.0]
    # the device-side guard
    for reset in (False, True):
        amax_bad = np.concatenate([amax_np, bad[:1]])
        sc_np = np.concatenate([scale0, np.float32([2.0])])
        amax, scale, flag = dev(amax_bad.view(np.int32)), dev(sc_np), izeros(1, 4)
        K.f16x3_update_scales(amax, scale, target_exp=14, reset=reset, flag=flag, skip=izeros(1, 1))
        assert np.array_equal(amax.cpu().numpy().view(np.uint32), amax_bad), 'a skipped update touched amax'
        assert np.array_equal(scale.cpu().numpy().view(np.uint32), sc_np.view(np.uint32)), 'a skipped update touched the scales'
        assert int(flag.item()) == 4
        K.f16x3_update_scales(amax, scale, target_exp=14, reset=reset, flag=flag, skip=izeros(1, 0))
        want, wflag = X.update_scales(amax_bad, sc_np, 14)
        assert np.array_equal(scale.cpu().numpy().view(np.uint32), want.view(np.uint32)) and int(flag.item()) == 5


def test_adam_ema_step_skip_guard(K):
    """vqw_adam_ema_step_guarded: *skip != 0 leaves param, m, v, ema bit-unchanged; *skip == 0 equals the unguarded call."""
    gen = torch.Generator().manual_seed(80)
    n = 100003
    state0 = [torch.randn(n, generator=gen).to(DEV) for _ in range(4)]
    state0[2] = state0[2].abs() * 1e-3                                   # v >= 0
    grad = (torch.randn(n, generator=gen) * 1e-2).to(DEV)

    def run(skip):
        st = [t.clone() for t in state0]
        K.adam_ema_step(st[0], grad, st[1], st[2], st[3], lr_t=1e-3, grad_scale=0.5, skip=skip)
        return st
    plain = run(None)
    assert not any(torch.equal(a, b) for a, b in zip(plain, state0))
    for a, b in zip(run(izeros(1, 0)), plain):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    for sk in (1, -1, 1 << 20):
        for a, b in zip(run(izeros(1, sk)), state0):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), 'a skipped step changed the state'


@pytest.mark.parametrize('mode', [0, HALF], ids=['blocks256', 'blocks128'])
def test_out_conv_range_flag_edge(K, mode):
    """vqw_f16x3_out_conv: the flag rises when one output exceeds 65504 / (plane_scale * out_scale) and stays 0 exactly at it.  The
    input is zero but for one channel at one time step and the weight zero but for one entry, both pieces of which are exact in
    fp16, so the output is that entry exactly; out_amax is its bit pattern."""
    B, T, R = 2, 512, 256
    b0, c0, t0, m0 = 1, 77, 300, 201
    plane_scale, out_scale = 4.0, 0.5
    edge = np.float32(65504.0 / (plane_scale * out_scale))
    x = np.zeros((B, R, T), np.float32)
    x[b0, c0, t0] = 1.0
    xp, wp = halves(2 * B * R * T), halves(2 * R * R)
    K.f16x3_split_activations(dev(x), xp, B, R, T, mode=mode)
    for v, raised in ((edge, 0), (-edge, 0), (np.nextafter(edge, np.float32(np.inf)), 1), (-np.nextafter(edge, np.float32(np.inf)), 1)):
        w = np.zeros((R, R), np.float32)
        w[c0, m0] = v
        h1, h2 = X.split(w[c0, m0:m0 + 1])
        assert float(h1[0]) + float(h2[0]) == float(v) and (h2[0] == 0 or abs(float(h2[0])) >= X.F16_MIN_NORMAL)
        K.f16x3_pack_weights(dev(w), wp, R, R, R, 1.0, mode=mode)
        out = torch.full((B, R, T), float('nan'), device=DEV)
        planes = halves(2 * B * R * T)
        amax, flag = izeros(), izeros(1, 4)
        K.f16x3_out_conv(xp=xp, wp=wp, net_out=out, net_out_planes=planes, B=B, T=T, R=R, S=0, w_scale_inv=1.0, plane_scale=plane_scale,
                         out_scale=slot(out_scale), out_amax=amax, flag=flag, mode=mode)
        want = np.zeros((B, R, T), np.float32)
        want[b0, m0, t0] = v
        assert np.array_equal(out.cpu().numpy(), want)
        assert int(amax.item()) == f32_bits(abs(v))
        assert int(flag.item()) == 4 + raised, 'output %r: flag %d' % (v, int(flag.item()))


# ----------------------------------------------------------------------------- (c) the dynamic-range curve
CURVES = {}


def working_scale(x, target_exp=14):
    """The engine's working point: the power of two that puts max |x| into [2^13, 2^14) (x3_ref.update_scales)."""
    s, flag = X.update_scales([X.amax_bits(x)], [1.0], target_exp)
    assert flag == 0 and 2.0 ** (target_exp - 1) <= float(np.abs(x).max()) * float(s[0]) < 2.0 ** target_exp
    return float(s[0])


def check_curve(name, got, a, b, sa, sb, ks, post=None, post32=None):
    """Rows of got [rows][n] = a [rows][K] b [K][n] on the GPU, row r of `a` lying 2^-ks[r] below the tensor max:
        err_gpu(row) <= 4 * err_model(row) + floor(row)
    err_*: relative L2 over the row against fp64 on the same fp32 inputs; err_model: x3_ref.contract (the format with fp64 sums);
    floor: 4 x the error of a CPU float32 evaluation (the cost of fp32 accumulation).  Rows whose err_model exceeds 0.25 carry
    no information and are left out; every row with k <= 30 is asserted.  post / post32: what the kernel applies behind the contraction."""
    post = post or (lambda z: z)
    post32 = post32 or (lambda z: z)
    want = post((torch.from_numpy(a).double() @ torch.from_numpy(b).double()).numpy())
    e_gpu = X.row_rel_l2(got, want)
    e_model = X.row_rel_l2(post(X.contract(a, b, sa, sb)), want)
    e_flush = X.row_rel_l2(post(X.contract(a, b, sa, sb, flush=True)), want)
    floor = 4 * X.row_rel_l2(post32(a @ b), want)
    by_k = lambda e: [float(e[ks == k].mean()) for k in range(KMAX + 1)]
    CURVES[name] = dict(k=list(range(KMAX + 1)), gpu=by_k(e_gpu), model=by_k(e_model), flush_model=by_k(e_flush), floor=by_k(floor))
    print('\n%s: mean relative L2 error of the rows 2^-k below the tensor max' % name)
    print('   k      gpu    model    flush    floor')
    for k in range(KMAX + 1):
        c = CURVES[name]
        print('  %2d  %.1e  %.1e  %.1e  %.1e' % (k, c['gpu'][k], c['model'][k], c['flush_model'][k], c['floor'][k]))
    path = os.environ.get('VQW_X3_CURVE_OUT')
    if path:
        with open(path, 'w') as f:
            json.dump(dict(what='relative L2 error per row, mean over the rows 2^-k below the tensor max (operand max scaled to [2^13, 2^14)): '
                                'gpu = the kernel, model / flush_model = tests/x3_ref.py contract() with fp16 subnormals kept / flushed, '
                                'floor = 4 x a CPU float32 evaluation; all against fp64', curves=CURVES), f, indent=1)
    live = e_model <= 0.25
    assert live[ks <= 30].all(), 'the reference itself loses rows with k <= 30'
    bar = 4 * e_model + floor
    worst = np.argmax(np.where(live, e_gpu / bar, 0))
    assert (e_gpu[live] <= bar[live]).all(), '%s: %d rows above the bar; worst k = %d: gpu %.3e, model %.3e, flush model %.3e, floor %.3e' % (
        name, int((e_gpu[live] > bar[live]).sum()), ks[worst], e_gpu[worst], e_model[worst], e_flush[worst], floor[worst])


def k_cycle(n):
    return np.arange(n) % (KMAX + 1)


def k_runs(B, T, run=12):
    """k per (b, t): runs of `run` equal values, so that the taps of a short conv mostly meet one k."""
    return np.tile((np.arange(T) // run) % (KMAX + 1), B)


@pytest.mark.parametrize('mode', [0, HALF], ids=['blocks256', 'blocks128'])
@pytest.mark.parametrize('which', ['weight_channels', 'time_steps'])
def test_range_curve_out_conv_1x1(K, mode, which):
    """The 1x1 skip conv (S = 512 skip rows from zero, no bias): weight output channels, then activation time steps, 2^-k down."""
    rng = np.random.RandomState(100)
    B, T, Cin, S = 2, 512, 256, 512
    x = rng.standard_normal((B, Cin, T)).astype(np.float32)
    w = (rng.standard_normal((Cin, S)) * 0.05).astype(np.float32)
    if which == 'weight_channels':
        ks = k_cycle(S)
        w *= np.exp2(-ks).astype(np.float32)[None, :]
    else:
        ks = k_cycle(B * T)
        x *= np.exp2(-ks).astype(np.float32).reshape(B, 1, T)
    sx, sw = working_scale(x), working_scale(w)
    xp, wp = halves(2 * B * Cin * T), halves(2 * Cin * S)
    sxd, swd = slot(sx), slot(sw)
    K.f16x3_split_activations(dev(x), xp, B, Cin, T, scale_dev=sxd, mode=mode)
    K.f16x3_pack_weights(dev(w), wp, Cin, S, S, 1.0, scale_dev=swd, mode=mode)
    skip = torch.zeros(B, S, T, device=DEV)
    K.f16x3_out_conv(xp=xp, wp=wp, skip=skip, B=B, T=T, R=0, S=S, Cin=Cin, w_scale_inv=1.0, x_scale=sxd, w_scale=swd, mode=mode)
    got = skip.cpu().numpy().transpose(1, 0, 2).reshape(S, B * T)
    xm = x.transpose(1, 0, 2).reshape(Cin, B * T)
    name = 'out_conv_1x1/%s/%s' % (which, 'blocks128' if mode else 'blocks256')
    if which == 'weight_channels':
        check_curve(name, got, np.ascontiguousarray(w.T), xm, sw, sx, ks)
    else:
        check_curve(name, np.ascontiguousarray(got.T), np.ascontiguousarray(xm.T), w, sx, sw, ks)


@pytest.mark.parametrize('mode', [0, HALF], ids=['blocks256', 'blocks128'])
@pytest.mark.parametrize('which', ['time_steps', 'weight_channels'])
def test_range_curve_input_gradient(K, mode, which):
    """The gate conv's input gradient (direction -1, three taps, reads ahead and zero behind the end of a batch row) from dpre
    planes: dpre time steps, then weight output channels, 2^-k down."""
    rng = np.random.RandomState(110)
    B, T, R, ksz, d = 2, 512, 256, 3, 1
    Cin = 2 * R
    dpre = (rng.standard_normal((B, Cin, T)) * 1e-5).astype(np.float32)
    wt = (rng.standard_normal((ksz, Cin, R)) * 0.05).astype(np.float32)
    if which == 'time_steps':
        ks = k_runs(B, T)
        dpre *= np.exp2(-ks).astype(np.float32).reshape(B, 1, T)
    else:
        ks = k_cycle(R)
        wt *= np.exp2(-ks).astype(np.float32)[None, None, :]
    sx, sw = working_scale(dpre), working_scale(wt)
    xp, wp = halves(2 * B * Cin * T), halves(2 * ksz * Cin * R)
    sxd, swd = slot(sx), slot(sw)
    K.f16x3_split_activations(dev(dpre), xp, B, Cin, T, scale_dev=sxd, mode=mode)
    K.f16x3_pack_weights(dev(wt), wp, ksz * Cin, R, R, 1.0, scale_dev=swd, mode=mode)
    out = torch.full((B, R, T), float('nan'), device=DEV)
    K.f16x3_out_conv(xp=xp, Cin=Cin, ks=ksz, dilation=d, direction=-1, wp=wp, net_out=out, B=B, T=T, R=R, S=0, w_scale_inv=1.0,
                     x_scale=sxd, w_scale=swd, mode=mode)
    got = out.cpu().numpy().transpose(1, 0, 2).reshape(R, B * T)
    cols = np.zeros((ksz, Cin, B, T), np.float32)                     # tap j reads dpre[t + (ks-1-j) d], zero from T on
    for j in range(ksz):
        sh = (ksz - 1 - j) * d
        cols[j, :, :, :T - sh] = dpre.transpose(1, 0, 2)[:, :, sh:]
    cols = cols.reshape(ksz * Cin, B * T)
    wm = wt.reshape(ksz * Cin, R)
    name = 'input_gradient/%s/%s' % (which, 'blocks128' if mode else 'blocks256')
    if which == 'weight_channels':
        check_curve(name, got, np.ascontiguousarray(wm.T), cols, sw, sx, ks)
    else:
        check_curve(name, np.ascontiguousarray(got.T), np.ascontiguousarray(cols.T), wm, sx, sw, ks)


def tanh_as_the_kernel_f32(z):
    """The gate kernel's epilogue in float32: tanh(x) = 1 - 2 / (exp(2x) + 1)."""
    z = z.astype(np.float32)
    with np.errstate(over='ignore'):
        return (np.float32(1) - np.float32(2) / (np.exp(np.float32(2) * z) + np.float32(1))).astype(np.float32)


@pytest.mark.parametrize('mode', [0, HALF], ids=['blocks256', 'blocks128'])
def test_range_curve_gate_conv(K, mode):
    """The gate conv (two taps, no bias, no condition) read through save0 = tanh(filter) against fp64 tanh: the filter half's weight
    output channels 2^-k down.  The kernel only shows tanh of the contraction, and its fp32 epilogue 1 - 2 / (exp(2x) + 1) has an ABSOLUTE
    error of ~1e-7, which would bury a row of size 2^-k.  So there is one launch per k with the input tensor multiplied by 2^k -- the
    same planes bit for bit, its device scale 2^-k times the first -- and a row is read from the launch that brings it back
    to the size of the k = 0 rows (rms 2^-3: tanh still passes the relative error on); the floor is that same fp32 formula on the CPU."""
    rng = np.random.RandomState(120)
    B, T, R, ksz, d = 2, 512, 256, 2, 1
    x = rng.standard_normal((B, R, T)).astype(np.float32)
    w = (rng.standard_normal((ksz, R, 2 * R)) * (2.0 ** -3 / np.sqrt(ksz * R))).astype(np.float32)
    ks = k_cycle(R)
    w[:, :, :R] *= np.exp2(-ks).astype(np.float32)[None, None, :]
    sx, sw = working_scale(x), working_scale(w)
    xp, wp = halves(2 * B * R * T), halves(2 * ksz * R * 2 * R)
    swd = slot(sw)
    K.f16x3_pack_gate_weights(dev(w), wp, ksz, R, 2 * R, 1.0, scale_dev=swd, mode=mode)
    got = np.zeros((R, B * T), np.float32)
    ref_planes = None
    for k in range(KMAX + 1):
        gain = np.float32(2.0 ** k)
        sxd = slot(sx / float(gain))
        K.f16x3_split_activations(dev(x * gain), xp, B, R, T, scale_dev=sxd, mode=mode)
        if ref_planes is None:
            ref_planes = xp.clone()
        assert torch.equal(xp.view(torch.int16), ref_planes.view(torch.int16))
        out, th = torch.empty(B, R, T, device=DEV), torch.full((B, R, T), float('nan'), device=DEV)
        K.f16x3_gate_conv(xp=xp, wp=wp, out0=out, save0=th, B=B, T=T, R=R, ks=ksz, dilation=d, w_scale_inv=1.0, x_scale=sxd, w_scale=swd,
                          mode=mode)
        rows = np.nonzero(ks == k)[0]
        got[rows] = th.cpu().numpy().transpose(1, 0, 2).reshape(R, B * T)[rows]
    cols = np.zeros((ksz, R, B, T), np.float32)                       # tap j reads x[t - (ks-1-j) d], zero before t = 0
    for j in range(ksz):
        sh = (ksz - 1 - j) * d
        cols[j, :, :, sh:] = x.transpose(1, 0, 2)[:, :, :T - sh]
    cols = cols.reshape(ksz * R, B * T)
    wm = np.ascontiguousarray(w[:, :, :R].reshape(ksz * R, R).T)
    gain64 = np.exp2(ks.astype(np.float64))[:, None]
    check_curve('gate_conv/filter_channels/%s' % ('blocks128' if mode else 'blocks256'), got, wm, cols, sw, sx, ks,
                post=lambda z: np.tanh(z * gain64), post32=lambda z: tanh_as_the_kernel_f32(z * gain64.astype(np.float32)))


def test_range_curve_strided_conv(K):
    """The encoder's stride-2 conv, forward (five taps, one zero in front, no bias / relu / affine): weight output channels 2^-k down."""
    rng = np.random.RandomState(130)
    B, Tout, Cin, M, ksz, pl = 2, 256, 128, 128, 5, 1
    Tin = 2 * Tout
    x = rng.standard_normal((B, Cin, Tin)).astype(np.float32)
    w = (rng.standard_normal((ksz, Cin, M)) * 0.05).astype(np.float32)
    ks = k_cycle(M)
    w *= np.exp2(-ks).astype(np.float32)[None, None, :]
    sx, sw = working_scale(x), working_scale(w)
    xp, wp = halves(2 * B * Cin * Tin), halves(2 * ksz * Cin * M)
    sxd, swd = slot(sx), slot(sw)
    K.f16x3_split_activations(dev(x), xp, B, Cin, Tin, scale_dev=sxd, mode=S2D)
    K.f16x3_pack_weights(dev(w), wp, ksz * Cin, M, M, 1.0, scale_dev=swd, mode=0)
    out = torch.full((B, M, Tout), float('nan'), device=DEV)
    K.f16x3_strided_conv(xp=xp, wp=wp, out=out, B=B, T=Tout, Cin=Cin, M=M, ks=ksz, pad_left=pl, x_scale=sxd, w_scale=swd)
    got = out.cpu().numpy().transpose(1, 0, 2).reshape(M, B * Tout)
    xpad = np.zeros((Cin, B, Tin + ksz), np.float32)
    xpad[:, :, pl:pl + Tin] = x.transpose(1, 0, 2)
    cols = np.stack([xpad[:, :, j:j + 2 * Tout:2] for j in range(ksz)]).reshape(ksz * Cin, B * Tout)   # tap j reads x[2t + j - pl]
    check_curve('strided_conv/weight_channels', got, np.ascontiguousarray(w.reshape(ksz * Cin, M).T), cols, sw, sx, ks)


@pytest.mark.parametrize('which', ['q_channels', 'p_channels'])
def test_range_curve_wgrad(K, which):
    """The weight gradient with the operands split in registers (one tap, contraction over batch and time): the output channels
    of q0 2^-k down (read along dw's columns), then the input channels of p (dw's rows)."""
    rng = np.random.RandomState(140)
    B, T, Cp, Q0 = 2, 512, 256, 256
    p = rng.standard_normal((B, Cp, T)).astype(np.float32)
    q = (rng.standard_normal((B, Q0, T)) * 1e-5).astype(np.float32)
    ks = k_cycle(256)
    if which == 'q_channels':
        q *= np.exp2(-ks).astype(np.float32)[None, :, None]
    else:
        p *= np.exp2(-ks).astype(np.float32)[None, :, None]
    sp, sq = working_scale(p), working_scale(q)
    dw = torch.zeros(Cp, Q0, device=DEV)
    slab = torch.empty(256 * 65536, device=DEV)
    K.f16x3_wgrad(p=dev(p), q0=dev(q), dw=dw, slab=slab, B=B, T=T, Cp=Cp, Q0=Q0, taps=[0], p_scale=slot(sp), q0_scale=slot(sq), mode=0)
    got = dw.cpu().numpy()
    pm = np.ascontiguousarray(p.transpose(1, 0, 2).reshape(Cp, B * T))
    qm = np.ascontiguousarray(q.transpose(1, 0, 2).reshape(Q0, B * T))
    if which == 'q_channels':
        check_curve('wgrad/q_channels', np.ascontiguousarray(got.T), qm, np.ascontiguousarray(pm.T), sq, sp, ks)
    else:
        check_curve('wgrad/p_channels', got, pm, np.ascontiguousarray(qm.T), sp, sq, ks)
