"""GPU parity tests of the individual HIP kernels (through the C ABI) against the CPU oracle.

Tolerances: integer / index outputs are compared bit-exactly; fp32 MFMA results against the
torch-CPU fp32 oracle within 2e-4 of the tensor max (`close`; both sides accumulate K<=2304 fp32
products in different orders); weight gradients (53 248-term sums) 5e-4, 1e-3 at the full size.
"""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import ref_ops as R
from oracle import ref_model as M

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import x3_ref as X  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def g(t):
    return t.contiguous().to(DEV)


@pytest.fixture(params=['0', '1'], ids=['blocks256', 'blocks128'])
def x3half(request, monkeypatch):
    """Both block heights of the fp16x3 conv kernels (VQW_X3_HALF: 128-row blocks, two per CU)."""
    monkeypatch.setenv('VQW_X3_HALF', request.param)
    return request.param


def bct(x_btc):
    """[B,T,C] -> contiguous (B,C,T) on the GPU."""
    return x_btc.transpose(1, 2).contiguous().to(DEV)


def btc(x_bct):
    return x_bct.detach().cpu().transpose(1, 2).contiguous()


def close(a, b, rtol=None, atol=None, what=''):
    """max |a - b| <= tol * max(1, max |b|), tol = the LARGER of rtol / atol where a test names them (they are one bar
    relative to the tensor max, not two that add up), else the 2e-4 of the module docstring / DESIGN 6."""
    given = [t for t in (rtol, atol) if t is not None]
    tol = max(given) if given else 2e-4
    a, b = a.detach().cpu().float(), b.detach().cpu().float()
    scale = max(1.0, float(b.abs().max()))
    err = float((a - b).abs().max())
    assert err <= tol * scale, '%s max abs err %.3e (scale %.3e)' % (what, err, scale)


# ----------------------------------------------------------------------------- mu-law
def test_mu_law_int_all_pcm_codes_bit_exact(K):
    pcm = np.arange(-32768, 32768, dtype=np.int64)
    xs = ((pcm.astype(np.float32) + np.float32(0.5)) / np.float32(32767.5)).astype(np.float32)
    want = R.mu_law_encode_np(xs, to_int=True)
    got = K.mu_law_encode_i32(g(torch.from_numpy(xs))).cpu().numpy()
    assert np.array_equal(got, want)
    import os
    fixture = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'mu_law_pcm_labels.npy'))   # committed vector
    assert np.array_equal(got.astype(np.uint8), fixture)


def test_mu_law_int_random_and_edges_bit_exact(K):
    rng = np.random.RandomState(0)
    xs = np.concatenate([rng.uniform(-1.2, 1.2, 1 << 20).astype(np.float32),
                         np.array([-2, -1, -0.0, 0.0, 1, 2, 1e-30, -1e-30, 0.999999, -0.999999], np.float32),
                         np.nextafter(np.float32(1), np.float32(0), dtype=np.float32).reshape(1)])
    want = R.mu_law_encode_np(xs, to_int=True)
    got = K.mu_law_encode_i32(g(torch.from_numpy(xs))).cpu().numpy()
    assert np.array_equal(got, want)


def test_mu_law_float_and_decode(K):
    rng = np.random.RandomState(1)
    xs = rng.uniform(-1.1, 1.1, 100000).astype(np.float32)
    got = K.mu_law_encode_f32(g(torch.from_numpy(xs))).cpu().numpy()
    np.testing.assert_allclose(got, R.mu_law_encode_np(xs), rtol=0, atol=3e-7)
    idx = np.arange(0, 257, dtype=np.float32)
    dec = K.mu_law_decode_f32(g(torch.from_numpy(idx))).cpu().numpy()
    np.testing.assert_allclose(dec, R.mu_law_decode_np(idx), rtol=2e-6, atol=1e-7)


def test_wavenet_inputs(K):
    x, _, _ = M.synthetic_batch(3, 512, 10, 7)
    xb = g(x[:, :, 0])
    inputs = torch.empty_like(xb)
    labels = torch.empty(xb.shape, dtype=torch.int32, device=DEV)
    K.wavenet_inputs(xb, inputs, labels)
    want_l = R.mu_law_encode_np(x[:, :, 0].numpy(), to_int=True)
    assert np.array_equal(labels.cpu().numpy(), want_l)
    want_i = R.mu_law_encode_np(R.shift_right(x)[:, :, 0].numpy())
    np.testing.assert_allclose(inputs.cpu().numpy(), want_i, atol=3e-7)


def test_empty_inputs_are_ok(K):
    e = torch.empty(0, device=DEV)
    assert K.mu_law_encode_f32(e).numel() == 0
    assert K.mu_law_encode_i32(e).numel() == 0


# ----------------------------------------------------------------------------- VQ
@pytest.mark.parametrize('B,Tz,D,Kc', [(2, 8, 16, 32), (8, 104, 64, 512), (3, 5, 64, 100)])
def test_vq_nearest_bit_exact(K, B, Tz, D, Kc):
    rng = np.random.RandomState(3)
    z = torch.from_numpy(rng.standard_normal((B, Tz, D)).astype(np.float32) * 0.2)
    emb = torch.from_numpy(rng.uniform(-0.13, 0.13, (Kc, D)).astype(np.float32))
    emb[7] = emb[3]                       # exact tie between two codes: lowest index must win
    z[0, 0] = emb[7]
    q, e_k, z_q = M.discretise(z, emb)
    zb = bct(z)
    idx = torch.empty(B, Tz, dtype=torch.int64, device=DEV)
    ek = torch.empty(B, D, Tz, device=DEV)
    zq = torch.empty(B, D, Tz, device=DEV)
    mind = torch.empty(B, Tz, device=DEV)
    K.vq_nearest_fwd(zb, g(emb), idx=idx, e_k=ek, zq=zq, mind=mind)
    assert torch.equal(idx.cpu(), q)
    assert int(idx[0, 0]) == 3
    assert torch.equal(btc(ek), e_k)
    assert torch.equal(btc(zq), z_q)      # z_e + (e_k - z_e), same rounding
    d = M.vq_distances_np(z.reshape(-1, D).numpy(), emb.numpy()).min(-1)
    assert np.array_equal(mind.cpu().numpy().reshape(-1), d)


def test_vq_bwd_and_speaker(K):
    rng = np.random.RandomState(4)
    B, Tz, D, Kc, Cs, S = 2, 8, 16, 32, 16, 5
    z = torch.from_numpy(rng.standard_normal((B, D, Tz)).astype(np.float32)).to(DEV)
    emb = torch.from_numpy(rng.standard_normal((Kc, D)).astype(np.float32)).to(DEV)
    idx = torch.empty(B, Tz, dtype=torch.int64, device=DEV)
    ek = torch.empty(B, D, Tz, device=DEV)
    K.vq_nearest_fwd(z, emb, idx=idx, e_k=ek)
    Cc = D + Cs
    dcond = torch.from_numpy(rng.standard_normal((B, Cc, Tz)).astype(np.float32)).to(DEV)
    dz = torch.empty_like(z)
    demb = torch.zeros(Kc, D, device=DEV)
    K.vq_nearest_bwd(z, ek, idx, dzq=dcond, dzq_bstride=Cc * Tz, dz_e=dz, demb=demb, cscale=0.3, escale=0.7, K=Kc)
    want_dz = dcond[:, :D] + 0.3 * (z - ek)
    close(dz, want_dz, what='dz_e')
    want_demb = torch.zeros(Kc, D, device=DEV)
    want_demb.index_add_(0, idx.reshape(-1), (0.7 * (ek - z)).permute(0, 2, 1).reshape(-1, D))
    close(demb, want_demb, what='demb')
    table = torch.from_numpy(rng.standard_normal((S, Cs)).astype(np.float32)).to(DEV)
    spk = torch.tensor([4, 1], dtype=torch.int64, device=DEV)
    cond = torch.zeros(B, Cc, Tz, device=DEV)
    K.speaker_tile_fwd(table, spk, cond, cond_bstride=Cc * Tz, row0=D, Cs=Cs, Tz=Tz)
    assert torch.equal(cond[:, D:], table[spk][:, :, None].expand(-1, -1, Tz))
    assert float(cond[:, :D].abs().max()) == 0.0
    dt = torch.zeros(S, Cs, device=DEV)
    K.speaker_tile_bwd(dcond, spk, dt, dcond_bstride=Cc * Tz, row0=D, Cs=Cs, Tz=Tz)
    want = torch.zeros(S, Cs, device=DEV)
    want.index_add_(0, spk, dcond[:, D:].sum(-1))
    close(dt, want, what='dspeaker')
    # ids outside the table: row 0, as the reference's one_hot -> argmax (model.py:22); never a read outside the table
    bad = torch.tensor([S + 3, -1], dtype=torch.int64, device=DEV)
    K.speaker_tile_fwd(table, bad, cond, cond_bstride=Cc * Tz, row0=D, Cs=Cs, Tz=Tz)
    assert torch.equal(cond[:, D:], table[[0, 0]][:, :, None].expand(-1, -1, Tz))
    dt.zero_()
    K.speaker_tile_bwd(dcond, bad, dt, dcond_bstride=Cc * Tz, row0=D, Cs=Cs, Tz=Tz)
    assert float(dt[1:].abs().max()) == 0.0
    close(dt[0], dcond[:, D:].sum((0, 2)), what='out-of-range ids accumulate into row 0')
    with pytest.raises(ValueError):
        K.speaker_tile_fwd(table, spk.to(torch.int32), cond, cond_bstride=Cc * Tz, row0=D, Cs=Cs, Tz=Tz)


# ----------------------------------------------------------------------------- conv engine
def rnd(*shape, seed=0, s=1.0):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(shape).astype(np.float32) * s)


CONV_CASES = [
    # B, T, Cin, Cout, k, dilation, tile
    (2, 512, 32, 64, 3, 1, 0),
    (2, 512, 32, 64, 3, 4, 24),
    (1, 1024, 64, 128, 3, 512, 24),     # dilation larger than the tile: whole taps skipped
    (2, 260, 48, 68, 2, 3, 22),         # ragged T and channel counts
    (2, 512, 32, 64, 1, 1, 12),
    (1, 6656, 256, 512, 3, 64, 0),      # full-size decoder layer (B=1)
]


@pytest.mark.parametrize('B,T,Cin,Cout,k,dil,tile', CONV_CASES)
def test_causal_conv_fwd_matches_oracle(K, B, T, Cin, Cout, k, dil, tile):
    x, w, b = rnd(B, T, Cin, seed=1), rnd(k, Cin, Cout, seed=2, s=(k * Cin) ** -0.5), rnd(Cout, seed=3)
    want = R.conv1d_v2(x, w, b, dilations=dil)
    out = torch.full((B, Cout, T), float('nan'), device=DEV)
    K.conv_gemm(x0=bct(x), w=g(w), bias=g(b), out0=out, B=B, T_in=T, T_out=T, M=Cout, C0=Cin,
                taps=[-(k - 1 - j) * dil for j in range(k)], tile=tile)
    close(btc(out), want, what='conv fwd')


def _ragged_cases():
    """Seeded random shapes for the conv engine: ragged T (partial tiles, 4-byte-aligned-only rows), every tile,
    tail tiles forced on, split-K forced on, dilations that put taps outside the signal, odd batch sizes."""
    rng = np.random.RandomState(2026)
    cases = []
    for i in range(28):
        B = int(rng.choice([1, 2, 3, 5]))
        T = int(rng.choice([64, 100, 128, 200, 260, 384, 500, 777, 1024, 1500]))
        Cin = 16 * int(rng.randint(1, 7))
        Cout = 4 * int(rng.randint(1, 80))
        k = int(rng.choice([1, 2, 3, 5]))
        dil = int(rng.choice([1, 2, 3, 8, 64, 300]))
        tile = int(rng.choice([0, 11, 12, 14, 21, 22, 24]))
        if tile and tile % 10 > 1 and rng.rand() < 0.5:
            tile += 10000 * int(rng.randint(1, 4))           # hand some columns to half-width tail tiles
        split = int(rng.choice([0, 0, 1, 2, 3, 7]))
        cases.append((B, T, Cin, Cout, k, dil, tile, split, i))
    return cases


@pytest.mark.parametrize('B,T,Cin,Cout,k,dil,tile,split,seed', _ragged_cases())
def test_conv_engine_ragged_shapes(K, B, T, Cin, Cout, k, dil, tile, split, seed):
    """wavenet_ops.py:59-90 on shapes the model never uses: the engine's paths (LDS-DMA interior blocks, register
    pipeline at the edges, tail tiles, split-K with atomics, tile heuristic) must agree with the oracle on all."""
    x, w, b = rnd(B, T, Cin, seed=seed), rnd(k, Cin, Cout, seed=seed + 100, s=(k * Cin) ** -0.5), rnd(Cout, seed=seed + 200)
    want = R.conv1d_v2(x, w, b, dilations=dil)
    out = torch.full((B, Cout, T), float('nan'), device=DEV)
    K.conv_gemm(x0=bct(x), w=g(w), bias=g(b), out0=out, B=B, T_in=T, T_out=T, M=Cout, C0=Cin,
                taps=[-(k - 1 - j) * dil for j in range(k)], tile=tile, split_k=split)
    close(btc(out), want, what='conv fwd (tile %d, split %d)' % (tile, split))


def test_named_wrappers_causal(K, pkg):
    L = pkg._lib
    B, T, Cin, Cout, k, dil = 2, 384, 32, 64, 3, 2
    x, w, b = rnd(B, T, Cin, seed=1), rnd(k, Cin, Cout, seed=2, s=0.1), rnd(Cout, seed=3)
    xb, wb, bb = bct(x), g(w), g(b)
    y = torch.empty(B, Cout, T, device=DEV)
    L.check(L.lib().vqw_causal_conv1d_fwd(L.ptr(xb), L.ptr(wb), L.ptr(bb), L.ptr(y), B, Cin, Cout, T, k, dil, 1, L.stream()))
    xr = x.clone().requires_grad_(True); wr = w.clone().requires_grad_(True)
    yo = R.conv1d_v2(xr, wr, b, dilations=dil)
    close(btc(y), yo, what='wrapper fwd')
    dy = rnd(B, T, Cout, seed=9)
    yo.backward(dy)
    wT = torch.empty(k, Cout, Cin, device=DEV)
    K.transpose(wb, wT, k, Cin, Cout)
    assert torch.equal(wT.cpu(), w.transpose(1, 2))
    dx = torch.empty(B, Cin, T, device=DEV)
    dyb = bct(dy)
    L.check(L.lib().vqw_causal_conv1d_dgrad(L.ptr(dyb), L.ptr(wT), L.ptr(dx), B, Cin, Cout, T, k, dil, L.stream()))
    close(btc(dx), xr.grad, what='wrapper dgrad')
    dw = torch.zeros(k, Cin, Cout, device=DEV)
    L.check(L.lib().vqw_causal_conv1d_wgrad(L.ptr(xb), L.ptr(dyb), L.ptr(dw), B, Cin, Cout, T, k, dil, L.stream()))
    close(dw, wr.grad, rtol=5e-4, atol=5e-4, what='wrapper wgrad')
    # stride 2 (conv1d_v2 with stride, Encoder_Magenta use)
    y2 = torch.empty(B, Cout, T // 2, device=DEV)
    L.check(L.lib().vqw_causal_conv1d_fwd(L.ptr(xb), L.ptr(wb), L.ptr(bb), L.ptr(y2), B, Cin, Cout, T, k, dil, 2, L.stream()))
    close(btc(y2), R.conv1d_v2(x, w, b, dilations=dil, stride=2), what='wrapper fwd stride 2')


def test_named_wrappers_pointwise(K, pkg):
    """vqw_pointwise_gemm_{fwd,dgrad,wgrad} (wavenet_ops.py:132-136 / 147-160: the 1x1 convs) through the C ABI:
    plain, relu prologue, accumulate-into-output; input and weight gradients against torch autograd."""
    L = pkg._lib
    B, T, Cin, Cout = 2, 320, 64, 96
    x, w, b = rnd(B, T, Cin, seed=11), rnd(Cin, Cout, seed=12, s=0.1), rnd(Cout, seed=13)
    xb, wb, bb = bct(x), g(w), g(b)
    y = torch.full((B, Cout, T), float('nan'), device=DEV)
    L.check(L.lib().vqw_pointwise_gemm_fwd(L.ptr(xb), L.ptr(wb), L.ptr(bb), L.ptr(y), B, Cin, Cout, T, 0, 0, L.stream()))
    close(btc(y), x @ w + b, what='pointwise fwd')
    L.check(L.lib().vqw_pointwise_gemm_fwd(L.ptr(xb), L.ptr(wb), None, L.ptr(y), B, Cin, Cout, T, 1, 0, L.stream()))
    close(btc(y), torch.relu(x) @ w, what='pointwise fwd, relu prologue, no bias')
    acc0 = rnd(B, T, Cout, seed=14)
    acc = bct(acc0)
    L.check(L.lib().vqw_pointwise_gemm_fwd(L.ptr(xb), L.ptr(wb), L.ptr(bb), L.ptr(acc), B, Cin, Cout, T, 0, 1, L.stream()))
    close(btc(acc), acc0 + x @ w + b, what='pointwise fwd, accumulate (skip += ...)')
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    dy = rnd(B, T, Cout, seed=15)
    (torch.relu(xr) @ wr).backward(dy)
    dyb = bct(dy)
    wT = torch.empty(Cout, Cin, device=DEV)
    K.transpose(wb, wT, 1, Cin, Cout)
    dx = torch.empty(B, Cin, T, device=DEV)
    L.check(L.lib().vqw_pointwise_gemm_dgrad(L.ptr(dyb), L.ptr(wT), L.ptr(dx), B, Cin, Cout, T, L.stream()))
    close(btc(dx) * (x > 0), xr.grad, what='pointwise dgrad (relu mask applied by the caller)')
    dw = torch.zeros(Cin, Cout, device=DEV)
    L.check(L.lib().vqw_pointwise_gemm_wgrad(L.ptr(xb), L.ptr(dyb), L.ptr(dw), B, Cin, Cout, T, 1, L.stream()))
    close(dw, wr.grad, rtol=5e-4, atol=5e-4, what='pointwise wgrad, relu prologue')
    L.check(L.lib().vqw_pointwise_gemm_wgrad(L.ptr(xb), L.ptr(dyb), L.ptr(dw), B, Cin, Cout, T, 1, L.stream()))
    close(dw, 2 * wr.grad, rtol=5e-4, atol=5e-4, what='pointwise wgrad accumulates into dw')
    assert L.lib().vqw_pointwise_gemm_fwd(None, L.ptr(wb), None, L.ptr(y), B, Cin, Cout, T, 0, 0, L.stream()) != 0
    assert b'null' in L.lib().vqw_last_error().lower() or L.lib().vqw_last_error()


def test_conv1d_v2_is_differentiable(pkg):
    """ops.conv1d_v2 / ops.linear under torch.autograd: the gradients TF would derive (Conv2DBackpropInput,
    Conv2DBackpropFilter, BiasAddGrad) come from vqw_causal_conv1d_{dgrad,wgrad} and match autograd through the oracle."""
    O = pkg.ops
    B, T, Cin, Cout, k, dil = 2, 320, 32, 48, 3, 4
    x, w, b = rnd(B, T, Cin, seed=21), rnd(k, Cin, Cout, seed=22, s=0.1), rnd(Cout, seed=23)
    dy = rnd(B, T, Cout, seed=24)
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, b))
    R.conv1d_v2(xr, wr, br, dilations=dil).backward(dy)
    xg, wg, bg = (g(t).requires_grad_(True) for t in (x, w, b))
    y = O.conv1d_v2(xg, wg, bg, dilations=dil)
    assert y.requires_grad
    y.backward(g(dy))
    close(y, R.conv1d_v2(x, w, b, dilations=dil), what='fwd')
    close(xg.grad, xr.grad, what='d input')
    close(wg.grad, wr.grad, rtol=5e-4, atol=5e-4, what='d kernel')
    close(bg.grad, br.grad, rtol=5e-4, atol=5e-4, what='d bias')
    v = g(rnd(B, Cin, seed=25)).requires_grad_(True)
    O.linear(v, wg[1:2].detach(), None).sum().backward()                 # wavenet_ops.py:147-160 on [B, Cin]
    close(v.grad, w[1].sum(-1)[None].expand(B, -1), what='linear d input')


def test_bad_arguments_return_errors_not_faults(K, pkg):
    L = pkg._lib
    x = torch.zeros(1, 24, 64, device=DEV)
    with pytest.raises(RuntimeError, match='multiples of 16'):
        K.conv_gemm(x0=x, w=torch.zeros(24, 16, device=DEV), out0=torch.zeros(1, 16, 64, device=DEV),
                    B=1, T_in=64, T_out=64, M=16, C0=24, taps=[0])
    with pytest.raises(ValueError, match='elements'):
        K.conv_gemm(x0=x, w=torch.zeros(4, device=DEV), out0=torch.zeros(1, 16, 64, device=DEV),
                    B=1, T_in=64, T_out=64, M=16, C0=16, taps=[0])
    assert L.lib().vqw_conv_gemm(None, None) != 0


@pytest.mark.parametrize('T,tile', [(512, 24), (384, 22)])
def test_gate_epilogue_with_condition(K, T, tile):
    B, Cin, H, Cc, ratio = 2, 32, 32, 16, 64
    Tz = T // ratio
    x, w, b = rnd(B, T, Cin, seed=1), rnd(3, Cin, 2 * H, seed=2, s=0.1), rnd(2 * H, seed=3, s=0.3)
    cond, wc = rnd(B, Tz, Cc, seed=4), rnd(1, Cc, 2 * H, seed=5, s=0.2)
    p = {'gated/kernel': w, 'gated/bias': b, 'gated/local_condition/kernel': wc}
    want = R.gated_cnn(x, p, H, 2, cond)
    enc = R.conv1d_v2(cond, wc)                                  # [B,Tz,2H]
    out = torch.empty(B, H, T, device=DEV); th = torch.empty_like(out); sg = torch.empty_like(out)
    K.conv_gemm(x0=bct(x), w=g(w), bias=g(b), out0=out, save0=th, save1=sg, B=B, T_in=T, T_out=T, M=2 * H,
                C0=Cin, taps=[-4, -2, 0], epilogue=K.EPI_GATE, cond=bct(enc), cond_T=Tz, tile=tile)
    close(btc(out), want, atol=2e-5, rtol=2e-5, what='gated')
    close(th * sg, out, atol=1e-6, rtol=0, what='saved tanh*sigmoid')


@pytest.mark.parametrize('d', [1, 8, 512])
def test_gate_conv_full_size_properties(K, d):
    """BASELINE.json configs[1] sizes (B=8, T=6656, 256 -> 512, k=3): the grid the bench runs (LDS-DMA interior
    blocks, register-pipeline edge blocks, half-width tail tiles).  Size-independent checks: (1) sampled outputs
    against an fp64 evaluation of wavenet_ops.py:81-113 at those points; (2) causality -- perturbing x at
    t >= t0 leaves every output at t < t0 bit-identical; (3) saved tanh * sigmoid == gated."""
    B, T, Rr, ratio = 8, 6656, 256, 64
    Tz = T // ratio
    gen = torch.Generator().manual_seed(10 + d)
    x = torch.randn(B, Rr, T, generator=gen)
    w = torch.randn(3, Rr, 2 * Rr, generator=gen) * 0.05
    b = torch.randn(2 * Rr, generator=gen) * 0.3
    cond = torch.randn(B, 2 * Rr, Tz, generator=gen) * 0.3
    xd, wd, bd, cd = x.to(DEV), w.to(DEV), b.to(DEV), cond.to(DEV)
    out = torch.empty(B, Rr, T, device=DEV); th = torch.empty_like(out); sg = torch.empty_like(out)
    args = dict(w=wd, bias=bd, save0=th, save1=sg, B=B, T_in=T, T_out=T, M=2 * Rr, C0=Rr, taps=[-2 * d, -d, 0],
                epilogue=K.EPI_GATE, cond=cd, cond_T=Tz)
    K.conv_gemm(x0=xd, out0=out, **args)
    got = out.cpu()
    assert torch.isfinite(got).all()
    assert float((th * sg - out).abs().max()) <= 1e-6
    # (1) sampled points, biased towards the edges of the signal and of the tiles
    g2 = torch.Generator().manual_seed(99)
    n = 3000
    bb = torch.randint(0, B, (n,), generator=g2)
    cc = torch.randint(0, Rr, (n,), generator=g2)
    tt = torch.randint(0, T, (n,), generator=g2)
    tt[:300] = torch.randint(0, 2 * d + 2, (300,), generator=g2).clamp(max=T - 1)
    tt[300:600] = T - 1 - torch.randint(0, 130, (300,), generator=g2)
    tt[600:900] = (torch.randint(0, T // 128, (300,), generator=g2) * 128 + torch.randint(-1, 2, (300,), generator=g2)).clamp(0, T - 1)
    x64, w64 = x.double(), w.double()
    worst = 0.0
    for i in range(n):
        bi, ci, ti = int(bb[i]), int(cc[i]), int(tt[i])
        pre = torch.zeros(2, dtype=torch.float64)
        for j, sh in enumerate((-2 * d, -d, 0)):
            if ti + sh >= 0:
                xv = x64[bi, :, ti + sh]
                pre[0] += (xv * w64[j, :, ci]).sum()
                pre[1] += (xv * w64[j, :, Rr + ci]).sum()
        pre[0] += float(b[ci]) + float(cond[bi, ci, ti // ratio])
        pre[1] += float(b[Rr + ci]) + float(cond[bi, Rr + ci, ti // ratio])
        want = float(torch.tanh(pre[0]) * torch.sigmoid(pre[1]))
        worst = max(worst, abs(float(got[bi, ci, ti]) - want))
    assert worst < 2e-5, 'sampled gate outputs differ from fp64 evaluation by %.3e' % worst
    # (2) causality
    t0 = 4001
    x2 = xd.clone()
    x2[:, :, t0:] += 1.0
    out2 = torch.empty_like(out)
    K.conv_gemm(x0=x2, out0=out2, **args)
    assert torch.equal(out2[:, :, :t0], out[:, :, :t0]), 'outputs before t0 changed'
    assert not torch.equal(out2[:, :, t0:], out[:, :, t0:])


@pytest.mark.parametrize('B,T,Rr,ks,d', [(2, 512, 128, 3, 1), (2, 512, 128, 2, 7), (1, 1024, 256, 3, 64),
                                         (2, 768, 128, 3, 300), (8, 6656, 256, 3, 4), (8, 6656, 256, 3, 512)])
def test_gate_conv_f16x3_matches_fp32_engine(K, x3half, B, T, Rr, ks, d):
    """Gate conv of the fp16x3 engine (two fp16 planes per operand, three MFMA terms)
    against (1) the fp32-MFMA engine on the same inputs -- two fp32-accurate evaluations of wavenet_ops.py:104-114,
    equal to 2e-5 over all 13.6 M outputs of the benchmark shape -- and (2) an fp64 evaluation at sampled points, where it must be at least as close as the
    tolerance the fp32 engine is held to (2e-5).  Covers the causal zero padding (dilation beyond the tile and
    beyond the signal), both kernel sizes of the reference configs, and the full benchmark shape."""
    ratio = 64 if T % 64 == 0 and (T // 64) >= 1 else 32
    Tz = T // ratio
    gen = torch.Generator().manual_seed(1000 + d + T)
    x = torch.randn(B, Rr, T, generator=gen)
    w = torch.randn(ks, Rr, 2 * Rr, generator=gen) * 0.05
    b = torch.randn(2 * Rr, generator=gen) * 0.3
    cond = torch.randn(B, 2 * Rr, Tz, generator=gen) * 0.3
    xd, wd, bd, cd = x.to(DEV), w.to(DEV), b.to(DEV), cond.to(DEV)
    taps = [-(ks - 1 - j) * d for j in range(ks)]
    ref = torch.empty(B, Rr, T, device=DEV); rth = torch.empty_like(ref); rsg = torch.empty_like(ref)
    K.conv_gemm(x0=xd, w=wd, bias=bd, out0=ref, save0=rth, save1=rsg, B=B, T_in=T, T_out=T, M=2 * Rr, C0=Rr,
                taps=taps, epilogue=K.EPI_GATE, cond=cd, cond_T=Tz)
    xp = torch.empty(2 * B * Rr * T, dtype=torch.float16, device=DEV)
    wp = torch.empty(2 * ks * Rr * 2 * Rr, dtype=torch.float16, device=DEV)
    out = torch.empty_like(ref); th = torch.empty_like(ref); sg = torch.empty_like(ref)
    K.f16x3_split_activations(xd, xp, B, Rr, T)
    K.f16x3_pack_gate_weights(wd, wp, ks, Rr, 2 * Rr, 256.0)
    K.f16x3_gate_conv(xp=xp, wp=wp, out0=out, save0=th, save1=sg, bias=bd, cond=cd, cond_T=Tz, B=B, T=T, R=Rr, ks=ks,
                      dilation=d, w_scale_inv=1.0 / 256.0)
    assert torch.isfinite(out).all()
    for got, want, nm in ((out, ref, 'gated'), (th, rth, 'tanh'), (sg, rsg, 'sigmoid')):
        err = float((got - want).abs().max())
        assert err <= 2e-5, '%s differs from the fp32 engine by %.3e' % (nm, err)
    assert float((th * sg - out).abs().max()) <= 1e-6
    # sampled points against fp64
    g2 = torch.Generator().manual_seed(7)
    n = 600
    bb = torch.randint(0, B, (n,), generator=g2); cc = torch.randint(0, Rr, (n,), generator=g2)
    tt = torch.randint(0, T, (n,), generator=g2)
    tt[:150] = torch.randint(0, min(T, (ks - 1) * d + 2), (150,), generator=g2)
    x64, w64, got = x.double(), w.double(), out.cpu()
    worst = worst_ref = 0.0
    refc = ref.cpu()
    for i in range(n):
        bi, ci, ti = int(bb[i]), int(cc[i]), int(tt[i])
        pre = torch.zeros(2, dtype=torch.float64)
        for j, sh in enumerate(taps):
            if ti + sh >= 0:
                xv = x64[bi, :, ti + sh]
                pre[0] += (xv * w64[j, :, ci]).sum()
                pre[1] += (xv * w64[j, :, Rr + ci]).sum()
        pre[0] += float(b[ci]) + float(cond[bi, ci, ti // ratio])
        pre[1] += float(b[Rr + ci]) + float(cond[bi, Rr + ci, ti // ratio])
        want = float(torch.tanh(pre[0]) * torch.sigmoid(pre[1]))
        worst = max(worst, abs(float(got[bi, ci, ti]) - want))
        worst_ref = max(worst_ref, abs(float(refc[bi, ci, ti]) - want))
    assert worst < 2e-5, 'f16x3 gate outputs differ from fp64 by %.3e (fp32 engine: %.3e)' % (worst, worst_ref)


@pytest.mark.parametrize('B,T', [(2, 512), (8, 6656)])
def test_out_conv_f16x3_matches_fp32_engine(K, x3half, B, T):
    """1x1 skip + residual conv of the fp16x3 engine, fed by the gate kernel's plane output and
    writing the next layer's input planes: against the fp32 engine's ACCUM_SPLIT launch on the same inputs (2e-5 of
    the tensor max) and the planes against a split of the fp32 result (bit-identical fp16 pieces)."""
    Rr, S, ks, d = 256, 512, 3, 2
    gen = torch.Generator().manual_seed(77 + T)
    x = torch.randn(B, Rr, T, generator=gen)
    wg = torch.randn(ks, Rr, 2 * Rr, generator=gen) * 0.05
    wo = torch.randn(Rr, S + Rr, generator=gen) * 0.08
    bo = torch.randn(S + Rr, generator=gen) * 0.3
    skip0 = torch.randn(B, S, T, generator=gen)
    xd, wgd, wod, bod = x.to(DEV), wg.to(DEV), wo.to(DEV), bo.to(DEV)
    xp = torch.empty(2 * B * Rr * T, dtype=torch.float16, device=DEV)
    gp = torch.empty_like(xp); np_ = torch.empty_like(xp); np_ref = torch.empty_like(xp)
    wgp = torch.empty(2 * ks * Rr * 2 * Rr, dtype=torch.float16, device=DEV)
    wop = torch.empty(2 * Rr * (S + Rr), dtype=torch.float16, device=DEV)
    gated = torch.empty(B, Rr, T, device=DEV)
    K.f16x3_split_activations(xd, xp, B, Rr, T)
    K.f16x3_pack_gate_weights(wgd, wgp, ks, Rr, 2 * Rr, 256.0)
    K.f16x3_gate_conv(xp=xp, wp=wgp, out0=gated, out_planes=gp, B=B, T=T, R=Rr, ks=ks, dilation=d, w_scale_inv=1.0 / 256.0)
    gp_ref = torch.empty_like(xp)
    K.f16x3_split_activations(gated, gp_ref, B, Rr, T)
    assert torch.equal(gp.view(torch.int16), gp_ref.view(torch.int16)), 'gated planes differ from a split of the gated tensor'
    # fp32 engine reference
    skip_ref = skip0.to(DEV); net_ref = torch.empty(B, Rr, T, device=DEV)
    K.conv_gemm(x0=gated, w=wod, bias=bod, out0=skip_ref, out1=net_ref, aux1=xd, B=B, T_in=T, T_out=T, M=S + Rr, M0=S,
                C0=Rr, taps=[0], epilogue=K.EPI_ACCUM_SPLIT)
    skip = skip0.to(DEV); net = torch.empty(B, Rr, T, device=DEV)
    K.f16x3_pack_weights(wod, wop, Rr, S + Rr, S + Rr, 64.0)
    K.f16x3_out_conv(xp=gp, wp=wop, bias=bod, skip=skip, net_in=xd, net_out=net, net_out_planes=np_, B=B, T=T, R=Rr, S=S,
                     w_scale_inv=1.0 / 64.0)
    for got, want, nm in ((skip, skip_ref, 'skip'), (net, net_ref, 'net')):
        err = float((got - want).abs().max()) / float(want.abs().max())
        assert err <= 2e-5, '%s differs from the fp32 engine by %.3e of max' % (nm, err)
    K.f16x3_split_activations(net, np_ref, B, Rr, T)
    assert torch.equal(np_.view(torch.int16), np_ref.view(torch.int16)), 'net planes differ from a split of net_out'


@pytest.mark.parametrize('B,T,d,top', [(2, 512, 3, False), (2, 768, 300, True), (8, 6656, 16, False)])
def test_dgrad_f16x3_matches_fp32_engine(K, x3half, B, T, d, top):
    """fp16x3 input gradient of the gate conv (reads AHEAD: x[t + (ks-1-j) d], zero behind the end of a batch row)
    with the gradient operand lifted by 2^20 into fp16 planes: against the fp32 engine's dgrad launch on the same
    tiny-magnitude inputs (relative 2e-5 of the tensor max)."""
    Rr, ks = 256, 3
    gen = torch.Generator().manual_seed(5 + T + d)
    dpre = (torch.randn(B, 2 * Rr, T, generator=gen) * 3e-6).to(DEV)
    wt = (torch.randn(ks, 2 * Rr, Rr, generator=gen) * 0.05).to(DEV)
    dnet = (torch.randn(B, Rr, T, generator=gen) * 1e-5).to(DEV)
    taps_b = [(ks - 1 - j) * d for j in range(ks)]
    ref = torch.empty(B, Rr, T, device=DEV)
    if top:
        K.conv_gemm(x0=dpre, w=wt, out0=ref, B=B, T_in=T, T_out=T, M=Rr, C0=2 * Rr, taps=taps_b)
    else:
        K.conv_gemm(x0=dpre, w=wt, out1=ref, aux1=dnet, out0=ref, B=B, T_in=T, T_out=T, M=Rr, M0=0, C0=2 * Rr, taps=taps_b,
                    epilogue=K.EPI_ACCUM_SPLIT)
    GS = float(2 ** 20)
    dp = torch.empty(2 * B * 2 * Rr * T, dtype=torch.float16, device=DEV)
    wp = torch.empty(2 * ks * 2 * Rr * Rr, dtype=torch.float16, device=DEV)
    out = torch.empty_like(ref)
    K.f16x3_split_activations(dpre, dp, B, 2 * Rr, T, scale=GS)
    K.f16x3_pack_weights(wt, wp, ks * 2 * Rr, Rr, Rr, 256.0)
    K.f16x3_out_conv(xp=dp, Cin=2 * Rr, ks=ks, dilation=d, direction=-1, wp=wp, net_in=None if top else dnet, net_out=out,
                     B=B, T=T, R=Rr, S=0, w_scale_inv=1.0 / (256.0 * GS))
    assert torch.isfinite(out).all()
    err = float((out - ref).abs().max()) / float(ref.abs().max())
    assert err <= 2e-5, 'input gradient differs from the fp32 engine by %.3e of max' % err


@pytest.mark.parametrize('B,T,d,Q1,scaled', [(2, 512, 1, 256, False), (2, 512, 2, 0, True), (1, 1024, 4, 256, True), (2, 512, 16, 256, False),
                                             (1, 512, 512, 0, False), (3, 544, 3, 256, True)])
def test_wgrad_f16x3_matches_fp64(K, B, T, d, Q1, scaled):
    """vqw_f16x3_wgrad (the weight gradient of a causal dilated conv with two gradient sources, on the fp16 pipe with
    the operands split in registers) against an fp64 evaluation: taps that read before t = 0 (zero), shifts that are
    not multiples of 4 (16-byte windows straddling the row start), a dilation beyond the signal, guard scales, a T
    that is not a multiple of 64, accumulation into dw, run-to-run bitwise reproducibility."""
    Cp, Q0, ks = 256, 512, 3
    gen = torch.Generator().manual_seed(100 + d)
    p = torch.randn(B, Cp, T, generator=gen).to(DEV)
    q0 = (torch.randn(B, Q0, T, generator=gen) * (1e-6 if scaled else 1.0)).to(DEV)
    q1 = (torch.randn(B, Q1, T, generator=gen) * (3e-6 if scaled else 1.0)).to(DEV) if Q1 else None
    taps = [-(ks - 1 - j) * d for j in range(ks)]
    sc = torch.tensor([4.0, 2.0 ** 30, 2.0 ** 28] if scaled else [1.0, 1.0, 1.0], device=DEV)
    dw0 = torch.randn(ks, Cp, Q0 + Q1, generator=gen).to(DEV)
    slab = torch.empty(64 * 65536 * 4, device=DEV)

    def run():
        dw = dw0.clone()
        K.f16x3_wgrad(p=p, q0=q0, q1=q1, Q1=Q1, dw=dw, slab=slab, B=B, T=T, Cp=Cp, Q0=Q0, taps=taps,
                      p_scale=sc[0:1], q0_scale=sc[1:2], q1_scale=sc[2:3] if Q1 else None)
        return dw
    got = run()
    q = torch.cat([q0, q1], 1).double() if Q1 else q0.double()
    want = dw0.double().clone()
    for j, sh in enumerate(taps):
        ps = torch.zeros(B, Cp, T, dtype=torch.float64, device=DEV)
        if -sh < T:
            ps[:, :, -sh:] = p.double()[:, :, :T + sh]
        want[j] += torch.einsum('bct,bot->co', ps, q)
    upd = (want - dw0.double()).abs().max().item()
    err = (got.double() - want).abs().max().item()
    assert err <= 2e-6 * max(upd, 1e-30) + 1e-6 * dw0.abs().max().item(), 'max err %.3e of update %.3e' % (err, upd)
    assert torch.equal(run(), got), 'dw is not bitwise reproducible'
    # the sums of q that ride along: bias gradients (a column range) and the per-frame sums of add_condition's transpose
    Q = Q0 + Q1
    seg_T = T // 32
    bst = (Q + 5) * seg_T                                   # a batch stride wider than the rows written
    tot0 = torch.randn(Q, generator=gen).to(DEV)
    tot, seg = tot0.clone(), torch.zeros(B * bst, device=DEV)
    cols = (Q0, Q) if Q1 else (0, Q)
    K.f16x3_wgrad(p=p, q0=q0, q1=q1, Q1=Q1, dw=dw0.clone(), slab=slab, B=B, T=T, Cp=Cp, Q0=Q0, taps=taps, p_scale=sc[0:1],
                  q0_scale=sc[1:2], q1_scale=sc[2:3] if Q1 else None, q_total=tot, total_cols=cols, q_seg=seg, seg_T=seg_T,
                  seg_bstride=bst)
    want_tot = tot0.double().clone()
    want_tot[cols[0]:cols[1]] += q.sum((0, 2))[cols[0]:cols[1]]
    assert (tot.double() - want_tot).abs().max().item() <= 1e-5 * q.abs().sum((0, 2)).max().item() + 2e-6 * tot0.abs().max().item()   # tens of atomic adds into O(1) values
    want_seg = q.reshape(B, Q, seg_T, 32).sum(-1)
    got_seg = seg.view(B, Q + 5, seg_T)
    assert (got_seg[:, :Q].double() - want_seg).abs().max().item() <= 1e-5 * q.abs().max().item() * 32
    assert float(got_seg[:, Q:].abs().max()) == 0.0


@pytest.mark.parametrize('B,Tq,Tin,pl,scaled', [(2, 416, 832, 1, True), (3, 32, 64, 1, False), (1, 128, 255, 2, True), (3, 104, 208, 1, True), (8, 1664, 3328, 1, True)])
def test_wgrad_f16x3_stride2_matches_fp64(K, B, Tq, Tin, pl, scaled):
    """The encoder's strided convs (encoder.py:17-18, k=5 stride 2, SAME padding): dW[j][c][o] = sum p[b][c][2t + j - pl] q[b][o][t]
    with both paddings (2t + j - pl < 0 and >= T_in read zero), an odd input length, guard scales, the bias sum riding along;
    the last case is the benchmark's first 768 -> 768 layer."""
    Cp = Q0 = 768 if B == 8 else 256
    gen = torch.Generator().manual_seed(77 + Tq)
    p = torch.randn(B, Cp, Tin, generator=gen).to(DEV)
    q = (torch.randn(B, Q0, Tq, generator=gen) * (1e-6 if scaled else 1.0)).to(DEV)
    taps = [j - pl for j in range(5)]
    sc = torch.tensor([4.0, 2.0 ** 30] if scaled else [1.0, 1.0], device=DEV)
    dw0 = torch.randn(5, Cp, Q0, generator=gen).to(DEV) * (1e-6 if scaled else 1.0)
    slab = torch.empty(256 * 65536, device=DEV)
    tot0 = torch.randn(Q0, generator=gen).to(DEV) * (1e-4 if scaled else 1.0)

    def run():
        dw, tot = dw0.clone(), tot0.clone()
        K.f16x3_wgrad(p=p, q0=q, dw=dw, slab=slab, B=B, T=Tq, Cp=Cp, Q0=Q0, taps=taps, p_scale=sc[0:1], q0_scale=sc[1:2],
                      p_stride=2, T_p=Tin, q_total=tot)
        return dw, tot
    got, tot = run()
    assert torch.equal(run()[0], got), 'dw is not bitwise reproducible'
    if B == 8:        # against the fp32 engine's strided wgrad (fp64 over 78 GFLOP is too slow) + fp64 samples
        ref = dw0.clone()
        K.wgrad_gemm(p=p, q0=q, dw=ref, B=B, T_q=Tq, T_p=Tin, Cp=Cp, Q0=Q0, p_stride=2, taps=taps)
        upd = (ref - dw0).abs().max().item()
        assert (got - ref).abs().max().item() <= 2e-5 * upd
        for (j, c, o) in ((0, 3, 500), (1, 767, 0), (4, 100, 257), (2, 5, 5)):
            idx = 2 * torch.arange(Tq, device=DEV) + taps[j]
            ok = (idx >= 0) & (idx < Tin)
            w64 = (p[:, c, idx.clamp(0, Tin - 1)].double() * ok * q[:, o].double()).sum().item() + dw0[j, c, o].item()
            assert abs(got[j, c, o].item() - w64) <= 2e-6 * upd, (j, c, o)
    else:
        pd = torch.zeros(B, Cp, 2 * Tq + 8, dtype=torch.float64, device=DEV)      # p with its zero padding, index + pl
        pd[:, :, pl:pl + Tin] = p.double()
        want = dw0.double().clone()
        for j in range(5):
            want[j] += torch.einsum('bct,bot->co', pd[:, :, j:j + 2 * Tq:2], q.double())
        upd = (want - dw0.double()).abs().max().item()
        err = (got.double() - want).abs().max().item()
        assert err <= 2e-6 * upd + 1e-6 * dw0.abs().max().item(), 'max err %.3e of update %.3e' % (err, upd)
    want_tot = tot0.double() + q.double().sum((0, 2))
    assert (tot.double() - want_tot).abs().max().item() <= 1e-5 * q.abs().sum((0, 2)).max().item() + 2e-6 * tot0.abs().max().item()
    # the same gradient over the space-to-depth planes of p (what the forward conv reads) and the planes of q (what the input gradient
    # reads): tap j with e = j - pl is parity block e & 1 at row offset e >> 1 -- the same fp16 pieces, hence the same bits
    if Tin == 2 * Tq:          # (also where T_out is not a multiple of the 32-step pairs: 104 = encoder layer 5)
        pp = torch.empty(2 * B * Cp * Tin, dtype=torch.float16, device=DEV)
        qp = torch.empty(2 * B * Q0 * Tq, dtype=torch.float16, device=DEV)
        K.f16x3_split_activations(p, pp, B, Cp, Tin, scale_dev=sc[0:1], mode=K.X3_S2D)
        K.f16x3_split_activations(q, qp, B, Q0, Tq, scale_dev=sc[1:2])
        dw2, tot2 = dw0.clone(), tot0.clone()
        K.f16x3_wgrad(p_planes=pp, p_planes_KC=2 * Cp // 8, p_tap_chunk=[((j - pl) & 1) * (Cp // 8) for j in range(5)], q_planes=qp, dw=dw2,
                      slab=slab, B=B, T=Tq, Cp=Cp, Q0=Q0, taps=[(j - pl) >> 1 for j in range(5)], p_scale=sc[0:1], q0_scale=sc[1:2], q_total=tot2)
        assert torch.equal(dw2, got), 'strided weight gradient from planes differs from the fp32-operand launch'
        assert (tot2.double() - want_tot).abs().max().item() <= 1e-5 * q.abs().sum((0, 2)).max().item() + 2e-6 * tot0.abs().max().item()


@pytest.mark.parametrize('B,Tout,Cin,M', [(2, 128, 128, 128), (1, 256, 128, 256), (8, 96, 128, 128), (3, 104, 128, 128), (8, 1664, 768, 768)])
def test_strided_conv_f16x3_forward_and_input_gradient(K, B, Tout, Cin, M):
    """vqw_f16x3_strided_conv against torch's conv1d / its autograd in fp64 (encoder.py:17-18: k=5, stride 2, SAME = one zero in
    front, two behind; bias -> relu -> BatchNorm affine): column tiles that straddle batch rows (T = 96, 1664), a partial last column tile (3 x 104 = 312 columns), both paddings,
    operand scales on the device, the saved relu output; the last case is the benchmark's first 768 -> 768 layer (against the
    fp32 engine's kernels there)."""
    import torch.nn.functional as Fn
    ks, pl, Tin = 5, 1, 2 * Tout
    gen = torch.Generator().manual_seed(31 + Tout)
    x = torch.randn(B, Cin, Tin, generator=gen).to(DEV)
    w = (torch.randn(ks, Cin, M, generator=gen) * 0.05).to(DEV)
    bias, bsc, bsh = (torch.randn(M, generator=gen).to(DEV) * s_ for s_ in (0.5, 1.0, 0.3))
    sc = torch.tensor([8.0, 256.0, 2.0 ** 22], device=DEV)                 # x, w, dy
    xp = torch.empty(2 * B * Cin * Tin, dtype=torch.float16, device=DEV)
    wp = torch.empty(2 * ks * Cin * M, dtype=torch.float16, device=DEV)
    K.f16x3_split_activations(x, xp, B, Cin, Tin, scale_dev=sc[0:1], mode=K.X3_S2D)
    K.f16x3_pack_weights(w, wp, ks * Cin, M, M, 1.0, scale_dev=sc[1:2], mode=0)
    out, r = torch.empty(B, M, Tout, device=DEV), torch.empty(B, M, Tout, device=DEV)
    K.f16x3_strided_conv(xp=xp, wp=wp, out=out, save_r=r, B=B, T=Tout, Cin=Cin, M=M, ks=ks, pad_left=pl, bias=bias, bn_scale=bsc,
                         bn_shift=bsh, relu=True, x_scale=sc[0:1], w_scale=sc[1:2])
    big = B * Cin * Tin > (1 << 22)
    if big:
        want, want_r = torch.empty_like(out), torch.empty_like(r)
        K.conv_gemm(x0=x, w=w, bias=bias, out0=want, save0=want_r, scale=bsc, shift=bsh, B=B, T_in=Tin, T_out=Tout, M=M, C0=Cin,
                    in_stride=2, taps=[j - pl for j in range(ks)], out_relu=True)
    else:
        y = Fn.conv1d(Fn.pad(x.double(), (pl, ks - 2 - pl)), w.permute(2, 1, 0).double(), bias.double(), stride=2)
        want_r = torch.relu(y)
        want = bsc.double()[None, :, None] * want_r + bsh.double()[None, :, None]
    tol = 2e-5 if big else 3e-6
    assert (r.double() - want_r.double()).abs().max().item() <= tol * want_r.abs().max().item()
    assert (out.double() - want.double()).abs().max().item() <= tol * want.abs().max().item()
    # input gradient: dy [B][M][Tout] -> dx [B][Cin][Tin] through the transposed kernel wt[j][m][c]
    dy = (torch.randn(B, M, Tout, generator=gen) * 1e-4).to(DEV)
    wt = w.permute(0, 2, 1).contiguous()
    dyp = torch.empty(2 * B * M * Tout, dtype=torch.float16, device=DEV)
    wtp = torch.empty(2 * ks * M * Cin, dtype=torch.float16, device=DEV)
    K.f16x3_split_activations(dy, dyp, B, M, Tout, scale_dev=sc[2:3], mode=0)
    K.f16x3_pack_weights(wt, wtp, ks * M, Cin, Cin, 1.0, scale_dev=sc[1:2], mode=0)
    dx = torch.full((B, Cin, Tin), float('nan'), device=DEV)
    K.f16x3_strided_conv(xp=dyp, wp=wtp, out=dx, B=B, T=Tout, Cin=M, M=Cin, ks=ks, pad_left=pl, dgrad=True, x_scale=sc[2:3],
                         w_scale=sc[1:2])
    if big:
        want_dx = torch.empty_like(dx)
        for p in (0, 1):
            j0 = (p + pl) % 2
            js = list(range(j0, ks, 2))
            K.conv_gemm(x0=dy, w=wt[j0:], w_tap_stride=2 * M * Cin, out0=want_dx, B=B, T_in=Tout, T_out=(Tin - p + 1) // 2, M=Cin,
                        C0=M, taps=[(p + pl - j) // 2 for j in js], out_tstride=2, out_toffset=p, T_store=Tin)
    else:
        xd = x.double().requires_grad_(True)
        y = Fn.conv1d(Fn.pad(xd, (pl, ks - 2 - pl)), w.permute(2, 1, 0).double(), None, stride=2)
        want_dx, = torch.autograd.grad(y, xd, dy.double())
    assert torch.isfinite(dx).all()
    assert (dx.double() - want_dx.double()).abs().max().item() <= tol * want_dx.abs().max().item()


@pytest.mark.parametrize('B,Tout,Cin,M,shape,ksplit', [(3, 104, 256, 256, 2, 4), (2, 128, 256, 256, 0, 2), (1, 96, 256, 128, 2, 2),
                                                       (8, 104, 768, 768, 0, 0), (8, 208, 768, 768, 0, 0)])
def test_strided_conv_f16x3_split_k(K, B, Tout, Cin, M, shape, ksplit):
    """Split-K launches of vqw_f16x3_strided_conv (the short encoder layers: few tiles of many K steps): the K steps of a tile over
    several blocks, the output parities of the input gradient over separate blocks, partial tiles summed by the last block to arrive
    in a fixed order -- against fp64 (the fp32 engine at the benchmark's layers 4 and 5), bitwise equal from launch to launch, the
    ticket counters back at zero."""
    import torch.nn.functional as Fn
    ks, pl, Tin = 5, 1, 2 * Tout
    gen = torch.Generator().manual_seed(77 + Tout + ksplit)
    x = torch.randn(B, Cin, Tin, generator=gen).to(DEV)
    w = (torch.randn(ks, Cin, M, generator=gen) * 0.05).to(DEV)
    bias, bsc, bsh = (torch.randn(M, generator=gen).to(DEV) * s_ for s_ in (0.5, 1.0, 0.3))
    sc = torch.tensor([8.0, 256.0, 2.0 ** 22], device=DEV)
    xp = torch.empty(2 * B * Cin * Tin, dtype=torch.float16, device=DEV)
    wp = torch.empty(2 * ks * Cin * M, dtype=torch.float16, device=DEV)
    K.f16x3_split_activations(x, xp, B, Cin, Tin, scale_dev=sc[0:1], mode=K.X3_S2D)
    K.f16x3_pack_weights(w, wp, ks * Cin, M, M, 1.0, scale_dev=sc[1:2], mode=0)
    slab = torch.full((torch.cuda.get_device_properties(0).multi_processor_count * 65536,), float('nan'), device=DEV)
    cnt = torch.zeros(1024, dtype=torch.int32, device=DEV)
    outs = []
    for rep in range(2):
        out, r = torch.full((B, M, Tout), float('nan'), device=DEV), torch.full((B, M, Tout), float('nan'), device=DEV)
        K.f16x3_strided_conv(xp=xp, wp=wp, out=out, save_r=r, B=B, T=Tout, Cin=Cin, M=M, ks=ks, pad_left=pl, bias=bias, bn_scale=bsc,
                             bn_shift=bsh, relu=True, x_scale=sc[0:1], w_scale=sc[1:2], shape=shape, split_slab=slab, split_counters=cnt,
                             ksplit=ksplit)
        outs.append((out, r))
        assert int(cnt.abs().sum().item()) == 0, 'ticket counters not back at zero'
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), 'split-K forward differs from launch to launch'
    out, r = outs[0]
    big = Cin >= 768
    if big:
        want, want_r = torch.empty_like(out), torch.empty_like(r)
        K.conv_gemm(x0=x, w=w, bias=bias, out0=want, save0=want_r, scale=bsc, shift=bsh, B=B, T_in=Tin, T_out=Tout, M=M, C0=Cin,
                    in_stride=2, taps=[j - pl for j in range(ks)], out_relu=True)
    else:
        y = Fn.conv1d(Fn.pad(x.double(), (pl, ks - 2 - pl)), w.permute(2, 1, 0).double(), bias.double(), stride=2)
        want_r = torch.relu(y)
        want = bsc.double()[None, :, None] * want_r + bsh.double()[None, :, None]
    tol = 2e-5 if big else 3e-6
    assert torch.isfinite(out).all() and torch.isfinite(r).all()
    assert (r.double() - want_r.double()).abs().max().item() <= tol * want_r.abs().max().item()
    assert (out.double() - want.double()).abs().max().item() <= tol * want.abs().max().item()
    dy = (torch.randn(B, M, Tout, generator=gen) * 1e-4).to(DEV)
    wt = w.permute(0, 2, 1).contiguous()
    dyp = torch.empty(2 * B * M * Tout, dtype=torch.float16, device=DEV)
    wtp = torch.empty(2 * ks * M * Cin, dtype=torch.float16, device=DEV)
    K.f16x3_split_activations(dy, dyp, B, M, Tout, scale_dev=sc[2:3], mode=0)
    K.f16x3_pack_weights(wt, wtp, ks * M, Cin, Cin, 1.0, scale_dev=sc[1:2], mode=0)
    dxs = []
    for rep in range(2):
        dx = torch.full((B, Cin, Tin), float('nan'), device=DEV)
        K.f16x3_strided_conv(xp=dyp, wp=wtp, out=dx, B=B, T=Tout, Cin=M, M=Cin, ks=ks, pad_left=pl, dgrad=True, x_scale=sc[2:3],
                             w_scale=sc[1:2], shape=shape, split_slab=slab, split_counters=cnt, ksplit=ksplit)
        dxs.append(dx)
        assert int(cnt.abs().sum().item()) == 0
    assert torch.equal(dxs[0], dxs[1]), 'split-K input gradient differs from launch to launch'
    dx = dxs[0]
    if big:
        want_dx = torch.empty_like(dx)
        for p in (0, 1):
            j0 = (p + pl) % 2
            js = list(range(j0, ks, 2))
            K.conv_gemm(x0=dy, w=wt[j0:], w_tap_stride=2 * M * Cin, out0=want_dx, B=B, T_in=Tout, T_out=(Tin - p + 1) // 2, M=Cin,
                        C0=M, taps=[(p + pl - j) // 2 for j in js], out_tstride=2, out_toffset=p, T_store=Tin)
    else:
        xd = x.double().requires_grad_(True)
        y = Fn.conv1d(Fn.pad(xd, (pl, ks - 2 - pl)), w.permute(2, 1, 0).double(), None, stride=2)
        want_dx, = torch.autograd.grad(y, xd, dy.double())
    assert torch.isfinite(dx).all()
    assert (dx.double() - want_dx.double()).abs().max().item() <= tol * want_dx.abs().max().item()


@pytest.mark.parametrize('B,Cc,Mall,Tz', [(8, 80, 15872, 104), (3, 24, 1000, 12), (2, 128, 320, 132), (1, 1, 64, 4), (5, 33, 36, 200)])
def test_condition_projection_kernels(K, B, Cc, Mall, Tz):
    """vqw_cond_proj_fwd / _wgrad / _dgrad (add_condition's 1x1 conv of every layer in one matrix, wavenet_ops.py:93-101) against
    fp64: the benchmark's shape, channel counts that are not multiples of the 32-row MFMA tiles, frame rows shorter and longer than
    the 128-frame pass, an odd batch (the weight gradient's two batch ranges are unequal), the smallest shape.  Exact fp32 products
    (v_mfma_f32_32x32x2_f32): the bars are those of an fp32 sum of that length.  Forward and input gradient are reproducible bit for
    bit; the weight gradient accumulates into dw."""
    gen = torch.Generator().manual_seed(Cc * 7 + Tz)
    cond = torch.randn(B, Cc, Tz, generator=gen).to(DEV)
    w = (torch.randn(Cc, Mall, generator=gen) * 0.3).to(DEV)
    dce = torch.randn(B, Mall, Tz, generator=gen).to(DEV)
    out = torch.full((B, Mall, Tz), float('nan'), device=DEV)
    K.cond_proj_fwd(cond, w, out, B=B, Cc=Cc, Mall=Mall, Tz=Tz)
    want = torch.einsum('cm,bct->bmt', w.double(), cond.double())
    assert (out.double() - want).abs().max().item() <= 2e-6 * want.abs().max().item()
    dw = torch.zeros(Cc, Mall, device=DEV)
    K.cond_proj_wgrad(cond, dce, dw, B=B, Cc=Cc, Mall=Mall, Tz=Tz)
    want_dw = torch.einsum('bct,bmt->cm', cond.double(), dce.double())
    assert (dw.double() - want_dw).abs().max().item() <= 3e-6 * want_dw.abs().max().item()
    K.cond_proj_wgrad(cond, dce, dw, B=B, Cc=Cc, Mall=Mall, Tz=Tz)           # accumulates
    assert (dw.double() - 2 * want_dw).abs().max().item() <= 6e-6 * want_dw.abs().max().item()
    scratch = torch.full((K.cond_proj_dgrad_scratch(B, Cc, Mall, Tz),), float('nan'), device=DEV)
    dcond = torch.full((B, Cc, Tz), float('nan'), device=DEV)
    K.cond_proj_dgrad(w, dce, dcond, scratch, B=B, Cc=Cc, Mall=Mall, Tz=Tz)
    want_dc = torch.einsum('cm,bmt->bct', w.double(), dce.double())
    assert (dcond.double() - want_dc).abs().max().item() <= 1e-5 * want_dc.abs().max().item()
    out2, dcond2 = torch.empty_like(out), torch.empty_like(dcond)
    K.cond_proj_fwd(cond, w, out2, B=B, Cc=Cc, Mall=Mall, Tz=Tz)
    K.cond_proj_dgrad(w, dce, dcond2, scratch, B=B, Cc=Cc, Mall=Mall, Tz=Tz)
    assert torch.equal(out, out2) and torch.equal(dcond, dcond2)


@pytest.mark.parametrize('mode', [0, 1])
def test_pack_weights_from_transposed_storage(K, mode):
    """vqw_f16x3_pack_weights_t: the planes of the input-gradient kernels straight from the forward kernels (tap-wise transposed
    blocks, a row stride wider than the rows used, several matrices per launch) are bit-equal to vqw_f16x3_pack_weights of an
    explicit transposed copy."""
    gen = torch.Generator().manual_seed(5)
    Lc, ks, Cin, Cout = 3, 3, 64, 128
    w = torch.randn(Lc, ks, Cin, Cout, generator=gen).to(DEV)                      # [layer][tap][cin][cout]
    sc = torch.tensor([4.0], device=DEV)
    wt = w.permute(0, 1, 3, 2).contiguous()                                        # [layer][tap][cout][cin]
    n = Lc * 2 * ks * Cout * Cin
    want, got = torch.zeros(n, dtype=torch.float16, device=DEV), torch.zeros(n, dtype=torch.float16, device=DEV)
    K.f16x3_pack_weights(wt, want, ks * Cout, Cin, Cin, 2.0, count=Lc, scale_dev=sc, mode=mode)
    K.f16x3_pack_weights_t(w, got, ks * Cout, Cin, Cout, Cout, Cin * Cout, 2.0, count=Lc, scale_dev=sc, mode=mode)
    assert torch.equal(want.view(torch.int16), got.view(torch.int16))
    # one matrix, only the first 64 of its 128 stored columns (the top layer's skip half: ld_src > k_inner)
    w2 = torch.randn(Cin, Cout, generator=gen).to(DEV)
    n2 = 2 * 64 * Cin
    want2, got2 = torch.zeros(n2, dtype=torch.float16, device=DEV), torch.zeros(n2, dtype=torch.float16, device=DEV)
    K.f16x3_pack_weights(w2.t().contiguous(), want2, 64, Cin, Cin, 1.0, mode=mode)
    K.f16x3_pack_weights_t(w2, got2, 64, Cin, 64, Cout, 0, 1.0, mode=mode)
    assert torch.equal(want2.view(torch.int16), got2.view(torch.int16))
    # blocks of k that are not multiples of 64 (the direct kernel instead of the LDS-transposing one), M not a multiple of 64
    w3 = torch.randn(2, 72, 40, generator=gen).to(DEV)                            # [tap][m = 72][k_inner = 40]
    n3 = 2 * 80 * 72
    want3, got3 = torch.zeros(n3, dtype=torch.float16, device=DEV), torch.zeros(n3, dtype=torch.float16, device=DEV)
    K.f16x3_pack_weights(w3.permute(0, 2, 1).contiguous(), want3, 80, 72, 72, 1.0, mode=mode)
    K.f16x3_pack_weights_t(w3, got3, 80, 72, 40, 40, 72 * 40, 1.0, mode=mode)
    assert torch.equal(want3.view(torch.int16), got3.view(torch.int16))
    w4 = torch.randn(72, 128, generator=gen).to(DEV)                              # tile kernel with a partial column tile (M = 72)
    n4 = 2 * 128 * 72
    want4, got4 = torch.zeros(n4, dtype=torch.float16, device=DEV), torch.zeros(n4, dtype=torch.float16, device=DEV)
    K.f16x3_pack_weights(w4.t().contiguous(), want4, 128, 72, 72, 1.0, mode=mode)
    K.f16x3_pack_weights_t(w4, got4, 128, 72, 128, 128, 0, 1.0, mode=mode)
    assert torch.equal(want4.view(torch.int16), got4.view(torch.int16))


@pytest.mark.parametrize('half', [0, 1])
def test_head_conv_f16x3_epilogue_options(K, half):
    """vqw_f16x3_out_conv epi 2 (the 1x1 convs around the stack and their input gradients): mask * (net_in + W x + bias + upsampled
    condition) in place over the mask source, relu'd planes with their max-abs report -- against fp64."""
    B, T, Cin, M, Tz = 2, 512, 512, 256, 8
    gen = torch.Generator().manual_seed(41)
    x = torch.randn(B, Cin, T, generator=gen).to(DEV)
    w = (torch.randn(Cin, M, generator=gen) * 0.05).to(DEV)
    bias = torch.randn(M, generator=gen).to(DEV)
    cond = torch.randn(B, M + 3, Tz, generator=gen).to(DEV)            # batch stride wider than the rows read
    ni = torch.randn(B, M, T, generator=gen).to(DEV)
    mask_src = torch.randn(B, M, T, generator=gen).to(DEV)
    sc = torch.tensor([4.0, 64.0, 16.0], device=DEV)
    md = K.X3_HALF_BLOCKS if half else 0
    xp = torch.empty(2 * B * Cin * T, dtype=torch.float16, device=DEV)
    wp = torch.empty(2 * Cin * M, dtype=torch.float16, device=DEV)
    K.f16x3_split_activations(x, xp, B, Cin, T, scale_dev=sc[0:1], mode=md)
    K.f16x3_pack_weights(w, wp, Cin, M, M, 1.0, scale_dev=sc[1:2], mode=md)
    lin = torch.einsum('cm,bct->bmt', w.double(), x.double()) + bias.double()[None, :, None]
    up = cond[:, :M].double().repeat_interleave(T // Tz, dim=2)
    want = (mask_src > 0).double() * (ni.double() + lin + up)
    out = mask_src.clone()                                             # in place over the mask source
    planes = torch.zeros(2 * B * M * T, dtype=torch.float16, device=DEV)
    amax, flag = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    K.f16x3_out_conv(epi=2, xp=xp, Cin=Cin, wp=wp, bias=bias, net_in=ni, net_out=out, aux0=out, cond=cond, cond_T=Tz,
                     cond_bstride=(M + 3) * Tz, net_out_planes=planes, relu_planes=True, B=B, T=T, R=M, S=0, w_scale_inv=1.0,
                     x_scale=sc[0:1], w_scale=sc[1:2], out_scale=sc[2:3], out_amax=amax, flag=flag, mode=md)
    assert (out.double() - want).abs().max().item() <= 3e-6 * want.abs().max().item()
    pl = planes.view(2, M // 8, B * T, 8).double().sum(0) / 16.0       # [chunk][row][8] -> [B][M][T]
    got_p = pl.permute(1, 0, 2).reshape(B, T, M).permute(0, 2, 1)
    assert (got_p - torch.relu(want)).abs().max().item() <= 3e-6 * want.abs().max().item()
    assert abs(amax.view(torch.float32).item() - torch.relu(want).max().item()) <= 1e-5 * want.abs().max().item()
    assert flag.item() == 0
    # plain form: no mask, no net_in, no condition, planes without relu
    out2 = torch.empty(B, M, T, device=DEV)
    K.f16x3_out_conv(epi=2, xp=xp, Cin=Cin, wp=wp, bias=bias, net_out=out2, net_out_planes=planes, B=B, T=T, R=M, S=0,
                     w_scale_inv=1.0, x_scale=sc[0:1], w_scale=sc[1:2], out_scale=sc[2:3], mode=md)
    assert (out2.double() - lin).abs().max().item() <= 3e-6 * lin.abs().max().item()
    pl = planes.view(2, M // 8, B * T, 8).double().sum(0) / 16.0
    assert (pl.permute(1, 0, 2).reshape(B, T, M).permute(0, 2, 1) - lin).abs().max().item() <= 3e-6 * lin.abs().max().item()


def test_wgrad_f16x3_relu_operand(K):
    """p_relu: the weight gradient of a conv that sits behind a relu (wavenet.py:79, 93) reads max(p, 0)."""
    B, T, Cp, Q0 = 2, 512, 512, 256
    gen = torch.Generator().manual_seed(43)
    p = torch.randn(B, Cp, T, generator=gen).to(DEV)
    q = (torch.randn(B, Q0, T, generator=gen) * 1e-5).to(DEV)
    sc = torch.tensor([8.0, 2.0 ** 26], device=DEV)
    dw = torch.zeros(Cp, Q0, device=DEV)
    slab = torch.empty(256 * 65536, device=DEV)
    K.f16x3_wgrad(p=p, q0=q, dw=dw, slab=slab, B=B, T=T, Cp=Cp, Q0=Q0, taps=[0], p_scale=sc[0:1], q0_scale=sc[1:2], p_relu=True)
    want = torch.einsum('bct,bot->co', torch.relu(p).double(), q.double())
    assert (dw.double() - want).abs().max().item() <= 2e-6 * want.abs().max().item()


@pytest.mark.parametrize('half', [0, 1])
def test_gate_backward_f16x3_from_tanh_or_from_gated(K, half):
    """vqw_f16x3_out_conv epi 1 against fp64: dpre = {dg sg (1 - th^2), dg th sg (1 - sg)}, dg = W^T [dskip; dnet]; with aux0 = tanh
    (saved by the forward pass) and with aux0 = tanh * sigmoid (a forward pass that did not store tanh), including sigmoids that
    underflowed to zero."""
    B, T, R, S = 2, 512, 256, 256
    gen = torch.Generator().manual_seed(51)
    dcat = (torch.randn(B, S + R, T, generator=gen) * 1e-5).to(DEV)
    w = (torch.randn(S + R, R, generator=gen) * 0.05).to(DEV)
    xf, xg = torch.randn(B, R, T, generator=gen).to(DEV) * 2, torch.randn(B, R, T, generator=gen).to(DEV) * 3
    xg[:, ::7, ::5] = -200.0                                              # sigmoid == 0 exactly
    xg[:, 3::7, 1::5] = -88.0                                             # sigmoid = 6e-39: DENORMAL (v_rcp_f32 of it is inf, g^2 is 0)
    xg[:, 5::7, 2::5] = -87.0                                             # 1.6e-38: the smallest normal numbers
    th, sg = torch.tanh(xf), torch.sigmoid(xg)
    assert 0 < float(sg[:, 3::7, 1::5].max()) < 1.1754944e-38
    gated = th * sg
    md = K.X3_HALF_BLOCKS if half else 0
    sc = torch.tensor([2.0 ** 28, 64.0, 2.0 ** 26], device=DEV)
    gr = torch.empty(2 * B * (S + R) * T, dtype=torch.float16, device=DEV)
    wp = torch.empty(2 * (S + R) * R, dtype=torch.float16, device=DEV)
    K.f16x3_split_activations(dcat, gr, B, S + R, T, scale_dev=sc[0:1], mode=md)
    K.f16x3_pack_weights(w, wp, S + R, R, R, 1.0, scale_dev=sc[1:2], mode=md)
    dg = torch.einsum('kc,bkt->bct', w.double(), dcat.double())
    want = torch.cat([dg * sg.double() * (1 - th.double() ** 2), dg * th.double() * sg.double() * (1 - sg.double())], 1)
    # the gated output once more as the planes the forward gate conv writes, inside a wider planes tensor (3 layers side by side)
    gpl = torch.zeros(2 * B * 3 * R * T, dtype=torch.float16, device=DEV)
    K.f16x3_split_activations(gated, gpl, B, R, T, kc0=R // 8, KC=3 * (R // 8), mode=md)
    for aux0, flag_g, from_planes in ((th, False, False), (gated, True, False), (None, True, True)):
        dpre = torch.empty(B, 2 * R, T, device=DEV)
        planes = torch.empty(2 * B * 2 * R * T, dtype=torch.float16, device=DEV)
        K.f16x3_out_conv(epi=1, xp=gr, Cin=S + R, wp=wp, aux0=aux0, aux1=sg, net_out=dpre, net_out_planes=planes, B=B, T=T, R=R, S=0,
                         w_scale_inv=1.0, x_scale=sc[0:1], w_scale=sc[1:2], out_scale=sc[2:3], aux0_is_gated=flag_g, mode=md,
                         **(dict(aux0_planes=gpl, aux0_KC=3 * (R // 8), aux0_kc0=R // 8) if from_planes else {}))
        assert torch.isfinite(dpre).all()
        err = (dpre.double() - want).abs().max().item() / want.abs().max().item()
        assert err <= (3e-6 if from_planes else (2e-6 if flag_g else 1e-6)), 'aux0 %s: %.3e of max' % ('gated' if flag_g else 'tanh', err)
        pl = planes.view(2, 2 * R // 8, B * T, 8).double().sum(0) / 2.0 ** 26
        got_p = pl.permute(1, 0, 2).reshape(B, T, 2 * R).permute(0, 2, 1)
        assert (got_p - want).abs().max().item() <= 4e-6 * want.abs().max().item()
        if from_planes:      # planes only: gate backward need not write fp32 dpre at all
            planes2 = torch.empty_like(planes)
            K.f16x3_out_conv(epi=1, xp=gr, Cin=S + R, wp=wp, aux1=sg, net_out=None, net_out_planes=planes2, B=B, T=T, R=R, S=0,
                             w_scale_inv=1.0, x_scale=sc[0:1], w_scale=sc[1:2], out_scale=sc[2:3], aux0_is_gated=True, mode=md,
                             aux0_planes=gpl, aux0_KC=3 * (R // 8), aux0_kc0=R // 8)
            assert torch.equal(planes2, planes)


def test_wgrad_f16x3_batch_of_layers_in_one_launch(K):
    """vqw_f16x3_wgrad_batch: the gate-kernel gradients of five layers (different dilations, operands, scales, outputs, condition
    sums) in ONE launch against the five single launches and fp64 samples; the residual-half form (dw a column block of a wider
    matrix, bias sums); bitwise reproducible from run to run."""
    B, T, R, S, Tz = 2, 2048, 256, 512, 32
    gen = torch.Generator().manual_seed(19)
    dils = [4, 8, 64, 256, 512]
    nets = [torch.randn(B, R, T, generator=gen).to(DEV) for _ in dils]
    dpres = [(torch.randn(B, 2 * R, T, generator=gen) * 1e-5).to(DEV) for _ in dils]
    scales = torch.tensor([2.0 ** 9, 2.0 ** 10, 2.0 ** 11, 2.0 ** 10, 2.0 ** 9, 2.0 ** 27, 2.0 ** 26, 2.0 ** 27, 2.0 ** 28, 2.0 ** 27], device=DEV)
    slab = torch.empty(256 * 65536, device=DEV)

    def run(batched):
        dws = [torch.zeros(3, R, 2 * R, device=DEV) for _ in dils]
        segs = [torch.zeros(B, 2 * R, Tz, device=DEV) for _ in dils]
        probs = [dict(p=nets[i], q0=dpres[i], dw=dws[i], taps=[-2 * d, -d, 0], p_scale=scales[i:i + 1], q0_scale=scales[5 + i:6 + i],
                      q_seg=segs[i]) for i, d in enumerate(dils)]
        common = dict(slab=slab, B=B, T=T, Cp=R, Q0=2 * R, seg_T=Tz)
        if batched:
            K.f16x3_wgrad_batch(probs, **common)
        else:
            for pr in probs:
                K.f16x3_wgrad(**dict(common, **pr))
        return dws, segs
    one, seg1 = run(False)
    bat, segb = run(True)
    bat2, _ = run(True)
    for i, d in enumerate(dils):
        close(bat[i], one[i], rtol=2e-6, atol=2e-6, what='batched gate wgrad, layer %d' % i)     # other K ranges: not bit-equal
        assert torch.equal(bat[i], bat2[i]), 'batched dW is not reproducible'
        close(segb[i], dpres[i].view(B, 2 * R, Tz, T // Tz).sum(-1), rtol=1e-4, atol=1e-4, what='condition sums, layer %d' % i)
        for (j, c, o) in ((0, 3, 500), (1, 255, 0), (2, 100, 257)):
            sh = (2 - j) * d
            w64 = (nets[i][:, c, :T - sh].double() * dpres[i][:, o, sh:].double()).sum().item()
            assert abs(bat[i][j, c, o].item() - w64) <= 2e-6 * bat[i].abs().max().item(), (i, j, c, o)
    # q as operand planes (what gate backward writes for the input gradient anyway) instead of fp32: the transposed LDS reads hand
    # the MFMA the SAME fp16 pieces the in-register split makes -> dW bit-equal to the fp32-operand launch; the condition sums are
    # formed from the planes (2^-22 relative)
    for bf in (False, True):
        md = K.X3_BF16 if bf else 0
        planes = [torch.empty(2 * B * 2 * R * T, dtype=torch.float16, device=DEV) for _ in dils]
        for i in range(len(dils)):
            K.f16x3_split_activations(dpres[i], planes[i], B, 2 * R, T, scale_dev=scales[5 + i:6 + i], mode=md)
        res = {}
        for qp in (False, True):
            dws = [torch.zeros(3, R, 2 * R, device=DEV) for _ in dils]
            segs = [torch.zeros(B, 2 * R, Tz, device=DEV) for _ in dils]
            tots = [torch.zeros(2 * R, device=DEV) for _ in dils]
            probs = [dict(p=nets[i], dw=dws[i], taps=[-2 * d, -d, 0], p_scale=scales[i:i + 1], q0_scale=scales[5 + i:6 + i], q_seg=segs[i],
                          q_total=tots[i], **(dict(q_planes=planes[i]) if qp else dict(q0=dpres[i]))) for i, d in enumerate(dils)]
            K.f16x3_wgrad_batch(probs, slab=slab, B=B, T=T, Cp=R, Q0=2 * R, seg_T=Tz, mode=md)
            res[qp] = (dws, segs, tots)
        for i in range(len(dils)):
            assert torch.equal(res[True][0][i], res[False][0][i]), 'q from planes: dW of layer %d differs (bf16=%s)' % (i, bf)
            if bf:
                # One bf16 plane: the sums formed from the planes are sums of the ROUNDED q, the sums formed from fp32 q are taken
                # before it is rounded (include/vqwave.h, q_total) -- each against its own float64 sum, in the bound form of
                # test_wgrad_f16x3_matches_fp64 (per column 1e-5 sum |q|; 1e-5 * 32 max |q| per 32 steps of a segment).  The sums
                # are of order 6e-4 and 8e-5: a tolerance of the old 3e-3 passed an all-zero output.
                sq = float(scales[5 + i])
                q_r = torch.from_numpy(X.bf16_round(X.scaled(dpres[i].cpu().numpy(), sq))).to(DEV) / sq
                for qp, q64 in ((False, dpres[i].double()), (True, q_r)):
                    tot_err = (res[qp][2][i].double() - q64.sum((0, 2))).abs()
                    assert bool((tot_err <= 1e-5 * q64.abs().sum((0, 2))).all()), 'bias sums (q planes: %s), layer %d: %.3e' % (qp, i, float(tot_err.max()))
                    seg_err = float((res[qp][1][i].double() - q64.view(B, 2 * R, Tz, T // Tz).sum(-1)).abs().max())
                    assert seg_err <= 1e-5 * float(q64.abs().max()) * 32 * (T // Tz // 32), 'condition sums (q planes: %s), layer %d: %.3e' % (qp, i, seg_err)
                d, sp = dils[i], float(scales[i])
                for (j, c, o) in ((0, 3, 500), (1, 255, 0), (2, 100, 257)):       # dW against float64 of the rounded operands
                    sh = (2 - j) * d
                    p_r = X.bf16_round(X.scaled(nets[i][:, c, :T - sh].cpu().numpy(), sp)) / sp
                    w64 = float((p_r * q_r[:, o, sh:].cpu().numpy()).sum())
                    assert abs(res[True][0][i][j, c, o].item() - w64) <= 2e-6 * res[True][0][i].abs().max().item(), (i, j, c, o)
                continue
            for qp in (False, True):
                close(res[qp][2][i], dpres[i].sum((0, 2)), rtol=1e-4, atol=1e-6, what='bias sums (q planes: %s), layer %d' % (qp, i))
            close(res[True][1][i], dpres[i].view(B, 2 * R, Tz, T // Tz).sum(-1), rtol=1e-4, atol=1e-4,
                  what='condition sums from planes, layer %d' % i)
    # odd dilations (unaligned windows of p) with q from planes
    dwa, dwb = torch.zeros(3, R, 2 * R, device=DEV), torch.zeros(3, R, 2 * R, device=DEV)
    pl0 = torch.empty(2 * B * 2 * R * T, dtype=torch.float16, device=DEV)
    K.f16x3_split_activations(dpres[0], pl0, B, 2 * R, T, scale_dev=scales[5:6])
    K.f16x3_wgrad(p=nets[0], q0=dpres[0], dw=dwa, slab=slab, B=B, T=T, Cp=R, Q0=2 * R, taps=[-2, -1, 0], p_scale=scales[0:1], q0_scale=scales[5:6])
    K.f16x3_wgrad(p=nets[0], q_planes=pl0, dw=dwb, slab=slab, B=B, T=T, Cp=R, Q0=2 * R, taps=[-2, -1, 0], p_scale=scales[0:1], q0_scale=scales[5:6])
    assert torch.equal(dwa, dwb)
    w64 = (nets[0][:, 7, :T - 1].double() * dpres[0][:, 300, 1:].double()).sum().item()
    assert abs(dwb[1, 7, 300].item() - w64) <= 2e-6 * dwb.abs().max().item()
    # p as planes too (the layer-input planes of the forward pass): a shift is a row offset, also where it is not a multiple of 4;
    # all four operand combinations give the same bits
    npl = torch.empty(2 * B * R * T, dtype=torch.float16, device=DEV)
    K.f16x3_split_activations(nets[0], npl, B, R, T, scale_dev=scales[0:1])
    for taps in ([-2, -1, 0], [-16, -8, 0], [-1024, -512, 0]):
        ref = torch.zeros(3, R, 2 * R, device=DEV)
        K.f16x3_wgrad(p=nets[0], q0=dpres[0], dw=ref, slab=slab, B=B, T=T, Cp=R, Q0=2 * R, taps=taps, p_scale=scales[0:1], q0_scale=scales[5:6])
        for qp in (False, True):
            got = torch.zeros(3, R, 2 * R, device=DEV)
            seg = torch.zeros(B, 2 * R, Tz, device=DEV)
            K.f16x3_wgrad(p_planes=npl, dw=got, slab=slab, B=B, T=T, Cp=R, Q0=2 * R, taps=taps, p_scale=scales[0:1], q0_scale=scales[5:6],
                          q_seg=seg, seg_T=Tz, **(dict(q_planes=pl0) if qp else dict(q0=dpres[0])))
            assert torch.equal(got, ref), 'p from planes (q from planes: %s), taps %s' % (qp, taps)
            close(seg, dpres[0].view(B, 2 * R, Tz, T // Tz).sum(-1), rtol=1e-4, atol=1e-4, what='condition sums')
    # p planes inside a wider planes tensor (the gated planes of all layers side by side), batched
    gall = torch.empty(2 * B * 3 * R * T, dtype=torch.float16, device=DEV)
    gs = [torch.randn(B, R, T, generator=gen).to(DEV) * 0.3 for _ in range(3)]
    for i in range(3):
        K.f16x3_split_activations(gs[i], gall, B, R, T, kc0=i * (R // 8), KC=3 * (R // 8))
    dsk = (torch.randn(B, S, T, generator=gen) * 1e-5).to(DEV)
    a_ = [torch.zeros(R, S + R, device=DEV) for _ in range(3)]
    b_ = [torch.zeros(R, S + R, device=DEV) for _ in range(3)]
    K.f16x3_wgrad_batch([dict(p=gs[i], dw=a_[i].view(-1)) for i in range(3)], q0=dsk, slab=slab, B=B, T=T, Cp=R, Q0=S, lddw=S + R,
                        taps=[0], q0_scale=scales[6:7])
    K.f16x3_wgrad_batch([dict(p_planes=gall, p_planes_kc0=i * (R // 8), dw=b_[i].view(-1)) for i in range(3)], p_planes_KC=3 * (R // 8),
                        q0=dsk, slab=slab, B=B, T=T, Cp=R, Q0=S, lddw=S + R, taps=[0], q0_scale=scales[6:7])
    for i in range(3):
        assert torch.equal(a_[i], b_[i])
    # residual halves: dW_r[l] = gated[l] (x) dnet[l+1] into columns S.. of [R][S+R], bias sums of dnet
    gated = [torch.randn(B, R, T, generator=gen).to(DEV) * 0.3 for _ in range(3)]
    dnets = [(torch.randn(B, R, T, generator=gen) * 3e-5).to(DEV) for _ in range(3)]
    dwo = [torch.zeros(R, S + R, device=DEV) for _ in range(3)]
    tot = [torch.zeros(R, device=DEV) for _ in range(3)]
    K.f16x3_wgrad_batch([dict(p=gated[i], q0=dnets[i], dw=dwo[i].view(-1)[S:], q_total=tot[i]) for i in range(3)], slab=slab, B=B, T=T,
                        Cp=R, Q0=R, lddw=S + R, taps=[0], q0_scale=scales[6:7], total_cols=(0, R))
    for i in range(3):
        want = torch.einsum('bct,bot->co', gated[i].double(), dnets[i].double())
        assert float(dwo[i][:, :S].abs().max()) == 0.0
        assert float((dwo[i][:, S:].double() - want).abs().max()) <= 2e-6 * float(want.abs().max())
        close(tot[i], dnets[i].sum((0, 2)), rtol=1e-4, atol=1e-7, what='bias sums')
    with pytest.raises(RuntimeError, match='differs from problem 0'):
        K.f16x3_wgrad_batch([dict(p=nets[0], q0=dpres[0], dw=dws, taps=t_) for dws, t_ in ((one[0], [-8, -4, 0]), (one[1][:2], [-4, 0]))],
                            slab=slab, B=B, T=T, Cp=R, Q0=2 * R)


def test_wgrad_f16x3_full_size_matches_fp32_engine(K):
    """The benchmark's shapes (B=8, T=6656: 1664 stage pairs over 42 / 85 K splits): gate-conv and 1x1 weight gradients
    against the fp32 engine's wgrad kernel and fp64 samples."""
    B, T, R, S = 8, 6656, 256, 512
    gen = torch.Generator().manual_seed(9)
    net = torch.randn(B, R, T, generator=gen).to(DEV)
    dpre = (torch.randn(B, 2 * R, T, generator=gen) * 1e-5).to(DEV)
    dskip = (torch.randn(B, S, T, generator=gen) * 1e-5).to(DEV)
    dnet = (torch.randn(B, R, T, generator=gen) * 3e-5).to(DEV)
    slab = torch.empty(256 * 65536, device=DEV)
    sc = torch.tensor([2.0 ** 10, 2.0 ** 27, 2.0 ** 26], device=DEV)
    for d in (1, 64, 512):
        taps = [-2 * d, -d, 0]
        dw = torch.zeros(3, R, 2 * R, device=DEV)
        K.f16x3_wgrad(p=net, q0=dpre, dw=dw, slab=slab, B=B, T=T, Cp=R, Q0=2 * R, taps=taps, p_scale=sc[0:1], q0_scale=sc[1:2])
        ref = torch.zeros_like(dw)
        K.wgrad_gemm(p=net, q0=dpre, dw=ref, B=B, T_q=T, T_p=T, Cp=R, Q0=2 * R, taps=taps)
        close(dw, ref, rtol=2e-5, atol=2e-5, what='gate wgrad d=%d vs the fp32 engine' % d)
        for (j, c, o) in ((0, 3, 500), (1, 255, 0), (2, 100, 257)):
            sh = -taps[j]
            w64 = (net[:, c, :T - sh].double() * dpre[:, o, sh:].double()).sum().item()
            assert abs(dw[j, c, o].item() - w64) <= 2e-6 * dw.abs().max().item(), (d, j, c, o)
    dw = torch.zeros(R, S + R, device=DEV)
    K.f16x3_wgrad(p=net, q0=dskip, q1=dnet, Q1=R, dw=dw, slab=slab, B=B, T=T, Cp=R, Q0=S, taps=[0], p_scale=sc[0:1],
                  q0_scale=sc[1:2], q1_scale=sc[2:3])
    ref = torch.zeros_like(dw)
    K.wgrad_gemm(p=net, q0=dskip, q1=dnet, dw=ref, B=B, T_q=T, T_p=T, Cp=R, Q0=S, Q1=R, lddw=S + R, taps=[0])
    close(dw, ref, rtol=2e-5, atol=2e-5, what='1x1 wgrad vs the fp32 engine')


def test_accum_split_and_two_sources(K):
    B, T, Cg, S, Rr = 2, 512, 32, 64, 32
    gated, w, b = rnd(B, T, Cg, seed=1), rnd(Cg, S + Rr, seed=2, s=0.2), rnd(S + Rr, seed=3)
    skip0, net0 = rnd(B, T, S, seed=4), rnd(B, T, Rr, seed=5)
    want = gated @ w + b
    skip = bct(skip0); net_in = bct(net0); net_out = torch.empty_like(net_in)
    K.conv_gemm(x0=bct(gated), w=g(w), bias=g(b), out0=skip, out1=net_out, aux1=net_in, B=B, T_in=T, T_out=T,
                M=S + Rr, M0=S, C0=Cg, taps=[0], epilogue=K.EPI_ACCUM_SPLIT)
    close(btc(skip), skip0 + want[..., :S], what='skip +=')
    close(btc(net_out), net0 + want[..., S:], what='net = net + res')
    # dgated = [dskip; dnet] x Wcat^T with the two sources concatenated along K, gate backward epilogue
    dskip, dnet = rnd(B, T, S, seed=6), rnd(B, T, Rr, seed=7)
    th, sg = torch.tanh(rnd(B, T, Cg, seed=8)), torch.sigmoid(rnd(B, T, Cg, seed=9))
    dg = torch.cat([dskip, dnet], -1) @ w.t()
    want_pre = torch.cat([dg * sg * (1 - th * th), dg * th * sg * (1 - sg)], -1)
    wT = g(w.t().contiguous())
    dpre = torch.empty(B, 2 * Cg, T, device=DEV)
    K.conv_gemm(x0=bct(dskip), x1=bct(dnet), w=wT, out0=dpre, aux0=bct(th), aux1=bct(sg), B=B, T_in=T, T_out=T,
                M=Cg, C0=S, C1=Rr, taps=[0], epilogue=K.EPI_GATE_BWD)
    close(btc(dpre), want_pre, what='gate backward')


def test_mask_relu_in_and_bn_epilogues(K):
    B, T, Cin, Cout = 2, 256, 32, 64
    x, w, b = rnd(B, T, Cin, seed=1), rnd(1, Cin, Cout, seed=2, s=0.2), rnd(Cout, seed=3)
    sc, sh = rnd(Cout, seed=4), rnd(Cout, seed=5)
    out = torch.empty(B, Cout, T, device=DEV); r = torch.empty_like(out)
    K.conv_gemm(x0=bct(x), w=g(w), bias=g(b), scale=g(sc), shift=g(sh), out0=out, save0=r, B=B, T_in=T, T_out=T,
                M=Cout, C0=Cin, taps=[0], in_relu=True, out_relu=True)
    rr = torch.relu(torch.relu(x) @ w[0] + b)
    close(btc(r), rr, what='relu out')
    close(btc(out), rr * sc + sh, what='bn affine')
    aux = rnd(B, T, Cout, seed=6)
    K.conv_gemm(x0=bct(x), w=g(w), scale=g(sc), out0=out, aux0=bct(aux), B=B, T_in=T, T_out=T, M=Cout, C0=Cin,
                taps=[0], epilogue=K.EPI_MASK)
    close(btc(out), (x @ w[0]) * sc * (aux > 0), what='mask')


@pytest.mark.parametrize('T_in,k,stride', [(512, 5, 2), (208, 5, 2), (256, 4, 2), (250, 5, 2), (256, 3, 1)])
def test_keras_same_conv_fwd_dgrad_wgrad(K, pkg, T_in, k, stride):
    L = pkg._lib
    B, Cin, Cout = 2, 32, 48
    pl, pr = R.same_pads(T_in, k, stride)
    T_out = -(-T_in // stride)
    x, w, b = rnd(B, T_in, Cin, seed=1), rnd(k, Cin, Cout, seed=2, s=0.1), rnd(Cout, seed=3)
    xr = x.clone().requires_grad_(True); wr = w.clone().requires_grad_(True)
    yo = R.keras_conv1d(xr, wr, b, stride=stride, padding='same', relu=False)
    xb, wb, bb = bct(x), g(w), g(b)
    y = torch.empty(B, Cout, T_out, device=DEV)
    L.check(L.lib().vqw_conv1d_same_fwd(L.ptr(xb), L.ptr(wb), L.ptr(bb), L.ptr(y), B, Cin, Cout, T_in, T_out, k,
                                        stride, pl, 0, L.stream()))
    close(btc(y), yo, what='same fwd')
    dy = rnd(B, T_out, Cout, seed=7)
    yo.backward(dy)
    wT = torch.empty(k, Cout, Cin, device=DEV)
    K.transpose(wb, wT, k, Cin, Cout)
    dx = torch.full((B, Cin, T_in), float('nan'), device=DEV)
    dyb = bct(dy)
    L.check(L.lib().vqw_conv1d_same_dgrad(L.ptr(dyb), L.ptr(wT), L.ptr(dx), B, Cin, Cout, T_in, T_out, k, stride,
                                          pl, L.stream()))
    close(btc(dx), xr.grad, what='same dgrad')
    dw = torch.zeros(k, Cin, Cout, device=DEV)
    L.check(L.lib().vqw_conv1d_same_wgrad(L.ptr(xb), L.ptr(dyb), L.ptr(dw), B, Cin, Cout, T_in, T_out, k, stride,
                                          pl, L.stream()))
    close(dw, wr.grad, rtol=5e-4, atol=5e-4, what='same wgrad')


def test_wgrad_two_sources_relu_and_full_size(K):
    B, T, Cp, Q0, Q1 = 2, 512, 32, 64, 32
    p, q0, q1 = rnd(B, T, Cp, seed=1), rnd(B, T, Q0, seed=2), rnd(B, T, Q1, seed=3)
    want = torch.einsum('btc,bto->co', torch.relu(p), torch.cat([q0, q1], -1))
    dw = torch.zeros(Cp, Q0 + Q1, device=DEV)
    K.wgrad_gemm(p=bct(p), q0=bct(q0), q1=bct(q1), dw=dw, B=B, T_q=T, T_p=T, Cp=Cp, Q0=Q0, Q1=Q1, taps=[0], p_relu=True)
    close(dw, want, rtol=5e-4, atol=5e-4, what='wgrad 2 sources')
    # full-size decoder layer slice: B=1, T=6656, 256 -> 512, k=3, dilation 512
    T, d = 6656, 512
    x, dy = rnd(1, T, 256, seed=4), rnd(1, T, 512, seed=5)
    xr = x.clone(); wz = torch.zeros(3, 256, 512, requires_grad=True)
    R.conv1d_v2(xr, wz, None, dilations=d).backward(dy)
    dw = torch.zeros(3, 256, 512, device=DEV)
    K.wgrad_gemm(p=bct(x), q0=bct(dy), dw=dw, B=1, T_q=T, T_p=T, Cp=256, Q0=512, taps=[-2 * d, -d, 0])
    close(dw, wz.grad, rtol=1e-3, atol=1e-3, what='wgrad full size')


def _wgrad_ragged_cases():
    rng = np.random.RandomState(77)
    cases = []
    for i in range(16):
        B = int(rng.choice([1, 2, 3]))
        T = int(rng.choice([96, 160, 333, 512, 1000, 2080]))
        Cp = 16 * int(rng.randint(1, 12))
        Q = 4 * int(rng.randint(1, 70))
        k = int(rng.choice([1, 2, 3]))
        dil = int(rng.choice([1, 2, 5, 64]))
        splits = int(rng.choice([0, 0, 1, 2, 5]))
        cases.append((B, T, Cp, Q, k, dil, splits, i))
    return cases


@pytest.mark.parametrize('B,T,Cp,Q,k,dil,splits,seed', _wgrad_ragged_cases())
def test_wgrad_engine_ragged_shapes(K, B, T, Cp, Q, k, dil, splits, seed):
    """Conv2DBackpropFilter of wavenet_ops.py:59-90 on shapes the model never uses (ragged T, partial tiles, any
    split count incl. the automatic one) against autograd of the oracle's conv1d_v2."""
    x, dy = rnd(B, T, Cp, seed=seed), rnd(B, T, Q, seed=seed + 50)
    wz = torch.zeros(k, Cp, Q, requires_grad=True)
    R.conv1d_v2(x, wz, None, dilations=dil).backward(dy)
    dw = torch.zeros(k, Cp, Q, device=DEV)
    K.wgrad_gemm(p=bct(x), q0=bct(dy), dw=dw, B=B, T_q=T, T_p=T, Cp=Cp, Q0=Q, taps=[-(k - 1 - j) * dil for j in range(k)],
                 splits=splits)
    close(dw, wz.grad, rtol=1e-3, atol=1e-3, what='wgrad (splits %d)' % splits)


# ----------------------------------------------------------------------------- small kernels
def test_conv_cin1_fwd_and_wgrad(K):
    B, T, F, k = 2, 520, 32, 32
    x, w, b = rnd(B, T, 1, seed=1), rnd(k, 1, F, seed=2, s=0.2), rnd(F, seed=3)
    wr = w.clone().requires_grad_(True)
    yo = R.conv1d_v2(x, wr, b)
    out = torch.empty(B, F, T, device=DEV)
    xb = g(x[:, :, 0])
    K.conv_cin1_fwd(xb, g(w.reshape(k, F)), g(b), out, k=k, stride=1, offset=-(k - 1))
    close(btc(out), yo, what='preprocess fwd')
    dy = rnd(B, T, F, seed=4)
    yo.backward(dy)
    dw = torch.zeros(k, F, device=DEV)
    K.conv_cin1_wgrad(xb, bct(dy), dw, k=k, stride=1, offset=-(k - 1))
    close(dw, wr.grad.reshape(k, F), rtol=5e-4, atol=5e-4, what='preprocess wgrad')
    # encoder layer 1: k=5, stride 2, SAME (pads 1,2), relu + BN affine
    k, Fo = 5, 48
    w1, b1, sc, sh = rnd(k, 1, Fo, seed=5, s=0.3), rnd(Fo, seed=6, s=0.1), rnd(Fo, seed=7), rnd(Fo, seed=8)
    w1r = w1.clone().requires_grad_(True)
    r = R.keras_conv1d(x, w1r, b1, stride=2, padding='same', relu=True)
    out = torch.empty(B, Fo, T // 2, device=DEV); sr = torch.empty_like(out)
    K.conv_cin1_fwd(xb, g(w1.reshape(k, Fo)), g(b1), out, k=k, stride=2, offset=-1, relu=True, scale=g(sc), shift=g(sh), save_r=sr)
    close(btc(sr), r, what='enc1 relu')
    close(btc(out), r * sc + sh, what='enc1 bn')


@pytest.mark.parametrize('T', [2600, 2602])
def test_conv_cin1_long_rows(K, T):
    """Rows longer than one 1024-step chunk (the weight-gradient kernel walks them and reduces once), a length that is not
    a multiple of 4, both strides."""
    B, F, k = 3, 24, 32
    x, w, b = rnd(B, T, 1, seed=11), rnd(k, 1, F, seed=12, s=0.2), rnd(F, seed=13)
    wr = w.clone().requires_grad_(True)
    yo = R.conv1d_v2(x, wr, b)
    xb = g(x[:, :, 0])
    out = torch.empty(B, F, T, device=DEV)
    K.conv_cin1_fwd(xb, g(w.reshape(k, F)), g(b), out, k=k, stride=1, offset=-(k - 1))
    close(btc(out), yo, what='preprocess fwd')
    dy = rnd(B, T, F, seed=14)
    yo.backward(dy)
    dw = torch.zeros(k, F, device=DEV)
    K.conv_cin1_wgrad(xb, bct(dy), dw, k=k, stride=1, offset=-(k - 1))
    close(dw, wr.grad.reshape(k, F), rtol=1e-3, atol=1e-3, what='preprocess wgrad')
    k, Fo = 5, 40
    w1, b1 = rnd(k, 1, Fo, seed=15, s=0.3), rnd(Fo, seed=16, s=0.1)
    w1r = w1.clone().requires_grad_(True)
    r = R.keras_conv1d(x, w1r, b1, stride=2, padding='same', relu=True)
    To = r.shape[1]
    out = torch.empty(B, Fo, To, device=DEV)
    K.conv_cin1_fwd(xb, g(w1.reshape(k, Fo)), g(b1), out, k=k, stride=2, offset=-1, relu=True)
    close(btc(out), r, what='enc1 relu')
    dy2 = rnd(B, To, Fo, seed=17)
    r.backward(dy2)
    dpre = dy2 * (r.detach() > 0)
    dw1 = torch.zeros(k, Fo, device=DEV)
    K.conv_cin1_wgrad(xb, bct(dpre), dw1, k=k, stride=2, offset=-1)
    close(dw1, w1r.grad.reshape(k, Fo), rtol=1e-3, atol=1e-3, what='enc1 wgrad')


@pytest.mark.parametrize('T,with_r', [(416, True), (104, False), (37, True)])
def test_bn_relu_bwd_with_sums(K, T, with_r):
    """One pass: dz = dx * scale * (r > 0) and the three per-channel sums of an encoder layer's backward (encoder.py:19-20)."""
    B, Cc = 3, 40
    dx, y, sc = rnd(B, Cc, T, seed=21), rnd(B, Cc, T, seed=22), rnd(Cc, seed=23)
    r = torch.relu(y) if with_r else None
    yy = r if with_r else y
    dsc0, dbe0, dbi0 = rnd(Cc, seed=24), rnd(Cc, seed=25), rnd(Cc, seed=26)
    dsc, dbe, dbi = g(dsc0), g(dbe0), g(dbi0)
    dz = g(dx)
    K.bn_relu_bwd_sums(dz, g(yy), g(r) if with_r else None, g(sc), dz, dscale=dsc, dbeta=dbe, dbias=dbi)      # in place
    want = dx * sc[None, :, None] * ((r > 0) if with_r else 1.0)
    close(dz, want, what='dz')
    close(dsc, dsc0 + (dx * yy).sum((0, 2)), rtol=1e-4, atol=1e-4, what='d scale')
    close(dbe, dbe0 + dx.sum((0, 2)), rtol=1e-4, atol=1e-4, what='d beta')
    close(dbi, dbi0 + want.sum((0, 2)), rtol=1e-4, atol=1e-4, what='d bias')


def test_rowsum_transpose_softmax_adam(K):
    B, Cc, T = 3, 20, 448
    x, y = rnd(B, Cc, T, seed=1), rnd(B, Cc, T, seed=2)
    seg = torch.empty(B, Cc, T // 64, device=DEV); tot = torch.ones(Cc, device=DEV)
    K.rowsum(g(x), y=g(y), seg_out=seg, total=tot, alpha=0.5, seg=64)
    close(seg, (x * y).reshape(B, Cc, T // 64, 64).sum(-1), what='segsum')
    close(tot, 1 + 0.5 * (x * y).sum((0, 2)), rtol=1e-4, atol=1e-4, what='rowsum total')
    tot2 = torch.zeros(Cc, device=DEV)
    K.rowsum(g(x[:, :, :104].contiguous()), total=tot2)
    close(tot2, x[:, :, :104].sum((0, 2)), what='rowsum T=104')
    # softmax cross-entropy
    B, Q, T = 2, 256, 200
    lg = rnd(B, Q, T, seed=3, s=3.0); lab = torch.from_numpy(np.random.RandomState(4).randint(0, Q, (B, T)).astype(np.int32))
    lr = lg.clone().requires_grad_(True)
    loss = torch.nn.functional.cross_entropy(lr.permute(0, 2, 1).reshape(-1, Q), lab.reshape(-1).long(), reduction='sum')
    loss.backward()
    ls = torch.zeros(1, device=DEV); dl = torch.empty(B, Q, T, device=DEV); pr = torch.empty_like(dl)
    K.softmax_xent(g(lg), g(lab), loss_sum=ls, dlogits=dl, probs=pr, grad_scale=0.25)
    close(ls, loss.detach().reshape(1), rtol=1e-5, atol=1e-5, what='CE loss')
    close(dl, 0.25 * lr.grad, atol=1e-6, rtol=1e-5, what='dlogits')
    close(pr, torch.softmax(lg, 1), atol=1e-6, rtol=1e-5, what='probs')
    # the same op through the two entries SURVEY 8(b) names: bit-equal to the fused call
    ls2 = torch.zeros(1, device=DEV); pr2 = torch.full_like(dl, float('nan')); dl2 = torch.full_like(dl, float('nan'))
    K.softmax_xent_fwd(g(lg), g(lab), loss_sum=ls2, probs=pr2)
    K.softmax_xent_bwd(g(lg), g(lab), dlogits=dl2, grad_scale=0.25)
    close(ls2, loss.detach().reshape(1), rtol=1e-5, atol=1e-5, what='CE loss (fwd entry)')
    assert torch.equal(pr2, pr) and torch.equal(dl2, dl)
    inplace = g(lg).clone()
    K.softmax_xent_bwd(inplace, g(lab), dlogits=inplace, grad_scale=0.25)
    assert torch.equal(inplace, dl)
    # Adam + EMA, two steps, n not a multiple of 4
    n = 1003
    p0, gr = rnd(n, seed=5), rnd(n, seed=6)
    P = {'w': p0.clone()}; st = {'t': 0, 'm': {}, 'v': {}, 'ema': {}}
    pd, md, vd = g(p0.clone()), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    ed = pd.clone()
    for t in (1, 2):
        M.adam_ema_step(P, {'w': gr * t}, st, 1e-3)
        lr_t = 1e-3 * (1 - 0.999 ** t) ** 0.5 / (1 - 0.9 ** t)
        K.adam_ema_step(pd, g(gr * t), md, vd, ed, lr_t=lr_t)
    close(pd, P['w'], atol=1e-6, rtol=1e-6, what='adam param')
    close(ed, st['ema']['w'], atol=1e-6, rtol=1e-6, what='ema')


# ----------------------------------------------------------------------------- reference-named op surface
def test_reference_op_surface(pkg):
    O = pkg.ops
    B, T, R_, S_, Cc, Tz = 2, 512, 32, 64, 32, 8
    x = rnd(B, T, 1, seed=1, s=0.3)
    assert np.array_equal(O.mu_law_encode(g(x), to_int=True).cpu().numpy(), R.mu_law_encode_np(x.numpy(), to_int=True))
    np.testing.assert_allclose(O.mu_law_encode(g(x)).cpu().numpy(), R.mu_law_encode_np(x.numpy()), atol=3e-7)
    assert torch.equal(O.shift_right(g(x)).cpu(), R.shift_right(x))
    oh = O.mu_law_encode(g(x), one_hot=True)
    assert oh.shape == (B, T, 256) and float(oh.sum()) == B * T
    net, cond = rnd(B, T, R_, seed=2), rnd(B, Tz, Cc, seed=3)
    p = {'gated/kernel': rnd(3, R_, 2 * R_, seed=4, s=0.1), 'gated/bias': rnd(2 * R_, seed=5, s=0.1),
         'gated/local_condition/kernel': rnd(1, Cc, 2 * R_, seed=6, s=0.1),
         'skip/kernel': rnd(1, R_, S_, seed=7, s=0.1), 'skip/bias': rnd(S_, seed=8, s=0.1),
         'residual/kernel': rnd(1, R_, R_, seed=9, s=0.1), 'residual/bias': rnd(R_, seed=10, s=0.1)}
    pg = {k: g(v) for k, v in p.items()}
    sk, rs = O.residual_stack(g(net), pg, 4, g(cond))
    sk_ref, rs_ref = R.residual_stack(net, p, R_, 4, cond)
    close(sk, sk_ref, atol=5e-5, rtol=5e-5, what='residual_stack skip')
    close(rs, rs_ref, atol=5e-5, rtol=5e-5, what='residual_stack residual')
    close(O.add_condition(g(net[..., :2 * R_ // 2].repeat(1, 1, 2)), g(cond), pg['gated/local_condition/kernel']),
          R.add_condition(net.repeat(1, 1, 2), cond, p['gated/local_condition/kernel']), what='add_condition')
    w32, b32 = rnd(32, 1, R_, seed=11, s=0.2), rnd(R_, seed=12)
    close(O.conv1d_v2(g(x), g(w32), g(b32)), R.conv1d_v2(x, w32, b32), what='preprocess conv1d_v2')
    v = rnd(B, R_, seed=13)
    close(O.linear(g(v), pg['skip/kernel'], pg['skip/bias']), R.linear(v, p['skip/kernel'], p['skip/bias']), what='linear')
    e = rnd(B, 250, 32, seed=14)
    for fn, k, s_ in ((O.conv_3_768, 3, 1), (O.strided_conv_4_768, 4, 2), (O.linear_64, 1, 1)):
        wk, bk = rnd(k, 32, 48, seed=15, s=0.1), rnd(48, seed=16)
        want = R.keras_conv1d(e, wk, bk, stride=s_, padding='same', relu=fn is not O.linear_64)
        close(fn(g(e), g(wk), g(bk)), want, what=fn.__name__)
    h = rnd(B, 1, 16, seed=17)
    assert torch.equal(O.concat(g(cond), g(h)).cpu(), R.concat(cond, h))
    with pytest.raises(NotImplementedError):
        O.conv1d_v2(g(net), pg['skip/kernel'], None, padding='SAME')
