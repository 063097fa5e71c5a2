"""GPU tests of mu-law audio at 512 and 1024 levels, from the label kernels to every generator, against the oracle at the level
(tests/levels_ref.py: oracle.ref_model.wavenet_build with R.mu_law_encode bound to the level, R.mu_law_decode_np(., Q)).

Bars, none of them new: integer labels bit for bit; float encode atol 3e-7 and decode rtol 2e-6 / atol 1e-7
(test_kernels_gpu.test_mu_law_float_and_decode); the model at tests/test_model_gpu.py's bars (run_parity, imported: labels
exact, losses rtol 2e-5, tiny-width gradients 2e-3 of the tensor maximum; the engine head at test_default_width_short_segment's
5e-3 in relative L2); generated audio rtol 1e-5 / atol 1e-6 of decode(idx), every draw by gen_ref.check_sampled, greedy
indices the float64 argmax up to a 2e-6 tie (test_prefill_gpu.check_greedy's bar), last-step distributions rtol 2e-4 /
atol 1e-7; prefill's first distribution rtol 1e-4 / atol 1e-7 (test_prefill_gpu).  Each test prints what it measured."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import ref_model as M

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_ref as G  # noqa: E402
import levels_ref as LR  # noqa: E402
import sampling_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu
R = M.R
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DIL = [1, 2, 4, 8] * 2
N = 160                       # crosses two condition frames of 64
MAX_EXCUSED = 0.002           # of B * n (test_generation_long_gpu / test_wide_gen_gpu)


def model_tests():
    spec = importlib.util.spec_from_file_location('model_gpu_tests', os.path.join(HERE, 'test_model_gpu.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------ kernels
def thresholds(Q):
    import re
    name = 'mu_law_table.h' if Q == 256 else 'mu_law_table_%d.h' % Q
    text = open(os.path.join(ROOT, 'vq-vae-wavenet_amd', 'csrc', name)).read()
    return np.array([int(v, 16) for v in re.findall(r'0x([0-9A-F]{8})u', text)], dtype=np.uint32).view(np.float32)


@pytest.fixture(scope='module')
def kernel_inputs():
    """{Q: x}: every threshold with its two fp32 neighbours, the specials, all 65 536 PCM codes, 2^16 random values; the
    length is no multiple of 256 (the last block is ragged)."""
    out = {}
    for Q in LR.LEVELS:
        thr = thresholds(Q)
        rng = np.random.RandomState(Q)
        pcm = ((np.arange(-32768, 32768).astype(np.float32) + np.float32(0.5)) / np.float32(32767.5)).astype(np.float32)
        x = np.concatenate([thr, np.nextafter(thr, np.float32(-2), dtype=np.float32), np.nextafter(thr, np.float32(2), dtype=np.float32),
                            np.array([0.0, -0.0, 1.0, -1.0, 1.5, -1.5, 1e-41, -1e-41], np.float32), pcm,
                            rng.uniform(-1.1, 1.1, 1 << 16).astype(np.float32)]).astype(np.float32)
        if x.size % 256 == 0:
            x = np.concatenate([x, np.float32([0.25])])
        assert x.size % 256 != 0 and x.size > 70001
        out[Q] = x
    return out


@pytest.mark.parametrize('Q', [512, 1024])
def test_labels_are_the_oracles_bit_for_bit(K, kernel_inputs, Q):
    x = kernel_inputs[Q]
    got = K.mu_law_encode_i32(dev(x), levels=Q).cpu().numpy()
    want = R.mu_law_encode_np(x, Q, True)
    assert got.dtype == np.int32 and np.array_equal(got, want), 'first difference at x = %r' % x[np.argmax(got != want)]
    assert want.min() == 0 and want.max() == Q - 1 and len(np.unique(want)) == Q


@pytest.mark.parametrize('Q', LR.LEVELS)
def test_float_encode_and_decode_hold_the_256_level_bars(K, kernel_inputs, Q):
    x = kernel_inputs[Q]
    got = K.mu_law_encode_f32(dev(x), levels=Q).cpu().numpy()
    want = R.mu_law_encode_np(x, Q)
    idx = np.arange(0, Q + 1, dtype=np.float32)                      # Q itself: a uniform above the last cdf value
    dec = K.mu_law_decode_f32(dev(idx), levels=Q).cpu().numpy()
    wdec = R.mu_law_decode_np(idx, Q)
    print('\n[levels] Q=%d: float encode max abs error %.3g; decode max abs error %.3g, max rel. error %.3g' % (
        Q, np.abs(got - want).max(), np.abs(dec - wdec).max(), (np.abs(dec - wdec) / np.maximum(np.abs(wdec), 1e-30))[wdec != 0].max()))
    np.testing.assert_allclose(got, want, rtol=0, atol=3e-7)
    np.testing.assert_allclose(dec, wdec, rtol=2e-6, atol=1e-7)


@pytest.mark.parametrize('Q', [512, 1024])
def test_wavenet_inputs_levels(K, Q):
    B, T = 3, 320
    x, _, _ = M.synthetic_batch(B, T, 10, 7)
    xb = x[:, :, 0].contiguous().cuda()
    inputs = torch.full((B, T), float('nan'), device='cuda')
    labels = torch.full((B, T), -7, dtype=torch.int32, device='cuda')
    K.wavenet_inputs(xb, inputs, labels, levels=Q)
    assert np.array_equal(labels.cpu().numpy(), R.mu_law_encode_np(x[:, :, 0].numpy(), Q, True))
    want = R.mu_law_encode_np(R.shift_right(x)[:, :, 0].numpy(), Q)
    got = inputs.cpu().numpy()
    np.testing.assert_allclose(got, want, rtol=0, atol=3e-7)
    assert (got[:, 0] == 0).all()                                    # the shift: zero at t = 0 of each row
    assert torch.equal(inputs[:, 1:], K.mu_law_encode_f32(xb, levels=Q)[:, :-1])
    only = torch.full((B, T), -7, dtype=torch.int32, device='cuda')  # either output may be NULL
    K.wavenet_inputs(xb, None, only, levels=Q)
    assert torch.equal(only, labels)


def test_level_256_through_the_new_entries_is_the_old_entries_bitwise(pkg, K, kernel_inputs):
    L, lib = pkg._lib, pkg._lib.lib()
    x = dev(kernel_inputs[256])
    n = x.numel()
    f_old, f_new = torch.empty_like(x), torch.empty_like(x)
    i_old, i_new = (torch.empty(n, dtype=torch.int32, device='cuda') for _ in range(2))
    L.check(lib.vqw_mu_law_encode_f32(L.ptr(x), L.ptr(f_old), n, L.stream()))
    L.check(lib.vqw_mu_law_encode_f32_levels(L.ptr(x), L.ptr(f_new), n, 256, L.stream()))
    L.check(lib.vqw_mu_law_encode_i32(L.ptr(x), L.ptr(i_old), n, L.stream()))
    L.check(lib.vqw_mu_law_encode_i32_levels(L.ptr(x), L.ptr(i_new), n, 256, L.stream()))
    assert torch.equal(f_old.view(torch.int32), f_new.view(torch.int32)) and torch.equal(i_old, i_new)
    idx = torch.arange(0, 257, device='cuda', dtype=torch.float32)
    d_old, d_new = torch.empty_like(idx), torch.empty_like(idx)
    L.check(lib.vqw_mu_law_decode_f32(L.ptr(idx), L.ptr(d_old), 257, L.stream()))
    L.check(lib.vqw_mu_law_decode_f32_levels(L.ptr(idx), L.ptr(d_new), 257, 256, L.stream()))
    assert torch.equal(d_old.view(torch.int32), d_new.view(torch.int32))
    xb = x[:3 * 320].view(3, 320).contiguous()
    outs = []
    for new in (False, True):
        a, b = torch.empty_like(xb), torch.empty(3, 320, dtype=torch.int32, device='cuda')
        if new:
            L.check(lib.vqw_wavenet_inputs_levels(L.ptr(xb), L.ptr(a), L.ptr(b), 3, 320, 256, L.stream()))
        else:
            L.check(lib.vqw_wavenet_inputs(L.ptr(xb), L.ptr(a), L.ptr(b), 3, 320, L.stream()))
        outs.append((a, b))
    assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32)) and torch.equal(outs[0][1], outs[1][1])
    z = torch.randn(2, 256, 70, generator=torch.Generator().manual_seed(3)).cuda()
    a_old, a_new = torch.empty(2, 70, device='cuda'), torch.empty(2, 70, device='cuda')
    i_old = K.softmax_sample(z, mode='greedy', audio=a_old)         # (the wrapper at 256 calls the old symbol: the new one directly)
    i_new = torch.empty_like(i_old)
    L.check(lib.vqw_softmax_sample_levels(L.ptr(z), None, None, None, None, 0, L.ptr(i_new), L.ptr(a_new), None, 2, 256, 70, 256,
                                          L.stream()))
    assert torch.equal(i_old, i_new) and torch.equal(a_old.view(torch.int32), a_new.view(torch.int32))


# ------------------------------------------------------------------ the model
@pytest.mark.parametrize('Q', [512, 1024])
def test_tiny_model_at_a_level(pkg, Q):
    """'64' encoder, B = 2, T = 256: labels, losses, gradients, the Adam step -- run_parity of test_model_gpu.py against the
    oracle at the level."""
    m, w = G.tiny_cfg()
    w = LR.with_levels(w, Q)
    with LR.at_level():
        worst = model_tests().run_parity(pkg, m, w, 10, 2, 256, seed=11 + Q, steps=1)
    print('\n[levels] tiny model Q=%d: worst grad' % Q, worst)


def test_tiny_magenta_model_at_512(pkg):
    """Encoder_Magenta compands its own input at 256 levels into a buffer of its own (the decoder's holds the 512-level input):
    the gradient of its Cin = 1 input conv and of the decoder's are both the oracle's."""
    m, w = G.tiny_cfg()
    m, w = dict(m, encoder='Magenta'), LR.with_levels(w, 512)
    T = model_tests()
    seen = {}
    real = M.train_step

    def spy(*a, **kw):
        out, grads = real(*a, **kw)
        seen.update(grads)
        return out, grads
    with LR.at_level():
        M.train_step = spy
        try:
            worst = T.run_parity(pkg, m, w, 10, 2, 256, seed=21, steps=1)
        finally:
            M.train_step = real
    assert 'encoder/preprocess/kernel' in seen and 'decoder/preprocess/kernel' in seen
    assert float(seen['encoder/preprocess/kernel'].abs().max()) > 0
    print('\n[levels] tiny Magenta model Q=512: worst grad', worst)


def test_engine_eligible_head_at_1024(pkg):
    """R = S = 256, Q = 1024, two layers, B = 1, T = 256 at test_default_width_short_segment's bar (5e-3 in relative L2):
    postprocess2 with N = 1024 columns (and its input gradient with K = 1024) on whichever engine the plan picks."""
    T = model_tests()
    m = dict(M.DEFAULT_MODEL)
    w = dict(M.DEFAULT_WAVENET)
    w.update(quantization_channels=1024, num_cycles=1, num_cycle_layers=2, dilation_rates=[1, 2], dilation_filters=256,
             residual_filters=256, skip_filters=256, preprocess={'kernel_size': 32, 'filters': 256})
    with LR.at_level():
        worst = T.run_parity(pkg, m, w, 109, 1, 256, seed=3, steps=1, grad_tol=5e-3, err=T.l2err, check_params=False)
    probe = pkg.model.VQVAE(m, w, 109, device='cuda', seed=0)
    x, spk, _ = M.synthetic_batch(1, 256, 109, 1234)
    ws = probe.forward(x[:, :, 0].contiguous().cuda(), spk.cuda(), compute_grad_seed=False)
    print('\n[levels] engine head Q=1024: x3_used %s, head_x3 %s, why %r, worst grad %s' % (
        bool(ws['x3_used']), bool(ws['plan'].head_x3), ws['plan'].why, worst))


# ------------------------------------------------------------------ generators
def configs(Rw, Sw, Q):
    m, w = G.tiny_cfg()
    w.update(dilation_rates=list(DIL), num_cycles=2, num_cycle_layers=4, kernel_size=3, dilation_filters=Rw, residual_filters=Rw,
             skip_filters=Sw, quantization_channels=Q, preprocess={'kernel_size': 32, 'filters': Rw})
    return m, w


@pytest.fixture(scope='module')
def decoders(pkg):
    made = {}

    def get(Rw, Sw, Q):
        if (Rw, Sw, Q) not in made:
            m, w = configs(Rw, Sw, Q)
            P = M.init_params(m, w, 10, seed=100 + Rw + Q, randomize_all=True)
            model = pkg.model.VQVAE(m, w, 10, device='cuda', seed=0)
            model.load_named(P)
            assert model.levels == Q
            made[(Rw, Sw, Q)] = (model, P, w)
        return made[(Rw, Sw, Q)]
    yield get
    made.clear()
    torch.cuda.empty_cache()


def inputs(model, B, n, seed):
    g = torch.Generator().manual_seed(seed)
    enc = 0.5 * torch.randn(B, model.Cc, -(-n // 64), generator=g)            # [B][Cc][Tz]: no encoder run needed
    u = torch.rand(B, n, generator=g)
    return enc, u


def probs64(P, w, audio, enc, idx):
    """The float64 reference at the level; the labels it forms from the generated audio must be the generator's indices."""
    n = audio.shape[1]
    Tz = enc.shape[2]
    Q = w['quantization_channels']
    pad = Tz * 64 - n                                # wavenet_build wants whole condition frames: zeros after the run (causal),
    idx = np.asarray(idx)                            # whose label is Q / 2
    a = np.concatenate([audio, np.zeros((audio.shape[0], pad), np.float32)], 1)
    i = np.concatenate([idx, np.full((idx.shape[0], pad), Q // 2, idx.dtype)], 1)
    with LR.at_level():
        p = G.decoder_probs64(P, w, a, enc.permute(0, 2, 1), idx=i)[:, :n]
    assert np.array_equal(R.mu_law_encode_np(audio, Q, True), idx), 'mu_law_encode(audio) is not the index drawn'
    return p


def check_run(P, w, enc, u, audio, idx, probs, tag):
    """Sampled run from reset against the contract; returns p64."""
    Q = w['quantization_channels']
    a_h, i_h = audio.cpu().numpy(), idx.cpu().numpy()
    np.testing.assert_allclose(a_h, LR.decode(i_h, Q), rtol=1e-5, atol=1e-6)
    assert i_h.max() > 255, 'no index above 255 was drawn: the run shows nothing about the level'
    p64 = probs64(P, w, a_h, enc, i_h)
    B, n = i_h.shape
    excused = G.check_sampled(p64, u, i_h, G.ring_depths(3, DIL))
    print('\n[levels] %s Q=%d B=%d n=%d: excused %d, %d distinct indices, max index %d' % (
        tag, Q, B, n, excused, len(np.unique(i_h)), i_h.max()))
    assert excused <= max(1, MAX_EXCUSED * B * n), '%d of %d steps needed the cdf-edge excuse' % (excused, B * n)
    if probs is not None:
        np.testing.assert_allclose(probs.cpu().numpy(), p64[:, -1], rtol=2e-4, atol=1e-7, err_msg='distribution of the last step')
    return p64


def check_greedy(P, w, enc, audio, idx):
    Q = w['quantization_channels']
    a_h, i_h = audio.cpu().numpy(), idx.cpu().numpy()
    np.testing.assert_allclose(a_h, LR.decode(i_h, Q), rtol=1e-5, atol=1e-6)
    p64 = probs64(P, w, a_h, enc, i_h)
    gap = p64.max(-1) - np.take_along_axis(p64, i_h[:, :, None].astype(np.int64), -1)[:, :, 0]
    assert gap.max() <= 2e-6, 'greedy index is not the float64 argmax at (row, step) %s' % (np.unravel_index(gap.argmax(), gap.shape),)


def fast_case(pkg, decoders, monkeypatch, persistent, Rw, Sw, Q, B, n, cut):
    for k in ('VQW_AR_PERSISTENT', 'VQW_AR_CPB', 'VQW_AR_ROWS', 'VQW_AR_PLACE'):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('VQW_AR_PERSISTENT', persistent)
    model, P, w = decoders(Rw, Sw, Q)
    enc, u = inputs(model, B, n, Q + B + n)
    enc_d, u_d = enc.cuda(), u.cuda()
    gen = pkg.generator.FastGenerator(model, batch=B)
    try:
        nwg = [pkg._lib.lib().vqw_ar_decode_workgroups(h) for h in gen._hs]
        assert all((v > 0) == (persistent == '1') for v in nwg), 'workgroups per handle %s: another back end ran' % nwg
        audio, idx, probs = gen.generate(enc_d, n, mode='sample', uniforms=u_d, return_probs=True)
        check_run(P, w, enc, u, audio, idx, probs, 'FastGenerator persistent=%s' % persistent)
        if cut:      # a run cut at the checkpoints equals the single run
            gen.reset()
            ia, aa, prev = [], [], 0
            for t in G.checkpoints(n, 3, max(DIL)):
                a_c, i_c = gen.generate(enc_d, t - prev, mode='sample', uniforms=u_d[:, prev:t].contiguous())
                ia.append(i_c); aa.append(a_c)
                prev = t
            assert prev == n and torch.equal(torch.cat(ia, 1), idx) and torch.equal(torch.cat(aa, 1), audio)
        gen.reset()
        ga, gi = gen.generate(enc_d, n)
        check_greedy(P, w, enc, ga, gi)
    finally:
        gen.close()


@pytest.mark.parametrize('persistent', ['1', '0'])
def test_fast_generator_at_512(pkg, decoders, monkeypatch, persistent):
    fast_case(pkg, decoders, monkeypatch, persistent, 64, 128, 512, 2, N, cut=True)


def test_fast_generator_at_1024_on_the_persistent_kernel(pkg, decoders, monkeypatch):
    """LDS is sized by Q (the head's columns, the logits, the decode / re-encode table): the largest Q is where it breaks."""
    fast_case(pkg, decoders, monkeypatch, '1', 128, 256, 1024, 1, 64, cut=False)


@pytest.fixture(scope='module')
def wide3(pkg, decoders):
    model, P, w = decoders(64, 128, 512)
    enc, u = inputs(model, 3, N, 77)
    gen = pkg.generator.WideGenerator(model, batch=3)
    audio, idx, probs = gen.generate(enc.cuda(), N, mode='sample', uniforms=u.cuda(), return_probs=True)
    p64 = check_run(P, w, enc, u, audio, idx, probs, 'WideGenerator')
    yield dict(model=model, P=P, w=w, enc=enc, u=u, gen=gen, audio=audio, idx=idx, probs=probs, p64=p64)
    gen.close()


def test_wide_generator_at_512(pkg, wide3):
    """Sampled run against the contract (asserted when the fixture is made), greedy, row 1 alone, a run cut at the checkpoints."""
    r = wide3
    gen, enc_d, u_d = r['gen'], r['enc'].cuda(), r['u'].cuda()
    gen.reset()
    ia, aa, prev = [], [], 0
    for t in G.checkpoints(N, 3, max(DIL)):
        a_c, i_c = gen.generate(enc_d, t - prev, mode='sample', uniforms=u_d[:, prev:t].contiguous())
        ia.append(i_c); aa.append(a_c)
        prev = t
    assert prev == N and torch.equal(torch.cat(ia, 1), r['idx']) and torch.equal(torch.cat(aa, 1), r['audio'])
    one = pkg.generator.WideGenerator(r['model'], batch=1)
    a1, i1, p1 = one.generate(enc_d[1:2].contiguous(), N, mode='sample', uniforms=u_d[1:2].contiguous(), return_probs=True)
    one.close()
    assert torch.equal(i1, r['idx'][1:2]) and torch.equal(a1, r['audio'][1:2]) and torch.equal(p1, r['probs'][1:2])
    gen.reset()
    ga, gi = gen.generate(enc_d, N)
    check_greedy(r['P'], r['w'], r['enc'], ga, gi)


def test_wide_generator_at_1024(pkg, decoders):
    model, P, w = decoders(128, 256, 1024)
    enc, u = inputs(model, 3, 64, 5)
    gen = pkg.generator.WideGenerator(model, batch=3)
    audio, idx, probs = gen.generate(enc.cuda(), 64, mode='sample', uniforms=u.cuda(), return_probs=True)
    gen.close()
    check_run(P, w, enc, u, audio, idx, probs, 'WideGenerator')


@pytest.mark.parametrize('which', ['fast', 'wide'])
def test_truncated_row_beside_a_default_row_at_512(pkg, decoders, monkeypatch, which):
    """Row 0 at its defaults equals the plain run bit for bit; row 1 (temperature 0.8, top-k 50, top-p 0.9) follows
    tests/sampling_ref.py on the reference's logits (test_wide_gen_gpu.test_truncated_rows' criterion)."""
    monkeypatch.delenv('VQW_AR_PERSISTENT', raising=False)
    monkeypatch.setenv('VQW_AR_ROWS', '2')
    model, P, w = decoders(64, 128, 512)
    enc, u = inputs(model, 2, N, 9)
    make = pkg.generator.FastGenerator if which == 'fast' else pkg.generator.WideGenerator
    gen = make(model, batch=2)
    pa, pi, pp = gen.generate(enc.cuda(), N, mode='sample', uniforms=u.cuda(), return_probs=True)
    gen.reset()
    t, k, p = 0.8, 50, 0.9
    ta, ti, tp = gen.generate(enc.cuda(), N, mode='sample', uniforms=u.cuda(), return_probs=True, temperature=[1.0, t],
                              top_k=[0, k], top_p=[1.0, p])
    gen.close()
    assert torch.equal(ti[0], pi[0]) and torch.equal(ta[0], pa[0]) and torch.equal(tp[0], pp[0])
    got = ti.cpu().numpy()
    np.testing.assert_allclose(ta.cpu().numpy(), LR.decode(got, 512), rtol=1e-5, atol=1e-6)
    p64 = probs64(P, w, ta.cpu().numpy(), enc, got)
    z = np.log(np.maximum(p64, 1e-300))
    un = u.double().numpy()
    for i in range(N):
        pr, keep, q, want = S.restate(z[1, i], t, k, p, un[1, i])
        if got[1, i] != want or not keep[got[1, i]]:
            assert S.fp32_edge(pr, keep, q, k, p, un[1, i]), 'step %d: GPU %d, restated %d' % (i, got[1, i], want)
    pl = tp[1].cpu().double().numpy()
    np.testing.assert_allclose(pl, q, rtol=2e-4, atol=1e-7)
    assert (pl[~keep] == 0).all() and keep.sum() <= k


def test_set_levels_refusals_on_real_handles(pkg, decoders):
    """A level that is not the handle's Q, and a code-input handle, are refused by name; setting the same level twice is fine."""
    lib = pkg._lib.lib()
    err = lambda: lib.vqw_last_error().decode()                      # noqa: E731
    model, _, _ = decoders(64, 128, 512)
    fast, wide = pkg.generator.FastGenerator(model, batch=1), pkg.generator.WideGenerator(model, batch=2)
    try:
        for fn, h in ((lib.vqw_ar_decode_set_levels, fast._hs[0]), (lib.vqw_ar_wide_set_levels, wide._h)):
            assert fn(h, 1024) != 0 and 'levels=1024' in err() and 'Q=512' in err()
            assert fn(h, 256) != 0 and 'levels=256' in err()
            assert fn(h, 512) == 0
    finally:
        fast.close(); wide.close()
    pt = G.prior_tests()
    cfg = pt.tiny_prior(k=512, pre_k=2)
    cfg.update(residual_filters=64, dilation_filters=64, skip_filters=128, preprocess=dict(cfg['preprocess'], filters=64))
    prior = pkg.prior.LatentPrior(cfg, 10, device='cuda', seed=0)
    pg, wg = pkg.generator.PriorGenerator(prior, batch=1), pkg.generator.WidePriorGenerator(prior, batch=2)
    try:
        assert lib.vqw_ar_decode_set_levels(pg._hs[0], 512) != 0 and 'code-input handle' in err()
        assert lib.vqw_ar_wide_set_levels(wg._h, 512) != 0 and 'code-input handle' in err()
    finally:
        pg.close(); wg.close()


# ------------------------------------------------------------------ prefill
@pytest.mark.parametrize('persistent', ['1', '0'])
def test_prefill_at_512(pkg, decoders, monkeypatch, persistent):
    """test_prefill_gpu.py's criterion with the parallel float64 reference at the level: after prefill(prompt of T steps,
    T > pre_k) the first distribution is the reference's (rtol 1e-4, atol 1e-7) and every greedy index its argmax up to a 2e-6 tie."""
    monkeypatch.setenv('VQW_AR_PERSISTENT', persistent)
    monkeypatch.delenv('VQW_AR_ROWS', raising=False)
    model, P, w = decoders(64, 128, 512)
    T, n = model.pre_k + 5, 91
    enc, _ = inputs(model, 2, T + n, 31)
    prompt = (torch.rand(2, T, generator=torch.Generator().manual_seed(5)) * 2 - 1).float()
    gen = pkg.generator.FastGenerator(model, batch=2)
    try:
        assert (pkg._lib.lib().vqw_ar_decode_workgroups(gen._hs[0]) > 0) == (persistent == '1')
        gen.prefill(prompt.cuda(), enc.cuda())
        _, _, first = gen.generate(enc.cuda(), 1, return_probs=True)
        gen.prefill(prompt.cuda(), enc.cuda())
        audio, idx = gen.generate(enc.cuda(), n)
    finally:
        gen.close()
    a_h, i_h = audio.cpu().numpy(), idx.cpu().numpy()
    np.testing.assert_allclose(a_h, LR.decode(i_h, 512), rtol=1e-5, atol=1e-6)
    whole = np.concatenate([prompt.numpy(), a_h], 1)
    pad = enc.shape[2] * 64 - whole.shape[1]
    whole = np.concatenate([whole, np.zeros((2, pad), np.float32)], 1)
    with LR.at_level():
        p64 = G.decoder_probs64(P, w, whole, enc.permute(0, 2, 1))[:, T:T + n]
    np.testing.assert_allclose(first.cpu().numpy(), p64[:, 0], rtol=1e-4, atol=1e-7)
    gap = p64.max(-1) - np.take_along_axis(p64, i_h[:, :, None].astype(np.int64), -1)[:, :, 0]
    assert gap.max() <= 2e-6, 'after prefill, (row, step) %s is not the argmax' % (np.unravel_index(gap.argmax(), gap.shape),)
    assert np.array_equal(R.mu_law_encode_np(a_h, 512, True), i_h)


# ------------------------------------------------------------------ reconstruct
def test_reconstruct_at_512(pkg, decoders):
    model, P, w = decoders(64, 128, 512)
    x, spk, _ = M.synthetic_batch(2, 512, 10, 3)
    xd, sd = x[:, :, 0].contiguous().cuda(), spk.cuda()
    lengths = [512, 320]
    audio, idx, probs = model.reconstruct(xd, sd, lengths=lengths, weights='live', mode='greedy', return_probs=True)
    i_h, a_h = idx.cpu().numpy(), audio.cpu().numpy()
    assert (i_h[1, 320:] == -1).all() and (a_h[1, 320:] == 0).all() and (i_h[0] >= 0).all() and (i_h[1, :320] >= 0).all()
    inside = i_h >= 0
    want = LR.decode(np.maximum(i_h, 0), 512)
    np.testing.assert_allclose(a_h[inside], want[inside], rtol=1e-5, atol=1e-6)
    dec = pkg.kernels.mu_law_decode_f32(idx.clamp(min=0).float(), levels=512)
    assert torch.equal(audio[idx >= 0].view(torch.int32), dec[idx >= 0].view(torch.int32))
    assert np.array_equal(probs.cpu().numpy().argmax(-1)[inside], i_h[inside])      # greedy equals argmax
    assert i_h.max() < 512
    u = torch.rand(2, 512, generator=torch.Generator().manual_seed(1)).cuda()
    sa, si = model.reconstruct(xd, sd, lengths=lengths, weights='live', mode='sample', uniforms=u)
    s_h = si.cpu().numpy()
    assert (s_h[1, 320:] == -1).all() and float(sa[1, 320:].abs().max()) == 0 and s_h.max() > 255
    np.testing.assert_allclose(sa.cpu().numpy()[s_h >= 0], LR.decode(np.maximum(s_h, 0), 512)[s_h >= 0], rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------ command line
def test_cli_train_then_generate_at_512(tmp_path):
    """train.py for 4 steps, then generate.py -audio, with "quantization_channels": 512 in wavenet_parameters.json (the whole
    interface): every sample of the wav is a decode value of the 512-level alphabet."""
    from scipy.io import wavfile
    w = {"verbose": False, "quantization_channels": 512, "num_cycles": 1, "num_cycle_layers": 4,
         "dilation_rates": [1, 2, 4, 8], "kernel_size": 3, "dilation_filters": 64, "skip_filters": 128,
         "residual_filters": 64, "preprocess": {"kernel_size": 32, "filters": 64}}
    m = {"encoder": "64", "use_vq": True, "speaker_embedding": 16, "k": 32, "latent_dim": 16, "beta": 0.25,
         "encoder_filters": 48, "wavenet_parameters": str(tmp_path / 'w.json'), "verbose": False,
         "learning_rate_schedule": {"0": 1e-3}}
    (tmp_path / 'w.json').write_text(json.dumps(w))
    (tmp_path / 'm.json').write_text(json.dumps(m))
    env = dict(os.environ, PYTHONPATH=ROOT)
    cwd = str(tmp_path)
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'train.py'), '-dataset', 'synthetic', '-length', '512',
                          '-batch', '2', '-step', '4', '-interval', '2', '-save', 'saved_model/weights', '-params',
                          str(tmp_path / 'm.json')], cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    ckpt = tmp_path / 'saved_model' / 'weights-4.pt'
    assert ckpt.exists()
    (tmp_path / 'data').mkdir()
    (tmp_path / 'data' / 'vctk_speakers.txt').write_text('p225, 3\np226, 5\n')
    t = np.arange(1100) / 16000.0
    wavfile.write(str(tmp_path / 'a.wav'), 16000, (np.sin(2 * np.pi * 220 * t) * 8000).astype(np.int16))
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'generate.py'), '-restore', str(ckpt), '-audio',
                          str(tmp_path / 'a.wav'), '-speakers', 'p226', '-mode', 'sample', '-seed', '1', '-params',
                          str(tmp_path / 'm.json')], cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    sr, gen = wavfile.read(str(tmp_path / 'saved_model' / '4_p226.wav'))
    assert sr == 16000 and gen.dtype == np.float32 and gen.shape == (1024,) and np.isfinite(gen).all()

    def off_alphabet(Q):
        alpha = np.sort(LR.decode(np.arange(Q + 1), Q).astype(np.float64))
        j = np.clip(np.searchsorted(alpha, gen), 1, len(alpha) - 1)
        d = np.minimum(np.abs(gen - alpha[j - 1]), np.abs(gen - alpha[j]))
        return d > 1e-6 + 1e-5 * np.abs(gen)
    assert not off_alphabet(512).any(), 'samples that are no decode value of the 512-level alphabet'
    assert off_alphabet(256).mean() > 0.5, 'the wav could as well be 256-level audio: the check shows nothing'
