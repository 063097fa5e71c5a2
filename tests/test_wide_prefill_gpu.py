"""GPU tests of the wide generators' prefill: WideGenerator.prefill_prompt / WidePriorGenerator.prefill_codes
(WaveNet.decoder_states over the prompt's window, chunk_rows rows at a time, scattered by vqw_ar_wide_prefill_layer / _finish into the batch-row-innermost
state of csrc/ar_wide.hip) and `generate.py -takes`.

The contract: after prefill(prompt of T steps) a wide handle is in the state of reset + T steps teacher-forced on the prompt.
A wide handle cannot step through a prompt, so nothing here does: the judge is the float64 PARALLEL reference of gen_ref.py,
the training graph over concat(prompt, what the generator then produced), which shares nothing with rings, slots or
windows.  Bars: those of test_wide_gen_gpu.py (every sampled index is searchsorted(cumsum(p64), u), excused only where u lies
within gen_ref.EDGE of a cdf value, at most 0.2 % of B * n; probs_last within rtol 2e-4, atol 1e-7).  Everything that is
promised bit for bit (chunking of the rows, batch size, row position, reset hygiene, chunked runs) is held with torch.equal.

Tiny widths: R 32, S 64, Q 256, Cc 32, pre_k 32, dilations [1,2,4,8,16] * 2, ks 3, ratio 16; B = 70 (three column tiles, the
last partial; three scatter row tiles, the last partial); 25 condition frames.  The window is W = 2 * 62 + 32 = 156, the
deepest ring has 32 slots.  T + 96 passes 400 steps for T = 333: the generator keeps the last frame for steps beyond the
encoding, and the reference is given that frame repeated."""
import importlib
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

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIL = [1, 2, 4, 8, 16] * 2
DEPTHS = G.ring_depths(3, DIL, persistent=False)
B70, RATIO, FRAMES, N = 70, 16, 25, 96
STEPS = FRAMES * RATIO        # 400
MAX_EXCUSED = 0.002           # of B * n
T_ALL = [0, 1, 5, 31, 32, 33, 100, 156, 157, 200, 333]
PT = G.prior_tests()


def configs(R, S, ks, dil, Q=256):
    m, w = G.tiny_cfg()
    w.update(dilation_rates=list(dil), num_cycles=2, num_cycle_layers=len(dil) // 2, kernel_size=ks, dilation_filters=R,
             residual_filters=R, skip_filters=S, quantization_channels=Q, preprocess={"kernel_size": 32, "filters": R})
    return m, w


@pytest.fixture(scope='module')
def decoders(pkg):
    made = {}

    def get(Q=256):
        if Q not in made:
            m, w = configs(32, 64, 3, DIL, Q)
            P = M.init_params(m, w, 10, seed=163 + Q, randomize_all=True)
            model = pkg.model.VQVAE(m, w, 10, device='cuda', seed=0)
            model.load_named(P)
            assert model.levels == Q
            made[Q] = (model, P, w)
        return made[Q]
    yield get
    made.clear()
    torch.cuda.empty_cache()


def prompts(B, T, seed):
    """Random audio in [-1, 1], a different prompt per row."""
    return (torch.rand(B, T, generator=torch.Generator().manual_seed(seed)) * 2 - 1).float()


def inputs(model, B, seed):
    g = torch.Generator().manual_seed(seed)
    enc = 0.5 * torch.randn(B, model.Cc, FRAMES, generator=g)            # [B][Cc][Tz]: no encoder run needed
    u = torch.rand(B, N, generator=g)
    return enc, u


@pytest.fixture(scope='module')
def case70(pkg, decoders):
    """The inputs every tiny test shares, one B = 70 generator, and the continuation of T = 200 (default chunking)."""
    model, P, w = decoders()
    enc, u = inputs(model, B70, 77)
    prompt = prompts(B70, STEPS, 78)
    gen = pkg.generator.WideGenerator(model, batch=B70)
    d = dict(model=model, P=P, w=w, enc=enc, u=u, prompt=prompt, gen=gen, enc_d=enc.cuda(), u_d=u.cuda(), prompt_d=prompt.cuda())
    d['cont200'] = continuation(gen, d, 200)
    yield d
    gen.close()


def continuation(gen, d, T, rows=slice(None), **kw):
    """prefill(T) then N sampled steps of `rows` of the shared inputs: (audio, indices, probs of the last step)."""
    gen.prefill_prompt(d['prompt_d'][rows, :T].contiguous(), d['enc_d'][rows].contiguous(), ratio=RATIO, **kw)
    return gen.generate(d['enc_d'][rows].contiguous(), N, mode='sample', uniforms=d['u_d'][rows].contiguous(), ratio=RATIO,
                        return_probs=True)


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def probs_and_labels64(P, w, audio, enc):
    """gen_ref.decoder_probs64 that also returns the labels the graph forms from the audio.  audio [B][n], enc [B][Cc][Tz]."""
    B, n = audio.shape
    x = torch.as_tensor(audio).double().reshape(B, n, 1)
    with torch.no_grad():
        logits, labels = M.wavenet_build(x, enc.permute(0, 2, 1).double(), G.to64(P), w)
        p = torch.softmax(logits.reshape(B, n, -1), dim=-1)
    assert p.dtype == torch.float64
    return p.numpy(), labels.reshape(B, n).numpy().astype(np.int64)


def reference_after(P, w, enc, prompt, T, audio):
    """p64 and labels of steps T .. T+n-1 of concat(prompt[:, :T], audio, zeros): causal, so the padding cannot matter.  Past
    the encoding's last frame the generator keeps that frame: the reference gets it repeated."""
    B, n = audio.shape
    frames = max(FRAMES, -(-(T + n) // RATIO))
    full = np.zeros((B, frames * RATIO), np.float32)
    full[:, :T] = prompt[:, :T].numpy()
    full[:, T:T + n] = audio
    enc_ref = torch.cat([enc, enc[:, :, -1:].expand(-1, -1, frames - FRAMES)], 2) if frames > FRAMES else enc
    p64, labels = probs_and_labels64(P, w, full, enc_ref)
    return p64[:, T:T + n], labels[:, T:T + n]


# ------------------------------------------------------------------ 1. the distribution after prefill
@pytest.mark.parametrize('T', T_ALL)
def test_distribution_after_prefill_is_the_training_graphs(case70, T):
    d = case70
    audio, idx, probs = continuation(d['gen'], d, T)
    idx_h = idx.cpu().numpy()
    p64, labels = reference_after(d['P'], d['w'], d['enc'], d['prompt'], T, audio.cpu().numpy())
    excused = G.check_sampled(p64, d['u'], idx_h, DEPTHS)
    print('\n[wide prefill] T=%d B=%d n=%d: excused %d of %d' % (T, B70, N, excused, B70 * N))
    assert excused <= MAX_EXCUSED * B70 * N, '%d of %d steps needed the cdf-edge excuse' % (excused, B70 * N)
    assert np.array_equal(labels, idx_h.astype(np.int64)), 'mu_law_encode(generated audio) is not the index drawn'
    np.testing.assert_allclose(probs.cpu().numpy(), p64[:, -1], rtol=2e-4, atol=1e-7, err_msg='distribution of the last step')


# ------------------------------------------------------------------ 2. the scatter: an exact, chunk-independent copy
def c_prefill(pkg, gen, nets, s0, T, tail, chunks):
    """reset + vqw_ar_wide_prefill_layer for every (chunk, layer) + _finish through ctypes; chunks: [(row0, nrows)]."""
    L = pkg._lib
    lib, st = L.lib(), L.stream()
    L.check(lib.vqw_ar_wide_reset(gen._h, st))
    keep = []
    for row0, n in chunks:
        for l, net in enumerate(nets):
            x = net[row0:row0 + n]
            assert x.is_contiguous()
            keep.append(x)
            L.check(lib.vqw_ar_wide_prefill_layer(gen._h, l, L.ptr(x), x.shape[2], s0, T, row0, n, st))
    L.check(lib.vqw_ar_wide_prefill_finish(gen._h, T, L.ptr(tail), None, st))
    torch.cuda.synchronize()


def test_scatter_is_an_exact_chunk_independent_copy(pkg, case70):
    d = case70
    model, T = d['model'], 200
    nets, first = [], []
    model.decoder_states(d['prompt_d'][:, :T].contiguous(), d['enc_d'], T, lambda l, net, s0: (nets.append(net.clone()), first.append(s0)),
                         RATIO)
    assert len(nets) == len(DIL) and set(first) == {32} and nets[0].shape == (B70, 32, 176)
    tail = d['prompt_d'][:, T - 32:T].contiguous()

    def run(gen, rows=slice(None)):
        return gen.generate(d['enc_d'][rows].contiguous(), N, mode='sample', uniforms=d['u_d'][rows].contiguous(), ratio=RATIO,
                            return_probs=True)
    gen = d['gen']
    c_prefill(pkg, gen, nets, 32, T, tail, [(0, B70)])
    whole = run(gen)
    assert same(whole, d['cont200']), 'the C calls and WideGenerator.prefill_prompt disagree'
    for c in (1, 7, 32, 33):
        chunks = [(max(hi - c, 0), hi - max(hi - c, 0)) for hi in range(B70, 0, -c)]      # descending row order
        assert sum(n for _, n in chunks) == B70 and chunks[0][0] + chunks[0][1] == B70 and chunks[-1][0] == 0
        c_prefill(pkg, gen, nets, 32, T, tail, chunks)
        assert same(run(gen), whole), 'chunks of %d rows' % c
    g5 = pkg.generator.WideGenerator(model, batch=5)
    c_prefill(pkg, g5, [n[:5].contiguous() for n in nets], 32, T, tail[:5].contiguous(), [(0, 5)])
    five = run(g5, slice(0, 5))
    g5.close()
    assert same(five, [t[:5] for t in whole])


# ------------------------------------------------------------------ 3. the Python level inherits it
def test_chunk_rows_and_batch_do_not_change_a_row(pkg, case70):
    d = case70
    gen, want = d['gen'], d['cont200']
    for c in (1, 7, 32, 70, None):
        assert same(continuation(gen, d, 200, chunk_rows=c), want), 'chunk_rows=%r' % (c,)
    g5 = pkg.generator.WideGenerator(d['model'], batch=5)
    five = continuation(g5, d, 200, slice(0, 5))
    g5.close()
    assert same(five, [t[:5] for t in want])
    enc2, u2 = inputs(d['model'], B70, 79)
    prompt2 = prompts(B70, STEPS, 80)
    enc2[65:], u2[65:], prompt2[65:] = d['enc'][:5], d['u'][:5], d['prompt'][:5]
    other = dict(enc_d=enc2.cuda(), u_d=u2.cuda(), prompt_d=prompt2.cuda())
    got = continuation(gen, other, 200)
    assert not torch.equal(got[1][:5], want[1][:5])
    assert same([t[65:] for t in got], [t[:5] for t in want])
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match='chunk_rows'):
            continuation(gen, d, 200, chunk_rows=bad)


# ------------------------------------------------------------------ 4. state hygiene
def test_empty_prefill_is_reset_and_no_stale_slot_survives(pkg, case70):
    d = case70
    gen = d['gen']

    def run(n=N):
        return gen.generate(d['enc_d'], n, mode='sample', uniforms=d['u_d'][:, :n].contiguous(), ratio=RATIO, return_probs=True)
    gen.reset()
    from_reset = run()
    assert same(continuation(gen, d, 0), from_reset)
    fresh = pkg.generator.WideGenerator(d['model'], batch=B70)
    want5 = continuation(fresh, d, 5)
    fresh.close()
    gen.reset()
    gen.generate(d['enc_d'], 300, mode='sample', uniforms=torch.rand(B70, 300, device='cuda'), ratio=RATIO)
    assert same(continuation(gen, d, 5), want5), 'a slot of the 300-step run survived prefill(T = 5)'
    assert not same(want5, from_reset)


def test_chunked_run_after_prefill_equals_single_run(case70):
    """The host's step mirror and the first frame of the condition window after a prefill: T = 100 lies inside frame 6."""
    d = case70
    gen = d['gen']
    single = continuation(gen, d, 100)
    ends = sorted(set(G.checkpoints(N, 3, 16)) | {45})
    assert ends[-1] == N and any((100 + t) % RATIO for t in ends)
    gen.prefill_prompt(d['prompt_d'][:, :100].contiguous(), d['enc_d'], ratio=RATIO)
    aa, ia, prev = [], [], 0
    for t in ends:
        a_c, i_c, p_c = gen.generate(d['enc_d'], t - prev, mode='sample', uniforms=d['u_d'][:, prev:t].contiguous(), ratio=RATIO,
                                     return_probs=True)
        aa.append(a_c)
        ia.append(i_c)
        prev = t
    assert torch.equal(torch.cat(aa, 1), single[0]) and torch.equal(torch.cat(ia, 1), single[1]) and torch.equal(p_c, single[2])


# ------------------------------------------------------------------ 5. levels
def test_first_distribution_at_512_levels_is_fast_generators(pkg, decoders):
    model, _, _ = decoders(512)
    B, T = 5, 100
    enc = (0.5 * torch.randn(B, model.Cc, FRAMES, generator=torch.Generator().manual_seed(5))).cuda()
    prompt = prompts(B, T, 6).cuda()
    wide = pkg.generator.WideGenerator(model, batch=B)
    wide.prefill_prompt(prompt, enc, ratio=RATIO)
    _, _, got = wide.generate(enc, 1, ratio=RATIO, return_probs=True)
    wide.close()
    fast = pkg.generator.FastGenerator(model, batch=B)
    fast.prefill(prompt, enc, ratio=RATIO)
    _, _, want = fast.generate(enc, 1, ratio=RATIO, return_probs=True)
    fast.close()
    assert got.shape == (B, 512)
    np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), rtol=2e-4, atol=1e-7)


# ------------------------------------------------------------------ 6. reference widths, once
def test_reference_widths_against_fast_generator_prefill(pkg):
    """model_parameters.json, B = 3, T = 7000: the window is saturated and starts inside the prompt (s0 > 0).  The judge is
    FastGenerator.prefill on the prompt plus the wide generator's own audio; nothing is stepped through the prompt."""
    cfg, wcfg = pkg.model.load_configs(os.path.join(ROOT, 'model_parameters.json'))
    model = pkg.model.VQVAE(cfg, wcfg, 109, device='cuda', seed=0)
    B, T, n = 3, 7000, 150
    x, spk, _ = M.synthetic_batch(B, 7424, 109, 4321)
    enc = model.encode(x[:, :, 0].contiguous().cuda(), spk.cuda())
    W, s0, _ = pkg.wavenet.prefill_window(T, model.ks, model.dil, model.pre_k, 64)
    assert 0 < s0 and W < T
    prompt = prompts(B, T, 12).cuda()
    u = torch.rand(B, n + 1, generator=torch.Generator().manual_seed(13)).cuda()
    wide = pkg.generator.WideGenerator(model, batch=B)
    fast = pkg.generator.FastGenerator(model, batch=B)
    wide.prefill_prompt(prompt, enc)
    audio, prev = [], 0
    for end in (1, 2, n, n + 1):          # one-step chunks at k = 0, 1 and n wide samples: their probs are the next distribution
        a_c, _, p_c = wide.generate(enc, end - prev, mode='sample', uniforms=u[:, prev:end].contiguous(), return_probs=True)
        if end - prev == 1:
            so_far = torch.cat([prompt] + audio, 1).contiguous()
            assert so_far.shape[1] == T + prev and prev in (0, 1, n)
            fast.prefill(so_far, enc)
            _, _, want = fast.generate(enc, 1, return_probs=True)
            np.testing.assert_allclose(p_c.cpu().numpy(), want.cpu().numpy(), rtol=2e-4, atol=1e-7,
                                       err_msg='distribution after the prompt and %d wide samples' % prev)
        audio.append(a_c)
        prev = end
    wide.close()
    fast.close()


# ------------------------------------------------------------------ 7. the prior
@pytest.fixture(scope='module')
def priors(pkg):
    made = {}

    def get(pre_k):
        if pre_k not in made:
            cfg = PT.tiny_prior(k=32, pre_k=pre_k)
            prior = pkg.prior.LatentPrior(cfg, 10, device='cuda', seed=0)
            P = PT.random_params(prior, 21)
            prior.load_named(P)
            made[pre_k] = (prior, P, cfg, pkg.generator.WidePriorGenerator(prior, batch=33))
        return made[pre_k]
    yield get
    for v in made.values():
        v[3].close()
    made.clear()
    torch.cuda.empty_cache()


@pytest.mark.parametrize('pre_k', [1, 3])
@pytest.mark.parametrize('T', [0, 1, 3, 50, 64, 65, 300])
def test_prior_distribution_after_prefill(priors, pre_k, T):
    prior, P, cfg, gen = priors(pre_k)
    B, n, k = 33, 64, 32
    spk = torch.tensor([i % 10 for i in range(B)], dtype=torch.int64)
    codes = PT.rand_codes(B, T, k, 3 + T) if T >= 3 else torch.randint(0, k, (B, T), generator=torch.Generator().manual_seed(T))
    u = torch.rand(B, n, generator=torch.Generator().manual_seed(100 + T))
    gen.prefill_codes(codes.int().cuda(), spk.cuda())
    assert gen._t == T
    idx, probs = gen.sample(n, spk.cuda(), mode='sample', uniforms=u.cuda(), return_probs=True)
    assert gen._t == T + n
    idx_h = idx.cpu().numpy()
    assert idx_h.min() >= 0 and idx_h.max() < k
    total = -(-(T + n) // 64) * 64                       # prior_probs64 wants whole frames: code 0 behind the run (causal)
    full = np.zeros((B, total), np.int64)
    full[:, :T] = codes.numpy()
    full[:, T:T + n] = idx_h
    p64 = G.prior_probs64(P, cfg, full, spk)[:, T:T + n]
    excused = G.check_sampled(p64, u, idx_h, G.ring_depths(3, cfg['dilation_rates'], persistent=False))
    print('\n[wide prior prefill] pre_k=%d T=%d: excused %d of %d' % (pre_k, T, excused, B * n))
    assert excused <= MAX_EXCUSED * B * n, '%d of %d steps needed the cdf-edge excuse' % (excused, B * n)
    np.testing.assert_allclose(probs.cpu().numpy(), p64[:, -1], rtol=2e-4, atol=1e-7, err_msg='distribution of the last step')


def test_prior_prefill_refuses_codes_out_of_range(priors):
    _, _, _, gen = priors(3)
    sd = torch.tensor([i % 10 for i in range(33)], device='cuda')
    for bad in (32, -1):
        codes = torch.zeros(33, 10, dtype=torch.int32, device='cuda')
        codes[17, 4] = bad
        with pytest.raises(ValueError, match=r'codes must lie in \[0, 32\)'):
            gen.prefill_codes(codes, sd)
    with pytest.raises(ValueError, match='int32'):
        gen.prefill_codes(torch.zeros(33, 10, dtype=torch.int64, device='cuda'), sd)
    with pytest.raises(ValueError, match='34 speaker ids'):
        gen.prefill_codes(torch.zeros(33, 10, dtype=torch.int32, device='cuda'), torch.zeros(34, dtype=torch.int64, device='cuda'))


# ------------------------------------------------------------------ 8. refusals of the C calls
def test_c_calls_refuse_by_name_before_the_device(pkg, case70, priors):
    """Every refusal of vqw_ar_wide_prefill_layer / _finish names the value; none reaches the device: the handle, reset
    before them, still generates what a reset handle generates."""
    d = case70
    L = pkg._lib
    lib, st = L.lib(), L.stream()
    gen = d['gen']
    gen.reset()
    h = gen._h
    x = torch.full((B70, 32, 176), 7.0, device='cuda')
    tail = torch.full((B70, 32), 0.5, device='cuda')
    codes = torch.zeros(B70, 32, dtype=torch.int32, device='cuda')
    layer = [  # (l, ld, t_first, t_end, row0, nrows), message
        ((-1, 176, 32, 200, 0, 70), 'layer -1 outside 0..9'), ((10, 176, 32, 200, 0, 70), 'layer 10 outside 0..9'),
        ((0, 176, 32, -1, 0, 70), 't_end=-1'), ((0, 176, -1, 200, 0, 70), 't_first=-1'),
        ((9, 176, 169, 200, 0, 70), "columns [169, 345) do not cover layer 9's steps [168, 200)"),
        ((9, 167, 32, 200, 0, 70), "columns [32, 199) do not cover layer 9's steps [168, 200)"),
        ((0, 176, 32, 200, 0, 0), 'nrows=0'), ((0, 176, 32, 200, 0, -3), 'nrows=-3'),
        ((0, 176, 32, 200, -1, 5), 'rows [-1, 4) outside'), ((0, 176, 32, 200, 66, 5), 'rows [66, 71) outside'),
        ((0, 176, 32, 200, 0, 71), 'rows [0, 71) outside'), ((0, 176, 32, 200, 70, 1), 'rows [70, 71) outside')]
    for (l, ld, t_first, t_end, row0, nrows), match in layer:
        assert lib.vqw_ar_wide_prefill_layer(h, l, L.ptr(x), ld, t_first, t_end, row0, nrows, st) != 0, match
        msg = lib.vqw_last_error().decode()
        assert msg.startswith('vqw_ar_wide_prefill_layer: ') and match in msg, msg
    assert lib.vqw_ar_wide_prefill_layer(None, 0, L.ptr(x), 176, 32, 200, 0, 70, st) != 0 and b'null handle' in lib.vqw_last_error()
    assert lib.vqw_ar_wide_prefill_layer(h, 0, None, 176, 32, 200, 0, 70, st) != 0 and b'null x' in lib.vqw_last_error()
    finish = [((-1, L.ptr(tail), None), 't_end=-1'), ((200, None, None), 'neither is'), ((200, L.ptr(tail), L.ptr(codes)), 'both are'),
              ((200, None, L.ptr(codes)), 'an audio handle takes audio_tail')]
    for (t_end, a, c), match in finish:
        assert lib.vqw_ar_wide_prefill_finish(h, t_end, a, c, st) != 0, match
        msg = lib.vqw_last_error().decode()
        assert msg.startswith('vqw_ar_wide_prefill_finish: ') and match in msg, msg
    assert lib.vqw_ar_wide_prefill_finish(None, 0, L.ptr(tail), None, st) != 0 and b'null handle' in lib.vqw_last_error()
    pgen = priors(3)[3]
    assert lib.vqw_ar_wide_prefill_finish(pgen._h, 5, L.ptr(tail), None, st) != 0
    assert 'a code-input handle takes code_tail' in lib.vqw_last_error().decode()
    got = gen.generate(d['enc_d'], 40, mode='sample', uniforms=d['u_d'][:, :40].contiguous(), ratio=RATIO, return_probs=True)
    gen.reset()
    want = gen.generate(d['enc_d'], 40, mode='sample', uniforms=d['u_d'][:, :40].contiguous(), ratio=RATIO, return_probs=True)
    assert same(got, want), 'a refused call changed the handle'


# ------------------------------------------------------------------ 9. command line
@pytest.fixture(scope='module')
def checkpoint(tmp_path_factory):
    """A tiny VQ-VAE and a tiny prior trained for two steps, an utterance and a speaker list, as test_prefill_gpu.py makes them."""
    from scipy.io import wavfile
    tmp = tmp_path_factory.mktemp('takes')
    w = {"verbose": False, "quantization_channels": 256, "num_cycles": 1, "num_cycle_layers": 4,
         "dilation_rates": [1, 2, 4, 8], "kernel_size": 3, "dilation_filters": 32, "skip_filters": 64,
         "residual_filters": 32, "preprocess": {"kernel_size": 32, "filters": 32}}
    m = {"encoder": "64", "use_vq": True, "speaker_embedding": 16, "k": 32, "latent_dim": 16, "beta": 0.25,
         "encoder_filters": 48, "wavenet_parameters": str(tmp / 'w.json'), "verbose": False,
         "learning_rate_schedule": {"0": 1e-3}}
    (tmp / 'w.json').write_text(json.dumps(w))
    (tmp / 'm.json').write_text(json.dumps(m))
    (tmp / 'p.json').write_text(json.dumps(PT.tiny_prior(k=32, pre_k=2)))
    env = dict(os.environ, PYTHONPATH=ROOT)

    def run(args):
        return subprocess.run([sys.executable] + args, cwd=str(tmp), env=env, capture_output=True, text=True, timeout=600)
    out = run([os.path.join(ROOT, 'train.py'), '-dataset', 'synthetic', '-length', '512', '-batch', '2', '-step', '2',
               '-interval', '2', '-save', 'saved_model/weights', '-params', str(tmp / 'm.json')])
    assert out.returncode == 0, out.stderr[-2000:]
    out = run([os.path.join(ROOT, 'train_prior.py'), '-restore', 'saved_model/weights-2.pt', '-dataset', 'synthetic',
               '-length', '128', '-batch', '2', '-step', '2', '-interval', '2', '-save', 'saved_prior/prior',
               '-params', str(tmp / 'p.json'), '-vqvae_params', str(tmp / 'm.json')])
    assert out.returncode == 0, out.stderr[-2000:]
    (tmp / 'data').mkdir()
    (tmp / 'data' / 'vctk_speakers.txt').write_text('p225, 3\np226, 5\n')
    t = np.arange(1100) / 16000.0
    pcm = (np.sin(2 * np.pi * 220 * t) * 8000).astype(np.int16)
    wavfile.write(str(tmp / 'a.wav'), 16000, pcm)
    utt = pcm[:1024].astype(np.float32) / 32768.0                     # the trimmed utterance generate.py reads
    common = [os.path.join(ROOT, 'generate.py'), '-restore', 'saved_model/weights-2.pt', '-audio', 'a.wav', '-params', str(tmp / 'm.json')]
    return tmp, run, common, utt


def test_cli_takes_of_an_audio_prompt(checkpoint):
    from scipy.io import wavfile
    tmp, run, common, utt = checkpoint
    args = common + ['-prompt_samples', '300', '-takes', '3', '-speakers', 'p225', 'p226', '-mode', 'sample', '-seed', '1']
    names = ['2_%s_take_%d.wav' % (s, m) for s in ('p225', 'p226') for m in range(3)]
    got = {}
    for rows in ('6', '2'):
        out = run(args + ['-rows', rows])
        assert out.returncode == 0, out.stderr[-2000:]
        got[rows] = []
        for name in names:
            path = tmp / 'saved_model' / name
            got[rows].append(path.read_bytes())
            sr, a = wavfile.read(str(path))
            assert sr == 16000 and a.shape == (1024,) and a.dtype == np.float32 and np.isfinite(a).all()
            assert np.array_equal(a[:300], utt[:300]), '%s does not begin with the prompt' % name
            path.unlink()
    assert got['6'] == got['2'], '-rows changed a take'
    for k in range(2):
        assert len(set(got['6'][3 * k:3 * k + 3])) == 3, 'takes of one speaker are equal'


def test_cli_takes_of_a_prior_prompt(checkpoint):
    from scipy.io import wavfile
    tmp, run, common, utt = checkpoint
    out = run(common + ['-prior', 'saved_prior/prior-2.pt', '-prior_params', str(tmp / 'p.json'), '-frames', '6', '-prompt_frames', '5',
                        '-takes', '2', '-speakers', 'p225', 'p226', '-mode', 'sample', '-seed', '2', '-rows', '3'])
    assert out.returncode == 0, out.stderr[-2000:]
    sys.path.insert(0, ROOT)
    pkg = importlib.import_module('vq-vae-wavenet_amd')
    cfg, wcfg = pkg.model.load_configs(str(tmp / 'm.json'))
    model = pkg.model.VQVAE(cfg, wcfg, 109, device='cuda', seed=0)
    model.load_state_dict(torch.load(str(tmp / 'saved_model' / 'weights-2.pt'), map_location='cpu', weights_only=True))
    model.use_ema_weights()
    want = model.encode_codes(torch.from_numpy(utt).cuda().unsqueeze(0), torch.tensor([3], device='cuda'))[0, :5].cpu().numpy()
    seen = []
    for s in ('p225', 'p226'):
        for m in range(2):
            c = np.load(str(tmp / 'saved_model' / ('prior_codes_2_%s_take_%d.npy' % (s, m))))
            assert c.shape == (11,) and np.array_equal(c[:5], want) and c.min() >= 0 and c.max() < 32
            sr, a = wavfile.read(str(tmp / 'saved_model' / ('2_%s_prior_take_%d.wav' % (s, m))))
            assert sr == 16000 and a.shape == (11 * 64,) and np.array_equal(a[:320], utt[:320]) and np.isfinite(a).all()
            seen.append(a[320:].tobytes())
    assert len(set(seen)) == 4, 'takes are equal'
