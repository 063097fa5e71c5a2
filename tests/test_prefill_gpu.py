"""GPU tests of prompted generation: FastGenerator.prefill / PriorGenerator.prefill (VQVAE.decoder_states over the prompt's
window + vqw_ar_decode_prefill_layer / _finish into the rings of csrc/ar_persist.hip and csrc/ar_decode.hip).

The contract: after prefill(prompt of T steps) a handle is in the state of reset + T steps teacher-forced on the prompt.  The
oracle generators are stepped through the same prompt and then teacher-forced with the GPU's own outputs: every greedy GPU
index must be the oracle's argmax unless the top two oracle probabilities are within 2e-6 (fp32 noise, as in
test_prior_gpu.py); the distribution right after prefill is the oracle's (rtol 1e-4, atol 1e-7)."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import ref_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
N_ROWS = 12               # enough one-row handles (VQW_AR_ROWS=1) for two waves of a persistent launch
LENGTH = 1280             # 20 condition frames: covers a 1000-step prompt + 200 generated steps


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def prior_tests():
    return _load('prior_gpu_tests', os.path.join(HERE, 'test_prior_gpu.py'))


@pytest.fixture(scope='module')
def tiny(pkg):
    m, w = _load('make_golden', os.path.join(HERE, 'golden', 'make_golden.py')).tiny_cfg()
    P = M.init_params(m, w, 10, seed=11, randomize_all=True)
    model = pkg.model.VQVAE(m, w, 10, device='cuda', seed=0)
    model.load_named(P)
    x, spk, _ = M.synthetic_batch(N_ROWS, LENGTH, 10, 1234)
    enc = model.encode(x[:, :, 0].contiguous().cuda(), spk.cuda())
    with torch.no_grad():
        enc_ref = M.forward(x, spk, P, m, w)['local_condition']          # [B,Tz,Cc]
    return model, P, w, enc, enc_ref


def prompts(B, T, seed):
    """Random audio in [-1, 1], a different prompt per row."""
    return (torch.rand(B, T, generator=torch.Generator().manual_seed(seed)) * 2 - 1).float()


def oracle_after_prompt(P, w, enc_ref, prompt):
    """The oracle generator stepped (teacher-forced) through the prompt; returns it and the input of the next step."""
    B, T = prompt.shape
    g = M.FastGenerator(P, w, B)
    a = torch.zeros(B, 1)
    with torch.no_grad():
        for t in range(T):
            g.step(a, enc_ref[:, t // 64])
            a = prompt[:, t:t + 1]
    return g, a


def check_greedy(g, a, enc_ref, T, got_idx, got_audio):
    """Teacher-force the oracle with the GPU's outputs from step T on; every GPU index is the argmax up to a 2e-6 tie."""
    with torch.no_grad():
        for i in range(got_idx.shape[1]):
            pr = g.step(a, enc_ref[:, (T + i) // 64]).numpy()
            for b in range(pr.shape[0]):
                assert pr[b].max() - pr[b, got_idx[b, i]] <= 2e-6, \
                    'T %d step %d row %d: GPU %d, oracle argmax %d' % (T, T + i, b, got_idx[b, i], pr[b].argmax())
            a = torch.from_numpy(got_audio[:, i:i + 1])
    return g


# ------------------------------------------------------------------ 2. teacher-forced parity, both back ends
@pytest.mark.parametrize('persistent', ['1', '0'])
@pytest.mark.parametrize('T', [0, 37, 1000])
def test_prefill_matches_teacher_forced_oracle(pkg, tiny, monkeypatch, persistent, T):
    monkeypatch.setenv('VQW_AR_PERSISTENT', persistent)
    model, P, w, enc, enc_ref = tiny
    enc, enc_ref = enc[:2].contiguous(), enc_ref[:2]
    prompt = prompts(2, T, 5 + T)
    gen = pkg.generator.FastGenerator(model, batch=2)
    assert (pkg._lib.lib().vqw_ar_decode_workgroups(gen._hs[0]) > 0) == (persistent == '1')
    g, a = oracle_after_prompt(P, w, enc_ref, prompt)
    gen.prefill(prompt.cuda(), enc)
    _, _, probs = gen.generate(enc, 1, return_probs=True)
    with torch.no_grad():
        want = M.FastGenerator.step(g, a, enc_ref[:, T // 64]).numpy()
    np.testing.assert_allclose(probs.cpu().numpy(), want, rtol=1e-4, atol=1e-7)
    g, a = oracle_after_prompt(P, w, enc_ref, prompt)
    gen.prefill(prompt.cuda(), enc)                 # again, after a run: prefill starts from reset
    audio, idx = gen.generate(enc, 200)
    gen.close()
    check_greedy(g, a, enc_ref, T, idx.cpu().numpy(), audio.cpu().numpy())


# ------------------------------------------------------------------ 3. layouts: one-row / multi-row handles, two waves
@pytest.mark.parametrize('persistent, rows, B', [('1', None, 2), ('1', '2', 2), ('0', '2', 2), ('1', '1', N_ROWS)])
def test_prefill_layouts(pkg, tiny, monkeypatch, persistent, rows, B):
    monkeypatch.setenv('VQW_AR_PERSISTENT', persistent)
    if rows:
        monkeypatch.setenv('VQW_AR_ROWS', rows)
    model, P, w, enc, enc_ref = tiny
    enc, enc_ref = enc[:B].contiguous(), enc_ref[:B]
    T = 300
    prompt = prompts(B, T, 77)
    gen = pkg.generator.FastGenerator(model, batch=B)
    if B == N_ROWS:
        assert len(gen._waves) == 2 and gen._parts == [1] * N_ROWS
    gen.prefill(prompt.cuda(), enc)
    audio, idx = gen.generate(enc, 100)
    gen.close()
    g, a = oracle_after_prompt(P, w, enc_ref, prompt)
    check_greedy(g, a, enc_ref, T, idx.cpu().numpy(), audio.cpu().numpy())


# ------------------------------------------------------------------ 4. reference widths: the window is wide enough
@pytest.mark.parametrize('persistent', ['1', '0'])
def test_prefill_self_consistent_at_reference_widths(pkg, monkeypatch, persistent):
    monkeypatch.setenv('VQW_AR_PERSISTENT', persistent)
    cfg, wcfg = pkg.model.load_configs(os.path.join(ROOT, 'model_parameters.json'))
    model = pkg.model.VQVAE(cfg, wcfg, 109, device='cuda', seed=0)
    N, Mn = 7000, 300
    x, spk, _ = M.synthetic_batch(1, 7424, 109, 4321)
    enc = model.encode(x[:, :, 0].contiguous().cuda(), spk.cuda())
    gen = pkg.generator.FastGenerator(model, batch=1)
    audio, idx = gen.generate(enc, N + Mn)
    gen.reset()
    gen.prefill(audio[:, :N].contiguous(), enc)
    _, cont = gen.generate(enc, Mn)
    want, got = idx[0, N:].cpu().numpy(), cont[0].cpu().numpy()
    bad = np.nonzero(want != got)[0]
    if bad.size:                       # a divergence is only allowed at a demonstrated near-tie of the first run
        j = int(bad[0])
        gen.prefill(audio[:, :N + j].contiguous(), enc)
        _, _, p = gen.generate(enc, 1, return_probs=True)
        p = p[0].cpu().double().numpy()
        assert abs(p[want[j]] - p[got[j]]) <= 2e-6, \
            'continuation differs at step %d of %d: %d vs %d (p %.7g, %.7g)' % (j, Mn, got[j], want[j], p[got[j]], p[want[j]])
    gen.close()


# ------------------------------------------------------------------ 5. the prior
@pytest.mark.parametrize('pre_k', [1, 3])
@pytest.mark.parametrize('T', [0, 50, 300])
def test_prior_prefill_matches_restatement(pkg, monkeypatch, pre_k, T):
    pt = prior_tests()
    cfg = pt.tiny_prior(k=32, pre_k=pre_k)
    prior = pkg.prior.LatentPrior(cfg, 10, device='cuda', seed=0)
    P = pt.random_params(prior, 11)
    prior.load_named(P)
    spk = torch.tensor([2, 9])
    sd = spk.cuda()
    cond = P['prior/speaker_embedding'][spk]
    codes = pt.rand_codes(2, T, 32, 3 + T) if T else torch.zeros(2, 0, dtype=torch.int64)
    n = 40                                           # T = 50: crosses the 64-code frame boundary

    def ref_after_prompt():
        g = pt.RefPriorGen(P, cfg, 2)
        prev = [-1, -1]
        with torch.no_grad():
            for t in range(T):
                g.step(prev, cond)
                prev = list(codes[:, t].numpy())
        return g, prev

    gen = pkg.generator.PriorGenerator(prior, batch=2)
    seen = []
    real = prior.speaker_condition
    monkeypatch.setattr(prior, 'speaker_condition', lambda s, Tz: (seen.append(Tz), real(s, Tz))[1])
    gen.prefill(codes.int().cuda(), sd)
    assert gen._t == T
    got = gen.sample(n, sd).cpu().numpy()
    assert seen[-1] == -(-(T + n) // 64)              # the condition is sized from the prefilled step
    g, prev = ref_after_prompt()
    with torch.no_grad():
        for i in range(n):
            pr = g.step(prev, cond).numpy()
            for b in range(2):
                assert pr[b].max() - pr[b, got[b, i]] <= 2e-6, 'T %d step %d row %d' % (T, i, b)
            prev = list(got[:, i])
    u = torch.rand(2, n, generator=torch.Generator().manual_seed(T))
    gen.prefill(codes.int().cuda(), sd)
    si = gen.sample(n, sd, mode='sample', uniforms=u.cuda()).cpu().numpy()
    gen.close()
    g, prev = ref_after_prompt()
    with torch.no_grad():
        for i in range(n):
            cdf = np.cumsum(g.step(prev, cond).numpy(), axis=1)
            for b in range(2):
                want = min(int(cdf[b].searchsorted(u[b, i].item())), 31)
                if want != si[b, i]:
                    assert np.abs(cdf[b] - u[b, i].item()).min() < 2e-6, 'T %d step %d row %d: %d vs %d' % (T, i, b, si[b, i], want)
            prev = list(si[:, i])


def test_prior_prefill_refuses_codes_out_of_range(pkg):
    pt = prior_tests()
    prior = pkg.prior.LatentPrior(pt.tiny_prior(k=32, pre_k=3), 10, device='cuda', seed=0)
    gen = pkg.generator.PriorGenerator(prior, batch=2)
    sd = torch.tensor([1, 2], device='cuda')
    for bad in (32, -1):
        codes = torch.zeros(2, 10, dtype=torch.int32, device='cuda')
        codes[1, 4] = bad
        with pytest.raises(ValueError, match='codes'):
            gen.prefill(codes, sd)
    gen.close()


# ------------------------------------------------------------------ 6. prefill changes nothing that exists
@pytest.mark.parametrize('persistent', ['1', '0'])
def test_prefill_then_reset_and_empty_prefill_are_reset(pkg, tiny, monkeypatch, persistent):
    monkeypatch.setenv('VQW_AR_PERSISTENT', persistent)
    model, _, _, enc, _ = tiny
    enc = enc[:2].contiguous()
    u = torch.rand(2, 150, generator=torch.Generator().manual_seed(1)).cuda()
    fresh = pkg.generator.FastGenerator(model, batch=2)
    a0, i0, p0 = fresh.generate(enc, 150, mode='sample', uniforms=u, return_probs=True)
    fresh.close()
    gen = pkg.generator.FastGenerator(model, batch=2)
    gen.prefill(prompts(2, 500, 3).cuda(), enc)
    gen.reset()
    a1, i1, p1 = gen.generate(enc, 150, mode='sample', uniforms=u, return_probs=True)
    gen.prefill(prompts(2, 700, 4).cuda(), enc)
    gen.generate(enc, 20)
    gen.prefill(torch.zeros(2, 0, device='cuda'), enc)
    a2, i2, p2 = gen.generate(enc, 150, mode='sample', uniforms=u, return_probs=True)
    gen.close()
    for a, i, p in ((a1, i1, p1), (a2, i2, p2)):
        assert torch.equal(i, i0) and torch.equal(a, a0) and torch.equal(p, p0)


# ------------------------------------------------------------------ 7. command line
def test_cli_prompted_generation(tmp_path):
    from scipy.io import wavfile
    pt = prior_tests()
    w = {"verbose": False, "quantization_channels": 256, "num_cycles": 1, "num_cycle_layers": 4,
         "dilation_rates": [1, 2, 4, 8], "kernel_size": 3, "dilation_filters": 32, "skip_filters": 64,
         "residual_filters": 32, "preprocess": {"kernel_size": 32, "filters": 32}}
    m = {"encoder": "64", "use_vq": True, "speaker_embedding": 16, "k": 32, "latent_dim": 16, "beta": 0.25,
         "encoder_filters": 48, "wavenet_parameters": str(tmp_path / 'w.json'), "verbose": False,
         "learning_rate_schedule": {"0": 1e-3}}
    (tmp_path / 'w.json').write_text(json.dumps(w))
    (tmp_path / 'm.json').write_text(json.dumps(m))
    (tmp_path / 'p.json').write_text(json.dumps(pt.tiny_prior(k=32, pre_k=2)))
    env = dict(os.environ, PYTHONPATH=ROOT)
    cwd = str(tmp_path)
    run = lambda args: subprocess.run([sys.executable] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)  # noqa: E731
    out = run([os.path.join(ROOT, 'train.py'), '-dataset', 'synthetic', '-length', '512', '-batch', '2', '-step', '2',
               '-interval', '2', '-save', 'saved_model/weights', '-params', str(tmp_path / 'm.json')])
    assert out.returncode == 0, out.stderr[-2000:]
    out = run([os.path.join(ROOT, 'train_prior.py'), '-restore', 'saved_model/weights-2.pt', '-dataset', 'synthetic',
               '-length', '128', '-batch', '2', '-step', '2', '-interval', '2', '-save', 'saved_prior/prior',
               '-params', str(tmp_path / 'p.json'), '-vqvae_params', str(tmp_path / 'm.json')])
    assert out.returncode == 0, out.stderr[-2000:]
    (tmp_path / 'data').mkdir()
    (tmp_path / 'data' / 'vctk_speakers.txt').write_text('p225, 3\np226, 5\n')
    t = np.arange(1100) / 16000.0
    pcm = (np.sin(2 * np.pi * 220 * t) * 8000).astype(np.int16)
    wavfile.write(str(tmp_path / 'a.wav'), 16000, pcm)
    utt = pcm[:1024].astype(np.float32) / 32768.0                     # the trimmed utterance generate.py reads
    common = ['-restore', 'saved_model/weights-2.pt', '-audio', 'a.wav', '-params', str(tmp_path / 'm.json')]
    out = run([os.path.join(ROOT, 'generate.py')] + common + ['-speakers', 'p226', 'None', '-mode', 'sample', '-seed', '1',
                                                             '-prompt_samples', '300'])
    assert out.returncode == 0, out.stderr[-2000:]
    for s in ('p226', 'no_speaker'):
        sr, a = wavfile.read(str(tmp_path / 'saved_model' / ('2_%s.wav' % s)))
        assert sr == 16000 and a.shape == (1024,) and np.isfinite(a).all()
        assert np.array_equal(a[:300], utt[:300])
    for n in ('1024', '1025'):
        out = run([os.path.join(ROOT, 'generate.py')] + common + ['-speakers', 'p225', '-mode', 'greedy', '-prompt_samples', n])
        assert out.returncode == 2 and 'not shorter than the trimmed utterance' in out.stderr, out.stderr[-2000:]
    prior_args = ['-prior', 'saved_prior/prior-2.pt', '-prior_params', str(tmp_path / 'p.json'), '-frames', '6']
    out = run([os.path.join(ROOT, 'generate.py')] + common + prior_args + ['-speakers', 'p225', 'p226', '-mode', 'sample',
                                                                          '-seed', '2', '-prompt_frames', '5'])
    assert out.returncode == 0, out.stderr[-2000:]
    sys.path.insert(0, ROOT)
    pkg = importlib.import_module('vq-vae-wavenet_amd')
    cfg, wcfg = pkg.model.load_configs(str(tmp_path / 'm.json'))
    model = pkg.model.VQVAE(cfg, wcfg, 109, device='cuda', seed=0)
    model.load_state_dict(torch.load(str(tmp_path / 'saved_model' / 'weights-2.pt'), map_location='cpu', weights_only=True))
    model.use_ema_weights()
    want = model.encode_codes(torch.from_numpy(utt).cuda().unsqueeze(0), torch.tensor([3], device='cuda'))[0, :5].cpu().numpy()
    for s in ('p225', 'p226'):
        c = np.load(str(tmp_path / 'saved_model' / ('prior_codes_2_%s.npy' % s)))
        assert c.shape == (11,) and np.array_equal(c[:5], want) and c.min() >= 0 and c.max() < 32
        sr, a = wavfile.read(str(tmp_path / 'saved_model' / ('2_%s_prior.wav' % s)))
        assert a.shape == (11 * 64,) and np.array_equal(a[:320], utt[:320]) and np.isfinite(a).all()
    out = run([os.path.join(ROOT, 'generate.py')] + common + prior_args + ['-speakers', 'p225', '-prompt_frames', '17'])
    assert out.returncode == 2 and 'longer than the trimmed utterance' in out.stderr, out.stderr[-2000:]
