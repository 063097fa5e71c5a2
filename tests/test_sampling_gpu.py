"""GPU tests of temperature / top-k / top-p sampling on both generator back ends (the persistent kernel of
csrc/ar_persist.hip; VQW_AR_PERSISTENT=0: ar_sample_kernel of csrc/ar_decode.hip) and on the latent prior's code sampling.

Rows at their defaults must be bitwise today's results, also beside truncated rows in one launch.  Truncated rows are
teacher-forced against the oracle generators (their logits, restated in float64 by sampling_ref.py): every GPU index must be
the restated draw, unless the decision sits on an fp32 edge (u within 2e-6 of a cdf value, a top-p mass within 1e-5 of P,
a p-tie within 1e-7 at the cut); the last step's probabilities are the restated q (rtol 2e-4, atol 1e-7).

Ties at the cut are excused here (the logits are a random network's, an exact tie is an accident, and fp32_edge flags it).
They are held, with nothing excused, on the planted logits of test_sampling_planted_gpu.py."""
import importlib.util
import json
import os
import subprocess
import sys
from unittest import mock

import numpy as np
import pytest
import torch

from oracle import ref_model as M

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampling_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
MIX = (0.7, 20, 0.9)      # row 1 of the mixed runs: temperature, top_k, top_p


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def tiny_cfg():
    return _load('make_golden', os.path.join(HERE, 'golden', 'make_golden.py')).tiny_cfg()


def prior_tests():
    return _load('prior_gpu_tests', os.path.join(HERE, 'test_prior_gpu.py'))


def logits_of(step, *args):
    """The oracle generators end in torch.softmax: run one step with it switched off to get the logits (float64)."""
    with torch.no_grad(), mock.patch.object(torch, 'softmax', lambda x, dim=-1: x):
        return step(*args).double().numpy()


def check_row(z, got, u, t, k, p, where):
    """One truncated decision of the GPU against the restatement; returns the restated (p, keep, q)."""
    pr, keep, q, want = S.restate(z, t, k, p, u)
    if got != want or not keep[got]:
        assert S.fp32_edge(pr, keep, q, k, p, u), '%s: GPU %d, restated %d (kept: %s)' % (where, got, want, keep.nonzero()[0][:8])
    return pr, keep, q


@pytest.fixture(scope='module')
def tiny(pkg):
    m, w = tiny_cfg()
    P = M.init_params(m, w, 10, seed=11, randomize_all=True)
    model = pkg.model.VQVAE(m, w, 10, device='cuda', seed=0)
    model.load_named(P)
    x, spk, _ = M.synthetic_batch(2, 512, 10, 1234)
    enc = model.encode(x[:, :, 0].contiguous().cuda(), spk.cuda())
    with torch.no_grad():
        enc_ref = M.forward(x, spk, P, m, w)['local_condition']          # [B,Tz,Cc]
    return model, P, w, enc, enc_ref


LAYOUTS = [('1', None), ('1', '2'), ('0', '2')]     # (VQW_AR_PERSISTENT, VQW_AR_ROWS): one-row handles / one 2-row handle


# ------------------------------------------------------------------ 1. defaults through the new entry points == today
@pytest.mark.parametrize('persistent', ['1', '0'])
def test_defaults_are_bitwise_plain_sampling(pkg, tiny, monkeypatch, persistent):
    monkeypatch.setenv('VQW_AR_PERSISTENT', persistent)
    model, _, _, enc, _ = tiny
    n = 160
    u = torch.rand(2, n, generator=torch.Generator().manual_seed(4)).cuda()
    gen = pkg.generator.FastGenerator(model, batch=2)
    a0, i0, p0 = gen.generate(enc, n, mode='sample', uniforms=u, return_probs=True)
    outs = []
    for settings in ([(1.0, 0, 1.0)] * 2, [(1.0, 1 << 20, 1.0)] * 2):    # explicit defaults; top_k >= Q is off
        gen.reset()
        audio = torch.empty(2, n, device='cuda')
        idx, probs = gen._run(enc, n, 'sample', u, 64, audio, True, settings)
        outs.append((audio, idx, probs))
    gen.reset()
    outs.append(gen.generate(enc, n, mode='sample', uniforms=u, return_probs=True, top_k=[256, 1000]))
    gen.close()
    for a, i, p in outs:
        assert torch.equal(i, i0) and torch.equal(a, a0) and torch.equal(p, p0)


# ------------------------------------------------------------------ 2. mixed rows in one launch
@pytest.mark.parametrize('persistent, rows', LAYOUTS)
def test_mixed_rows_audio(pkg, tiny, monkeypatch, persistent, rows):
    monkeypatch.setenv('VQW_AR_PERSISTENT', persistent)
    if rows:
        monkeypatch.setenv('VQW_AR_ROWS', rows)
    model, P, w, enc, enc_ref = tiny
    n = 160                                                                # crosses two condition frames
    u = torch.rand(2, n, generator=torch.Generator().manual_seed(0))
    gen = pkg.generator.FastGenerator(model, batch=2)
    assert gen._parts == ([2] if rows else [1, 1])
    pa, pi = gen.generate(enc, n, mode='sample', uniforms=u.cuda())
    gen.reset()
    t, k, p = MIX
    ga, gi, probs = gen.generate(enc, n, mode='sample', uniforms=u.cuda(), return_probs=True,
                                 temperature=[1.0, t], top_k=[0, k], top_p=[1.0, p])
    gen.close()
    assert torch.equal(gi[0], pi[0]) and torch.equal(ga[0], pa[0])
    got, ga = gi.cpu().numpy(), ga.cpu().numpy()
    np.testing.assert_allclose(ga, M.R.mu_law_decode_np(got.astype(np.float32)), rtol=1e-5, atol=1e-6)
    g = M.FastGenerator(P, w, 2)
    a = np.zeros([2, 1], np.float32)
    for i in range(n):
        z = logits_of(g.step, torch.from_numpy(a), enc_ref[:, i // 64])
        pr, keep, q = check_row(z[1], int(got[1, i]), u[1, i].item(), t, k, p, 'step %d' % i)
        a = ga[:, i:i + 1]
    pl = probs[1].cpu().double().numpy()
    np.testing.assert_allclose(pl, q, rtol=2e-4, atol=1e-7)
    assert (pl[~keep] == 0).all() and keep.sum() <= k


# ------------------------------------------------------------------ 3. reductions
@pytest.mark.parametrize('persistent', ['1', '0'])
def test_reductions(pkg, tiny, monkeypatch, persistent):
    monkeypatch.setenv('VQW_AR_PERSISTENT', persistent)
    model, P, w, enc, enc_ref = tiny
    n = 128
    gen = pkg.generator.FastGenerator(model, batch=2)
    ga, gi = gen.generate(enc, n)
    u = torch.rand(2, n, generator=torch.Generator().manual_seed(9))
    u[0, :8] = torch.tensor([0.0, 1.0, 2.0, 1e-9, 0.999999, 0.5, 1.0, 2.0])
    for uu in (u, torch.full((2, n), 2.0)):
        gen.reset()
        sa, si = gen.generate(enc, n, mode='sample', uniforms=uu.cuda(), top_k=1)    # K = 1 is argmax whatever u
        assert torch.equal(si, gi) and torch.equal(sa, ga)
    # a low temperature follows argmax up to near-ties (q of a class d below the max is exp(-d / 0.05))
    gen.reset()
    u2 = torch.rand(2, n, generator=torch.Generator().manual_seed(10))
    ca, ci = gen.generate(enc, n, mode='sample', uniforms=u2.cuda(), temperature=0.05)
    got, ca = ci.cpu().numpy(), ca.cpu().numpy()
    g = M.FastGenerator(P, w, 2)
    a = np.zeros([2, 1], np.float32)
    for i in range(n):
        z = logits_of(g.step, torch.from_numpy(a), enc_ref[:, i // 64])
        for b in range(2):
            assert z[b].max() - z[b, got[b, i]] < 1.0, 'step %d row %d' % (i, b)
        a = ca[:, i:i + 1]
    # u = 1 and 2 with K = 3: the largest kept index (u = 1: unless the cdf already reaches 1 in fp32)
    for uval in (1.0, 2.0):
        gen.reset()
        ta, ti = gen.generate(enc, 64, mode='sample', uniforms=torch.full((2, 64), uval, device='cuda'), top_k=3)
        got, ta = ti.cpu().numpy(), ta.cpu().numpy()
        g = M.FastGenerator(P, w, 2)
        a = np.zeros([2, 1], np.float32)
        for i in range(64):
            z = logits_of(g.step, torch.from_numpy(a), enc_ref[:, i // 64])
            for b in range(2):
                pr, keep, q = check_row(z[b], int(got[b, i]), uval, 1.0, 3, 1.0, 'u %g step %d row %d' % (uval, i, b))
                if uval > 1.0:
                    assert got[b, i] == keep.nonzero()[0][-1]
            a = ta[:, i:i + 1]
    gen.close()


# ------------------------------------------------------------------ 4. the prior: defaults, mixed rows, reductions
def test_prior_sampling(pkg, monkeypatch):
    T = prior_tests()
    cfg = T.tiny_prior(k=32, pre_k=3)
    prior = pkg.prior.LatentPrior(cfg, 10, device='cuda', seed=0)
    P = T.random_params(prior, 11)
    prior.load_named(P)
    spk = torch.tensor([2, 9])
    sd = spk.cuda()
    cond = P['prior/speaker_embedding'][spk]
    n = 160
    u = torch.rand(2, n, generator=torch.Generator().manual_seed(0))
    for rows in (None, '2'):
        if rows:
            monkeypatch.setenv('VQW_AR_ROWS', rows)
        gen = pkg.generator.PriorGenerator(prior, batch=2)
        c0, p0 = gen.sample(n, sd, mode='sample', uniforms=u.cuda(), return_probs=True)
        gen.reset()
        idx, probs = gen._run(prior.speaker_condition(sd, 3), n, 'sample', u.cuda(), 64, None, True, [(1.0, 0, 1.0)] * 2)
        gen._t += n
        assert torch.equal(idx, c0) and torch.equal(probs, p0)
        gen.reset()
        t, k, p = MIX
        ci, pl = gen.sample(n, sd, mode='sample', uniforms=u.cuda(), return_probs=True,
                            temperature=[1.0, t], top_k=[0, k], top_p=[1.0, p])
        assert torch.equal(ci[0], c0[0])
        got = ci.cpu().numpy()
        g = T.RefPriorGen(P, cfg, 2)
        prev = [-1, -1]
        for i in range(n):
            z = logits_of(g.step, prev, cond)
            pr, keep, q = check_row(z[1], int(got[1, i]), u[1, i].item(), t, k, p, 'code step %d' % i)
            prev = list(got[:, i])
        pl = pl[1].cpu().double().numpy()
        np.testing.assert_allclose(pl, q, rtol=2e-4, atol=1e-7)
        assert (pl[~keep] == 0).all()
        # K = 1 is greedy; u = 2 with K = 3 is the largest kept code
        gen.reset()
        greedy = gen.sample(n, sd)
        gen.reset()
        assert torch.equal(gen.sample(n, sd, mode='sample', uniforms=torch.full((2, n), 2.0, device='cuda'), top_k=1), greedy)
        gen.reset()
        top = gen.sample(32, sd, mode='sample', uniforms=torch.full((2, 32), 2.0, device='cuda'), top_k=3).cpu().numpy()
        g = T.RefPriorGen(P, cfg, 2)
        prev = [-1, -1]
        for i in range(32):
            z = logits_of(g.step, prev, cond)
            for b in range(2):
                pr, keep, q = check_row(z[b], int(top[b, i]), 2.0, 1.0, 3, 1.0, 'code step %d row %d' % (i, b))
                assert top[b, i] == keep.nonzero()[0][-1]
            prev = list(top[:, i])
        gen.close()


# ------------------------------------------------------------------ 5. reference widths
@pytest.mark.parametrize('rows', [None, '2'])
def test_reference_width_audio(pkg, monkeypatch, rows):
    if rows:
        monkeypatch.setenv('VQW_AR_ROWS', rows)
    m, w = dict(M.DEFAULT_MODEL), dict(M.DEFAULT_WAVENET)
    model = pkg.model.VQVAE(m, w, 109, device='cuda', seed=0)
    n, ratio = 1200, 400
    enc = (torch.randn(2, model.Cc, 3, generator=torch.Generator().manual_seed(5)) * 0.5).cuda()
    u = torch.rand(2, n, generator=torch.Generator().manual_seed(6)).cuda()
    gen = pkg.generator.FastGenerator(model, batch=2)
    assert all(pkg._lib.lib().vqw_ar_decode_workgroups(h) > 0 for h in gen._hs)
    ga, gi = gen.generate(enc, n, ratio=ratio)
    gen.reset()
    ka, ki = gen.generate(enc, n, ratio=ratio, mode='sample', uniforms=u, top_k=1)
    assert torch.equal(ki, gi) and torch.equal(ka, ga)
    gen.reset()
    pa, pi, pp = gen.generate(enc, n, ratio=ratio, mode='sample', uniforms=u, return_probs=True)
    gen.reset()
    t, k, p = MIX
    ma, mi, mp = gen.generate(enc, n, ratio=ratio, mode='sample', uniforms=u, return_probs=True,
                              temperature=[1.0, t], top_k=[0, k], top_p=[1.0, p])
    gen.close()
    assert torch.equal(mi[0], pi[0]) and torch.equal(ma[0], pa[0]) and torch.equal(mp[0], pp[0])
    assert int(mi[1].min()) >= 0 and int(mi[1].max()) < 256
    assert int((mp[1] > 0).sum()) <= k and abs(float(mp[1].double().sum()) - 1.0) < 1e-5


def test_reference_width_prior(pkg):
    T = prior_tests()
    prior = pkg.prior.LatentPrior(T.default_prior(), 109, device='cuda', seed=0)
    k = prior.Q
    assert k == 512
    sd = torch.tensor([3, 77], device='cuda')
    n = 256
    u = torch.rand(2, n, generator=torch.Generator().manual_seed(7)).cuda()
    gen = pkg.generator.PriorGenerator(prior, batch=2)
    greedy = gen.sample(n, sd)
    gen.reset()
    assert torch.equal(gen.sample(n, sd, mode='sample', uniforms=u, top_k=1), greedy)
    gen.reset()
    plain, pp = gen.sample(n, sd, mode='sample', uniforms=u, return_probs=True)
    gen.reset()
    t, kk, p = MIX
    mixed, mp = gen.sample(n, sd, mode='sample', uniforms=u, return_probs=True, temperature=[1.0, t], top_k=[0, kk],
                           top_p=[1.0, p])
    gen.close()
    assert torch.equal(mixed[0], plain[0]) and torch.equal(mp[0], pp[0])
    assert int(mixed[1].min()) >= 0 and int(mixed[1].max()) < k and int((mp[1] > 0).sum()) <= kk


# ------------------------------------------------------------------ 6. errors
def test_generators_refuse_bad_settings(pkg, tiny):
    model, _, _, enc, _ = tiny
    gen = pkg.generator.FastGenerator(model, batch=2)
    u = torch.rand(2, 8, device='cuda')
    for kw in (dict(temperature=0.0), dict(temperature=float('inf')), dict(top_k=-1), dict(top_p=0.0), dict(top_p=1.01),
               dict(temperature=[0.5, 0.5, 0.5])):
        with pytest.raises(ValueError):
            gen.generate(enc, 8, mode='sample', uniforms=u, **kw)
    for kw in (dict(temperature=0.5), dict(top_k=3), dict(top_p=0.5)):
        with pytest.raises(ValueError, match='sample'):
            gen.generate(enc, 8, **kw)
    gen.close()
    T = prior_tests()
    prior = pkg.prior.LatentPrior(T.tiny_prior(k=32, pre_k=3), 10, device='cuda', seed=0)
    pg = pkg.generator.PriorGenerator(prior, batch=2)
    sd = torch.tensor([1, 2], device='cuda')
    with pytest.raises(ValueError):
        pg.sample(4, sd, mode='sample', top_p=2.0)
    with pytest.raises(ValueError, match='sample'):
        pg.sample(4, sd, top_k=5)
    pg.close()


# ------------------------------------------------------------------ 7. CLI
def test_cli_prior_generation_with_sampling_flags(tmp_path):
    T = prior_tests()
    w = {"verbose": False, "quantization_channels": 256, "num_cycles": 1, "num_cycle_layers": 4,
         "dilation_rates": [1, 2, 4, 8], "kernel_size": 3, "dilation_filters": 32, "skip_filters": 64,
         "residual_filters": 32, "preprocess": {"kernel_size": 32, "filters": 32}}
    m = {"encoder": "64", "use_vq": True, "speaker_embedding": 16, "k": 32, "latent_dim": 16, "beta": 0.25,
         "encoder_filters": 48, "wavenet_parameters": str(tmp_path / 'w.json'), "verbose": False,
         "learning_rate_schedule": {"0": 1e-3}}
    (tmp_path / 'w.json').write_text(json.dumps(w))
    (tmp_path / 'm.json').write_text(json.dumps(m))
    (tmp_path / 'p.json').write_text(json.dumps(T.tiny_prior(k=32, pre_k=2)))
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
    from scipy.io import wavfile
    results = []
    for _ in range(2):
        out = run([os.path.join(ROOT, 'generate.py'), '-restore', 'saved_model/weights-2.pt', '-prior', 'saved_prior/prior-2.pt',
                   '-frames', '24', '-speakers', 'p225', 'None', '-mode', 'sample', '-seed', '3', '-params', str(tmp_path / 'm.json'),
                   '-prior_params', str(tmp_path / 'p.json'), '-temperature', '0.8', '-top_k', '40', '-top_p', '0.95',
                   '-prior_temperature', '0.7', '-prior_top_k', '8', '-prior_top_p', '0.9'])
        assert out.returncode == 0, out.stderr[-2000:]
        res = []
        for s in ('p225', 'no_speaker'):
            sr, a = wavfile.read(str(tmp_path / 'saved_model' / ('2_%s_prior.wav' % s)))
            assert sr == 16000 and a.shape == (24 * 64,) and np.isfinite(a).all() and np.abs(a).max() <= 1.0
            c = np.load(str(tmp_path / 'saved_model' / ('prior_codes_2_%s.npy' % s)))
            assert c.shape == (24,) and c.min() >= 0 and c.max() < 32
            res.append((a, c))
        results.append(res)
    for (a1, c1), (a2, c2) in zip(*results):
        assert np.array_equal(a1, a2) and np.array_equal(c1, c2)
