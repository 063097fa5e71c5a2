"""GPU tests of teacher-forced reconstruction: the kernel (vqw_softmax_sample) against np.argmax and the float64 restatement
(recon_ref.py), its corner cases and reproducibility; VQVAE.reconstruct / LatentPrior.reconstruct against evaluate's hits,
their seeding and state preservation; and the command lines (generate.py -teacher_forced, train.py -audio_interval).

Bars: greedy idx, the values outside the range and audio are exact.  Sampled idx equals the restatement wherever
sampling_ref.fp32_edge does not flag the decision; at most 2 % of the positions may be flagged (the restatement alone flags
0 - 0.95 % on 3 randn logits for these settings at Q = 100, 256 and 512: measured on the CPU, 2000 positions per setting);
probs within 1e-6 of the restated q there, every row of probs sums to 1 within 1e-5.  Model level: the hits of a greedy
reconstruction are evaluate's hits, an integer compared exactly."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import ref_model as M

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import recon_ref as RR  # noqa: E402
from test_score_gpu import assert_unchanged, build_model, padded_batch, snapshot, tiny_cfg  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = [(1.0, 0, 1.0), (0.7, 0, 1.0), (1.0, 8, 1.0), (1.0, 0, 0.9), (1.3, 40, 0.8)]


def ranges_for(B, T):
    """Per row, in turn: t_begin > 0 with a ragged end, empty, first half, whole.  None is a multiple of 64."""
    pats = [(T // 3, T - 5), (10, 10), (0, T // 2 + 1), (0, T)]
    tb, te = zip(*[pats[b % 4] for b in range(B)])
    return np.array(tb, np.int32), np.array(te, np.int32)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def kw_of(settings):
    t, k, p = zip(*settings)
    return dict(temperature=list(t), top_k=list(k), top_p=list(p))


# ------------------------------------------------------------------ 1. greedy, exact
@pytest.mark.parametrize('with_ranges', [False, True])
@pytest.mark.parametrize('B, Q, T', [(3, 256, 200), (2, 4, 64), (2, 100, 70), (2, 1024, 130), (8, 256, 6656)])
def test_greedy_is_argmax(K, B, Q, T, with_ranges):
    g = np.random.RandomState(B + Q + T)
    z = (g.randn(B, Q, T) * 3).astype(np.float32)
    dup = [(b, int(t)) for b in range(B) for t in g.choice(T, 6, replace=False)]      # the maximum at two indices: the lower wins
    want_dup = []
    for b, t in dup:
        i, j = sorted(g.choice(Q, 2, replace=False).tolist())
        z[b, i, t] = z[b, j, t] = z[b, :, t].max() + 1
        want_dup.append(i)
    tb, te = ranges_for(B, T) if with_ranges else (None, None)
    mask = RR.range_mask(B, T, tb, te)
    want = np.where(mask, z.argmax(1), -1)
    assert [want[b, t] for b, t in dup] == [i if mask[b, t] else -1 for (b, t), i in zip(dup, want_dup)]
    zd, tbd, ted = dev(z), dev(tb), dev(te)
    # without probs: the argmax path; with probs: the transposing kernel
    audio = torch.full((B, T), float('nan'), device='cuda') if Q == 256 else None
    idx = K.softmax_sample(zd, mode='greedy', t_begin=tbd, t_end=ted, audio=audio)
    assert idx.dtype == torch.int32 and np.array_equal(idx.cpu().numpy(), want)
    probs = torch.full((B, T, Q), float('nan'), device='cuda')
    audio2 = torch.full((B, T), float('nan'), device='cuda') if Q == 256 else None
    idx2 = K.softmax_sample(zd, mode='greedy', t_begin=tbd, t_end=ted, audio=audio2, probs=probs)
    assert np.array_equal(idx2.cpu().numpy(), want)
    if Q == 256:
        dec = K.mu_law_decode_f32(idx.clamp(min=0).float())
        dec = torch.where(idx >= 0, dec, torch.zeros_like(dec))
        for a in (audio, audio2):
            assert torch.equal(a.view(torch.int32), dec.view(torch.int32))
            assert (a[idx < 0] == 0).all()
    assert (probs[idx2 < 0] == 0).all()
    inside = probs[idx2 >= 0]
    assert ((inside.sum(-1) - 1).abs() <= 1e-5).all()
    if B * Q * T <= 1 << 20:                                  # softmax(z) in float64
        ref = RR.sample_ref(z, None, None, tb, te, mode='greedy')
        assert np.abs(probs.cpu().double().numpy() - ref['probs']).max() <= 1e-6


# ------------------------------------------------------------------ 2. sample against float64
@pytest.mark.parametrize('B, Q, T', [(3, 256, 1500), (2, 512, 700), (2, 100, 700)])
def test_sample_against_float64(K, B, Q, T):
    g = np.random.RandomState(Q + T)
    z = (g.randn(B, Q, T) * 3).astype(np.float32)
    u = g.rand(B, T).astype(np.float32)
    zd, ud = dev(z), dev(u)
    flagged = total = 0
    for launch in range(-(-len(SETTINGS) // B)):              # every setting sits in a launch next to other settings
        settings = [SETTINGS[(launch * B + b) % len(SETTINGS)] for b in range(B)]
        ref = RR.sample_ref(z, u, settings)
        probs = torch.full((B, T, Q), float('nan'), device='cuda')
        audio = torch.full((B, T), float('nan'), device='cuda') if Q == 256 else None
        idx = K.softmax_sample(zd, mode='sample', uniforms=ud, audio=audio, probs=probs, **kw_of(settings))
        got, pr = idx.cpu().numpy(), probs.cpu().double().numpy()
        ok = ~ref['edge']
        flagged += int(ref['edge'].sum())
        total += B * T
        print('Q %d launch %d %s: flagged %d of %d, idx differs at %d flagged positions, probs error %.3g'
              % (Q, launch, settings, ref['edge'].sum(), B * T, (got != ref['idx'])[~ok].sum(), np.abs(pr - ref['probs'])[ok].max()))
        assert ((got >= 0) & (got < Q)).all()
        assert np.array_equal(got[ok], ref['idx'][ok])
        assert np.abs(pr - ref['probs'])[ok].max() <= 1e-6
        assert np.abs(pr.sum(-1) - 1).max() <= 1e-5
        if Q == 256:
            assert torch.equal(audio.view(torch.int32), K.mu_law_decode_f32(idx.float()).view(torch.int32))
    assert flagged <= 0.02 * total


# ------------------------------------------------------------------ 3. exact corner cases
def test_corner_cases(K):
    B, Q, T = 3, 256, 150
    g = np.random.RandomState(11)
    z = (g.randn(B, Q, T) * 3).astype(np.float32)
    zd = dev(z)
    greedy = K.softmax_sample(zd, mode='greedy')
    for u in (0.0, 0.37, 1.0):                                # top_k = 1: the greedy class whatever u
        ud = torch.full((B, T), u, device='cuda')
        assert torch.equal(K.softmax_sample(zd, uniforms=ud, top_k=1), greedy)
    ud = dev(g.rand(B, T).astype(np.float32))
    assert torch.equal(K.softmax_sample(zd, uniforms=ud, top_k=1, temperature=[0.5, 1.0, 2.0], top_p=[1.0, 0.5, 0.1]), greedy)
    # u = 0 on default rows: index 0 (its cdf value is >= 0)
    zero = torch.zeros(B, T, device='cuda')
    assert (K.softmax_sample(zd, uniforms=zero) == 0).all()
    # u = 1: the largest kept index.  Truncated rows on the wide logits (the kept classes are few and heavy); default rows
    # on narrow logits, where the last class (index Q - 1) is far heavier than the cdf's rounding
    one = torch.ones(B, T, device='cuda')
    settings = [(1.0, 8, 1.0), (1.0, 0, 0.9), (1.3, 40, 0.8)]
    ref = RR.sample_ref(z, np.ones((B, T), np.float32), settings)
    got = K.softmax_sample(zd, uniforms=one, **kw_of(settings)).cpu().numpy()
    ok = ~RR.sample_ref(z, np.full((B, T), -1.0), settings)['edge']      # (u far from every cdf value: the truncations' edges alone)
    assert ok.mean() > 0.98 and np.array_equal(got[ok], ref['last'][ok])
    narrow = dev((g.randn(B, Q, T) * 0.5).astype(np.float32))
    assert (K.softmax_sample(narrow, uniforms=one) == Q - 1).all()


# ------------------------------------------------------------------ 4. reproducibility
@pytest.mark.parametrize('mode', ['sample', 'greedy'])
def test_reproducible_and_row_independent(K, mode):
    B, Q, T = 3, 256, 333
    g = np.random.RandomState(5)
    zd, ud = dev((g.randn(B, Q, T) * 3).astype(np.float32)), dev(g.rand(B, T).astype(np.float32))
    tb, te = (dev(a) for a in ranges_for(B, T))
    te[1] = T - 7                                             # (row 1 of the pattern is empty: give it a range)
    tb[1] = 3
    settings = [(1.0, 0, 1.0), (0.7, 8, 1.0), (1.3, 40, 0.8)]

    def run(z, u, s, b0, b1):
        probs, audio = torch.empty(b1 - b0, T, Q, device='cuda'), torch.empty(b1 - b0, T, device='cuda')
        kw = kw_of(s) if mode == 'sample' else {}
        idx = K.softmax_sample(z, mode=mode, uniforms=u if mode == 'sample' else None, t_begin=tb[b0:b1].contiguous(),
                               t_end=te[b0:b1].contiguous(), audio=audio, probs=probs, **kw)
        return idx, audio.view(torch.int32), probs.view(torch.int32)
    first = run(zd, ud, settings, 0, B)
    for a, b in zip(first, run(zd, ud, settings, 0, B)):
        assert torch.equal(a, b)
    for b in range(B):
        alone = run(zd[b:b + 1].contiguous(), ud[b:b + 1].contiguous(), settings[b:b + 1], b, b + 1)
        for a, c in zip(first, alone):
            assert torch.equal(a[b:b + 1], c), b


# ------------------------------------------------------------------ 5. tiny VQ-VAE
def test_reconstruct_tiny_vqvae(pkg):
    K = pkg.kernels
    m, w = tiny_cfg()
    model, _, _ = build_model(pkg, m, w, 10, seed=3)
    lengths = [512, 320, 128]
    x, spk = padded_batch(3, 512, 10, lengths, seed=21)
    xd, sd = x[:, :, 0].contiguous().cuda(), spk.cuda()
    model.train_step(xd, sd)
    model.train_step(xd, sd)
    snap = snapshot(model)
    rng = torch.cuda.get_rng_state()
    labels = K.mu_law_encode_i32(xd)
    scored = torch.arange(512, device='cuda')[None, :] < torch.tensor(lengths, device='cuda')[:, None]
    by_weights = {}
    for weights in ('ema', 'live'):
        audio, idx, probs = model.reconstruct(xd, sd, lengths=lengths, weights=weights, mode='greedy', return_probs=True)
        assert audio.shape == (3, 512) and idx.shape == (3, 512) and idx.dtype == torch.int32 and probs.shape == (3, 512, 256)
        assert_unchanged(model, snap)
        assert (idx[~scored] == -1).all() and (audio[~scored] == 0).all() and (probs[~scored] == 0).all()
        assert ((idx[scored] >= 0) & (idx[scored] < 256)).all()
        hits = ((idx == labels) & scored).sum(1).cpu().tolist()
        want = model.evaluate(xd, sd, lengths=lengths, weights=weights).hits.tolist()
        print('%s weights: greedy hits %s, evaluate hits %s' % (weights, hits, want))
        assert hits == want                                   # idx[b][t] predicts sample t: the labels evaluate scores
        assert torch.equal(audio.view(torch.int32), torch.where(scored, K.mu_law_decode_f32(idx.clamp(min=0).float()),
                                                                torch.zeros_like(audio)).view(torch.int32))
        by_weights[weights] = idx
    assert not torch.equal(by_weights['ema'], by_weights['live'])
    # sampling: the same seed gives the same audio, another seed another; the global RNG is never touched.  Two passes do not
    # make the same logits bit for bit (the encoder's short layers add their split-K slices with fp32 atomics: 1e-6 of
    # difference, measured), so a draw whose uniform lies that close to a cdf value can differ between two calls.  Seed 6
    # is one at which no uniform does: the nearest cdf value is 1.1e-5 away (measured on MI355X over seeds 0 .. 11: 6.5e-9
    # at seed 4, which flipped one draw in 2 of 40 calls, 5e-7 .. 5e-6 at the others)
    a0, i0 = model.reconstruct(xd, sd, lengths=lengths, seed=6)
    a1, i1 = model.reconstruct(xd, sd, lengths=lengths, seed=6)
    a2, _ = model.reconstruct(xd, sd, lengths=lengths, seed=2)
    print('seed 6 twice: idx differs at %s; seed 2: audio differs from seed 6 at %d positions'
          % ((i0 != i1).nonzero().tolist(), int((a0 != a2).sum())))
    assert torch.equal(a0.view(torch.int32), a1.view(torch.int32)) and torch.equal(i0, i1) and not torch.equal(a0, a2)
    # given uniforms are used as they are: top_k = 1 is the greedy reconstruction
    u = torch.rand(3, 512, generator=torch.Generator().manual_seed(1)).cuda()
    _, ik = model.reconstruct(xd, sd, lengths=lengths, uniforms=u, top_k=1)
    assert torch.equal(ik, by_weights['ema'])
    assert torch.equal(torch.cuda.get_rng_state(), rng)
    assert_unchanged(model, snap)
    for bad, match in (([512, 100, 64], 'lengths'), ([576, 64, 64], 'lengths'), ([512, 64], 'lengths')):
        with pytest.raises(ValueError, match=match):
            model.reconstruct(xd, sd, lengths=bad)
        assert_unchanged(model, snap)
    with pytest.raises(ValueError, match='weights'):
        model.reconstruct(xd, sd, weights='best')
    with pytest.raises(ValueError, match='sample'):
        model.reconstruct(xd, sd, mode='greedy', top_k=3)
    with pytest.raises(ValueError, match='mode'):
        model.reconstruct(xd, sd, mode='beam')
    assert_unchanged(model, snap)


# ------------------------------------------------------------------ 6. tiny prior
def test_reconstruct_tiny_prior(pkg):
    from test_prior_gpu import random_params, tiny_prior
    cfg = tiny_prior()
    prior = pkg.prior.LatentPrior(cfg, 10, device='cuda', seed=0)
    prior.load_named(random_params(prior, 2))
    prior.load_named(random_params(prior, 1), also_ema=False)
    g = torch.Generator().manual_seed(4)
    codes = torch.randint(0, cfg['quantization_channels'], (3, 128), generator=g).int().cuda()
    spk = torch.randint(0, 10, (3,), generator=g).cuda()
    lengths = [128, 100, 7]
    scored = torch.arange(128, device='cuda')[None, :] < torch.tensor(lengths, device='cuda')[:, None]
    for weights in ('ema', 'live'):
        idx, probs = prior.reconstruct(codes, spk, lengths=lengths, weights=weights, mode='greedy', return_probs=True)
        assert idx.shape == (3, 128) and probs.shape == (3, 128, cfg['quantization_channels'])
        assert (idx[~scored] == -1).all() and (probs[~scored] == 0).all()
        hits = ((idx == codes) & scored).sum(1).cpu().tolist()
        assert hits == prior.evaluate(codes, spk, lengths=lengths, weights=weights).hits.tolist()
    idx = prior.reconstruct(codes, spk, lengths=lengths, seed=2, temperature=0.8, top_k=5)
    assert torch.is_tensor(idx) and torch.equal(idx, prior.reconstruct(codes, spk, lengths=lengths, seed=2, temperature=0.8, top_k=5))
    with pytest.raises(ValueError, match='lengths'):
        prior.reconstruct(codes, spk, lengths=[128, 0, 7])


# ------------------------------------------------------------------ 7. command lines
def test_cli_teacher_forced_and_train_audio(pkg, tmp_path):
    from scipy.io import wavfile
    from test_score_cpu import write_dataset
    w = {"verbose": False, "quantization_channels": 256, "num_cycles": 1, "num_cycle_layers": 4,
         "dilation_rates": [1, 2, 4, 8], "kernel_size": 3, "dilation_filters": 32, "skip_filters": 64,
         "residual_filters": 32, "preprocess": {"kernel_size": 32, "filters": 32}}
    m = {"encoder": "64", "use_vq": True, "speaker_embedding": 16, "k": 32, "latent_dim": 16, "beta": 0.25,
         "encoder_filters": 48, "wavenet_parameters": str(tmp_path / 'w.json'), "verbose": False,
         "learning_rate_schedule": {"0": 1e-3}}
    (tmp_path / 'w.json').write_text(json.dumps(w))
    (tmp_path / 'm.json').write_text(json.dumps(m))
    root = str(tmp_path / 'data')
    rels = write_dataset(root, [1000, 700, 1500], speakers=['p%d' % (225 + i) for i in range(109)])
    (tmp_path / 'held.txt').write_text('\n'.join(rels) + '\n')
    env = dict(os.environ, PYTHONPATH=ROOT)
    cwd = str(tmp_path)
    train = [sys.executable, os.path.join(ROOT, 'train.py'), '-dataset', 'synthetic', '-length', '512', '-batch', '2', '-step', '4',
             '-interval', '4', '-params', str(tmp_path / 'm.json'), '-eval_list', str(tmp_path / 'held.txt'), '-eval_interval', '4',
             '-eval_batches', '1', '-data_root', root]
    out = subprocess.run(train + ['-save', 'plain/weights'], cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert '[audio' not in out.stdout and not (tmp_path / 'plain' / 'audio').exists()
    assert not [f for f in os.listdir(str(tmp_path / 'plain')) if f.endswith('.wav')]
    out = subprocess.run(train + ['-save', 'saved_model/weights', '-audio_interval', '2'], cwd=cwd, env=env, capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.count('[audio 2]') == 2
    adir = tmp_path / 'saved_model' / 'audio'
    assert sorted(os.listdir(str(adir))) == sorted(['0_original.wav', '1_original.wav', '2_0_teacher.wav', '2_1_teacher.wav',
                                                    '4_0_teacher.wav', '4_1_teacher.wav'])
    for f in os.listdir(str(adir)):
        sr, a = wavfile.read(str(adir / f))
        assert sr == 16000 and a.dtype == np.float32 and a.shape == (512,) and np.abs(a).max() <= 1.0
    lines = [json.loads(ln) for ln in (tmp_path / 'saved_model' / 'summaries.jsonl').read_text().splitlines()]
    assert [ln['global_step'] for ln in lines] == [2, 4]
    # generate.py -teacher_forced: one wav of the utterance's (trimmed) length per speaker
    ckpt = tmp_path / 'saved_model' / 'weights-4.pt'
    t = np.arange(1100) / 16000.0
    wavfile.write(str(tmp_path / 'a.wav'), 16000, (np.sin(2 * np.pi * 220 * t) * 8000).astype(np.int16))
    gen = [sys.executable, os.path.join(ROOT, 'generate.py'), '-restore', str(ckpt), '-audio', str(tmp_path / 'a.wav'), '-speakers',
           'p226', 'None', '-params', str(tmp_path / 'm.json'), '-teacher_forced']
    got = {}
    for flags in (['-mode', 'greedy'], ['-seed', '3', '-temperature', '0.8', '-top_k', '20']):
        out = subprocess.run(gen + flags, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        for s in ('p226', 'no_speaker'):
            sr, a = wavfile.read(str(tmp_path / 'saved_model' / ('4_%s_teacher.wav' % s)))
            assert sr == 16000 and a.dtype == np.float32 and a.shape == (1100 // 64 * 64,)
            got.setdefault(s, []).append(a)
    for s, (greedy, sampled) in got.items():
        assert not np.array_equal(greedy, sampled)
    assert not np.array_equal(got['p226'][0], got['no_speaker'][0])
