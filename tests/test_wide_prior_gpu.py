"""GPU tests of the wide generator's code-input mode (generator.WidePriorGenerator, vqw_ar_wide_prior_create,
arw_pre_code_kernel and the code-mode sampling kernel of csrc/ar_wide.hip) against the float64 PARALLEL reference
gen_ref.prior_probs64: the training graph teacher-forced on the codes the generator produced, nothing in common with ring or
window logic.

The contract, as test_wide_gen_gpu.py pins it for the audio mode:
  (a) every code is min(searchsorted(cumsum(p64), u), k-1), excused only where u lies within gen_ref.EDGE of a cdf value, at
      most 0.2 % of the steps; probs_last at a chunk end is p64 within rtol 2e-4, atol 1e-7;
  (b) a row's codes and probs_last are bit for bit independent of the batch;
  (c) a run cut into chunks equals the single run bit for bit;
  (d) greedy is the reference's argmax unless the top two reference probabilities are within 2e-6 (test_prefill_gpu.py);
  (e) a truncated row follows tests/sampling_ref.py on the reference's logits at the bars of test_sampling_gpu.py, and a
      default row beside truncated rows keeps the bits of an all-default launch.

Tiny prior: test_prior_gpu.tiny_prior(k=32, pre_k=3): R 32, S 64, 32 codes, dilations [1,2,4,8] * 2 (deepest ring 16 slots),
the speaker (16 values) the only condition, 64 code steps per condition frame.  B = 70 is three column tiles of 32 with a
partial last one and two input-stage blocks of 64 rows with a partial second one; n = 320 is five condition frames (one
refresh of the 4-frame window at step 256) and twenty wraps of the deepest ring.  Every row has u = nextafter(1, 0) planted
at step 0 and at seven other steps: the fp32 cdf may end below it, which gives index k, clamped to k - 1; steps 0..2 have
an empty or partly empty history ("no code" is a zero one-hot, not code 0)."""
import ctypes
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_ref as G  # noqa: E402
import sampling_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = G.prior_tests()
K, N, B70 = 32, 320, 70
DIL = [1, 2, 4, 8] * 2
DEPTHS = G.ring_depths(3, DIL, persistent=False)
MAX_EXCUSED = 0.002           # of B * n
PARAM_SEED = 21               # of random_params
SEED = 2                      # of the B = 70 run's uniforms.  Checked on the CPU before it was committed: test_prior_gpu.py's
#                               RefPriorGen (the oracle's own fp32 stepping sampler) run on these parameters, speakers and
#                               uniforms needs no cdf-edge excuse against prior_probs64 of its own codes, and every row of its
#                               run shows at least 16 distinct codes (asserted below for the GPU run)
TOP = float(np.nextafter(np.float32(1), np.float32(0)))


def uniforms(B, n, seed, plant=True):
    """[B][n] uniforms; planted: u = nextafter(1, 0) at step 0 and at seven other steps of every row."""
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(B, n, generator=g)
    if plant:
        for b in range(B):
            u[b, 0] = TOP
            u[b, torch.randperm(n - 1, generator=g)[:7] + 1] = TOP
    return u


def speakers(B, shift=0):
    return torch.tensor([(i + shift) % 10 for i in range(B)], dtype=torch.int64)


@pytest.fixture(scope='module')
def priors(pkg):
    made = {}

    def get(pre_k):
        if pre_k not in made:
            cfg = T.tiny_prior(k=K, pre_k=pre_k)
            prior = pkg.prior.LatentPrior(cfg, 10, device='cuda', seed=0)
            P = T.random_params(prior, PARAM_SEED)
            prior.load_named(P)
            made[pre_k] = (prior, P, cfg)
        return made[pre_k]
    yield get
    made.clear()
    torch.cuda.empty_cache()


def check_a(P, cfg, spk, u, idx, probs, rows=None):
    """(a) of one run from reset (of `rows` only, when given); returns p64."""
    idx_h = idx.cpu().numpy()
    k = cfg['quantization_channels']
    assert idx_h.dtype == np.int32 and idx_h.min() >= 0 and idx_h.max() < k, 'codes outside [0, %d)' % k
    sel = slice(None) if rows is None else rows
    p64 = G.prior_probs64(P, cfg, idx_h[sel], spk[sel])
    B, n = idx_h[sel].shape
    excused = G.check_sampled(p64, u[sel], idx_h[sel], DEPTHS)
    print('\n[wide prior] B=%d n=%d: excused %d of %d' % (B, n, excused, B * n))
    assert excused <= MAX_EXCUSED * B * n, '%d of %d steps needed the cdf-edge excuse' % (excused, B * n)
    np.testing.assert_allclose(probs.cpu().numpy()[sel], p64[:, -1], rtol=2e-4, atol=1e-7, err_msg='distribution of the last step')
    return p64


@pytest.fixture(scope='module')
def run70(pkg, priors):
    """The B = 70 run every tiny test compares against: one sample() call from reset, and its float64 reference."""
    prior, P, cfg = priors(3)
    spk, u = speakers(B70), uniforms(B70, N, SEED)
    gen = pkg.generator.WidePriorGenerator(prior, batch=B70)
    idx, probs = gen.sample(N, spk.cuda(), mode='sample', uniforms=u.cuda(), return_probs=True)
    p64 = check_a(P, cfg, spk, u, idx, probs)
    yield dict(prior=prior, P=P, cfg=cfg, spk=spk, u=u, gen=gen, idx=idx, probs=probs, p64=p64)
    gen.close()


# ------------------------------------------------------------------ 1. distribution
def test_b70_distribution_is_the_training_graphs(run70):
    """(a): asserted when the fixture is made.  Here: the planted uniforms gave the last code, the history is varied."""
    idx = run70['idx'].cpu().numpy()
    planted = run70['u'].numpy() == np.float32(TOP)
    assert (planted.sum(1) == 8).all() and planted[:, 0].all()
    cdf_before_last = np.cumsum(run70['p64'], -1)[:, :, K - 2]
    sure = planted & (cdf_before_last < TOP - G.EDGE)
    assert sure.any()
    assert (idx[sure] == K - 1).all(), 'u = nextafter(1, 0) did not give the last code'
    distinct = [len(np.unique(r)) for r in idx]
    assert min(distinct) >= 16, 'degenerate history: %s distinct codes per row' % distinct


# ------------------------------------------------------------------ 2. chunking
def test_chunked_run_equals_single_run(run70):
    """(c): chunk ends around the steps where taps go live and the deepest ring wraps, one inside a condition frame (100),
    256 and 257 on either side of the refresh of the condition window."""
    r = run70
    gen, sd, u_d = r['gen'], r['spk'].cuda(), r['u'].cuda()
    ends = sorted(set(G.checkpoints(N, 3, 8)) | {100, 256, 257})
    assert ends[-1] == N
    gen.reset()
    ia, prev = [], 0
    for t in ends:
        i_c, p_c = gen.sample(t - prev, sd, mode='sample', uniforms=u_d[:, prev:t].contiguous(), return_probs=True)
        ia.append(i_c)
        np.testing.assert_allclose(p_c.cpu().numpy(), r['p64'][:, t - 1], rtol=2e-4, atol=1e-7, err_msg='distribution of step %d' % (t - 1))
        prev = t
    assert torch.equal(torch.cat(ia, 1), r['idx'])
    assert torch.equal(p_c, r['probs'])


# ------------------------------------------------------------------ 3. batch independence
def test_rows_do_not_depend_on_the_batch(pkg, run70):
    """(b): rows 0..4 as a B = 5 generator, and as rows 65..69 of another B = 70 batch whose other rows have other speakers,
    uniforms and truncation settings."""
    r = run70
    want = (r['idx'][:5], r['probs'][:5])
    g5 = pkg.generator.WidePriorGenerator(r['prior'], batch=5)
    i, p = g5.sample(N, r['spk'][:5].cuda(), mode='sample', uniforms=r['u'][:5].contiguous().cuda(), return_probs=True)
    g5.close()
    assert torch.equal(i, want[0]) and torch.equal(p, want[1])
    spk2, u2 = speakers(B70, shift=3), uniforms(B70, N, SEED + 1)
    spk2[65:], u2[65:] = r['spk'][:5], r['u'][:5]
    sets = [(0.8, 20, 0.9), (1.3, 0, 0.5), (1.0, 0, 1.0)]
    rows = [sets[b % 3] if b < 65 else (1.0, 0, 1.0) for b in range(B70)]
    gen = r['gen']
    gen.reset()
    i, p = gen.sample(N, spk2.cuda(), mode='sample', uniforms=u2.cuda(), return_probs=True, temperature=[s[0] for s in rows],
                      top_k=[s[1] for s in rows], top_p=[s[2] for s in rows])
    assert not torch.equal(i[:5], want[0])
    assert torch.equal(i[65:], want[0]) and torch.equal(p[65:], want[1])


# ------------------------------------------------------------------ 4. pre_k = 1
def test_pre_k_one(pkg, priors):
    """The default prior's preprocess: one tap, the code of the previous step alone; B = 33, n = 128."""
    prior, P, cfg = priors(1)
    spk, u = speakers(33), uniforms(33, 128, 5)
    gen = pkg.generator.WidePriorGenerator(prior, batch=33)
    idx, probs = gen.sample(128, spk.cuda(), mode='sample', uniforms=u.cuda(), return_probs=True)
    gen.close()
    check_a(P, cfg, spk, u, idx, probs)


# ------------------------------------------------------------------ 5. truncated rows
def test_truncated_rows(pkg, priors):
    """(e): B = 12, rows alternating default / (0.8, 10, 0.9) / (1.3, 0, 0.5); n = 128."""
    prior, P, cfg = priors(3)
    B, n = 12, 128
    sets = [(1.0, 0, 1.0), (0.8, 10, 0.9), (1.3, 0, 0.5)]
    spk, u = speakers(B), uniforms(B, n, 8, plant=False)
    gen = pkg.generator.WidePriorGenerator(prior, batch=B)
    pi, pp = gen.sample(n, spk.cuda(), mode='sample', uniforms=u.cuda(), return_probs=True)
    gen.reset()
    ti, tp = gen.sample(n, spk.cuda(), mode='sample', uniforms=u.cuda(), return_probs=True,
                        temperature=[sets[b % 3][0] for b in range(B)], top_k=[sets[b % 3][1] for b in range(B)],
                        top_p=[sets[b % 3][2] for b in range(B)])
    gen.close()
    d = list(range(0, B, 3))
    assert torch.equal(ti[d], pi[d]) and torch.equal(tp[d], pp[d])
    got = ti.cpu().numpy()
    assert got.min() >= 0 and got.max() < K
    p64 = G.prior_probs64(P, cfg, got, spk)
    z = np.log(np.maximum(p64, 1e-300))                  # the reference's logits up to a constant per step
    un = u.double().numpy()
    for b in range(B):
        t, k, p = sets[b % 3]
        if b % 3 == 0:
            continue
        for i in range(n):
            pr, keep, q, want = S.restate(z[b, i], t, k, p, un[b, i])
            if got[b, i] != want or not keep[got[b, i]]:
                assert S.fp32_edge(pr, keep, q, k, p, un[b, i]), 'row %d step %d: GPU %d, restated %d' % (b, i, got[b, i], want)
        pl = tp[b].cpu().double().numpy()
        np.testing.assert_allclose(pl, q, rtol=2e-4, atol=1e-7)
        assert (pl[~keep] == 0).all()
        if k:
            assert keep.sum() <= k


# ------------------------------------------------------------------ 6. greedy
def test_greedy_is_the_references_argmax(pkg, priors):
    prior, P, cfg = priors(3)
    B, n = 6, 128
    spk = speakers(B, shift=4)
    gen = pkg.generator.WidePriorGenerator(prior, batch=B)
    idx, probs = gen.sample(n, spk.cuda(), return_probs=True)
    gen.close()
    got = idx.cpu().numpy().astype(np.int64)
    assert got.min() >= 0 and got.max() < K
    p64 = G.prior_probs64(P, cfg, got, spk)
    gap = p64.max(-1) - np.take_along_axis(p64, got[:, :, None], -1)[:, :, 0]
    assert (gap <= 2e-6).all(), 'greedy is not argmax(p64) at (row, step) %s' % (np.argwhere(gap > 2e-6)[:4],)
    np.testing.assert_allclose(probs.cpu().numpy(), p64[:, -1], rtol=2e-4, atol=1e-7)


# ------------------------------------------------------------------ 7. the default widths, once
def test_default_widths(pkg):
    """prior_parameters.json (R 256, S 512, 512 codes, 20 layers, pre_k 1), B = 33, n = 1088: seventeen condition frames, past
    the wrap of the 1024-slot rings, four refreshes of the condition window.  The float64 reference is computed for rows 0
    and 32 only (row 32 sits alone in the partial column tile); every row's codes lie in [0, 512)."""
    cfg = T.default_prior()
    prior = pkg.prior.LatentPrior(cfg, 10, device='cuda', seed=0)
    P = T.random_params(prior, PARAM_SEED + 1)
    prior.load_named(P)
    B, n = 33, 1088
    spk, u = speakers(B), uniforms(B, n, 9)
    gen = pkg.generator.WidePriorGenerator(prior, batch=B)
    idx, probs = gen.sample(n, spk.cuda(), mode='sample', uniforms=u.cuda(), return_probs=True)
    gen.close()
    assert int(idx.min()) >= 0 and int(idx.max()) < 512
    check_a(P, cfg, spk, u, idx, probs, rows=[0, 32])


# ------------------------------------------------------------------ 8. lifecycle and refusals
def test_lifecycle_and_refusals(pkg, run70):
    r = run70
    prior, gen = r['prior'], r['gen']
    L = pkg._lib
    lib = L.lib()
    sd, u_d = r['spk'].cuda(), r['u'].cuda()
    cond = prior.speaker_condition(sd, 1)
    idx = torch.empty(B70, 8, dtype=torch.int32, device='cuda')
    audio = torch.empty(B70, 8, device='cuda')
    gen.reset()
    assert lib.vqw_ar_wide_run_async(gen._h, L.ptr(cond), 1, 64, 8, 0, None, None, L.ptr(audio), L.ptr(idx), None, L.stream()) != 0
    assert 'audio must be NULL on a code handle' in lib.vqw_last_error().decode()
    assert lib.vqw_ar_wide_run_async(gen._h, L.ptr(cond), 1, 64, 8, 0, None, None, None, None, None, L.stream()) != 0
    assert 'indices is NULL' in lib.vqw_last_error().decode()
    for q, n_codes, match in ((K, 64, 'n_codes=64 must equal w->Q=32'), (48, 48, 'n_codes=48')):
        keep = []
        wts = pkg.generator._weights_of(prior, keep)
        wts.Q = q
        h = ctypes.c_void_p()
        assert lib.vqw_ar_wide_prior_create(ctypes.byref(h), ctypes.byref(wts), 4, n_codes) != 0
        assert match in lib.vqw_last_error().decode(), lib.vqw_last_error()
        assert h.value is None
    # the refused calls left the handle as reset left it; a run, then reset, then the B = 70 run again
    gen.sample(40, sd, mode='sample', uniforms=u_d[:, :40].contiguous())
    gen.reset()
    i1, p1 = gen.sample(N, sd, mode='sample', uniforms=u_d, return_probs=True)
    assert torch.equal(i1, r['idx']) and torch.equal(p1, r['probs'])
    other = pkg.generator.WidePriorGenerator(prior, batch=3)
    other.close()
    other.close()


# ------------------------------------------------------------------ 9. command line
def test_cli_prior_corpus(pkg, tmp_path):
    """generate.py -prior -count 3 with two speakers: six wavs and six code files; -rows 2 writes the same bytes as -rows 4;
    each row's wav is what WideGenerator decodes from that row's code file with the row's audio uniforms."""
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
               '-length', '128', '-batch', '2', '-step', '4', '-interval', '2', '-save', 'saved_prior/prior',
               '-params', str(tmp_path / 'p.json'), '-vqvae_params', str(tmp_path / 'm.json')])
    assert out.returncode == 0, out.stderr[-2000:]
    (tmp_path / 'data').mkdir()
    (tmp_path / 'data' / 'vctk_speakers.txt').write_text('p225, 3\np226, 5\n')
    names = ['2_%s_prior_%d.wav' % (s, j) for s in ('p225', 'p226') for j in range(3)] + \
            ['prior_codes_2_%s_%d.npy' % (s, j) for s in ('p225', 'p226') for j in range(3)]
    saved = tmp_path / 'saved_model'
    files = {}
    for rows in (4, 2):
        out = run([os.path.join(ROOT, 'generate.py'), '-restore', 'saved_model/weights-2.pt', '-prior', 'saved_prior/prior-4.pt',
                   '-frames', '8', '-speakers', 'p225', 'p226', '-count', '3', '-rows', str(rows), '-mode', 'sample', '-seed', '1',
                   '-params', str(tmp_path / 'm.json'), '-prior_params', str(tmp_path / 'p.json')])
        assert out.returncode == 0, out.stderr[-2000:]
        files[rows] = {}
        for name in names:
            assert (saved / name).exists(), '%s was not written (-rows %d)' % (name, rows)
            files[rows][name] = (saved / name).read_bytes()
            (saved / name).unlink()
        assert not [f for f in os.listdir(str(saved)) if '_prior' in f or f.startswith('prior_codes')], 'unexpected outputs'
    assert files[4] == files[2], 'a row\'s bytes depend on -rows'
    # each row's wav from its code file
    import io
    from scipy.io import wavfile
    spec = importlib.util.spec_from_file_location('generate_cli', os.path.join(ROOT, 'generate.py'))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    parameters, wavenet_parameters = pkg.model.load_configs(str(tmp_path / 'm.json'))
    model = pkg.model.VQVAE(parameters, wavenet_parameters, 109, device='cuda', seed=0)
    model.load_state_dict(torch.load(str(saved / 'weights-2.pt'), map_location='cpu', weights_only=True))
    model.use_ema_weights()
    gen = pkg.generator.WideGenerator(model, batch=1)
    for k, (s, sid) in enumerate((('p225', 3), ('p226', 5))):
        for j in range(3):
            i = k * 3 + j
            codes = np.load(io.BytesIO(files[4]['prior_codes_2_%s_%d.npy' % (s, j)]))
            assert codes.shape == (8,) and codes.dtype == np.int32 and codes.min() >= 0 and codes.max() < 32
            sr, a = wavfile.read(io.BytesIO(files[4]['2_%s_prior_%d.wav' % (s, j)]))
            assert sr == 16000 and a.shape == (512,) and a.dtype == np.float32
            spk = torch.tensor([sid], dtype=torch.int64, device='cuda')
            cond = model.condition_from_codes(torch.from_numpy(codes).cuda().unsqueeze(0).contiguous(), spk)
            gen.reset()
            audio, _ = gen.generate(cond, 512, mode='sample', ratio=64, uniforms=cli.row_uniforms(1, i, 512, stage=1).unsqueeze(0).cuda())
            assert np.array_equal(audio[0].cpu().numpy(), a), 'row %d: the wav is not the decode of its code file' % i
    gen.close()
