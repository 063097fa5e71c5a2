"""GPU tests of held-out scoring: the two kernels (vqw_softmax_score, vqw_code_histogram) against the float64 restatement
(score_ref.py), VQVAE.evaluate / LatentPrior.evaluate against the oracle on padded batches, state preservation, the score
workspace, and the command lines (evaluate.py, train.py -eval_list).

Bars: hits, counts and histograms exact; unscored positions exactly 0; row means rtol 2e-5; per-position nll /
entropy within 4 x (the float32 numpy evaluation's own distance from float64 on the same inputs) + 4 ulp of the position's
largest |logit| (the "4 x model" rule of test_x3_range_gpu.py); model level: codes and code counts exact, per-position nll
within 2e-4 of the logits' max for the tiny configurations and 5e-4 at the reference widths (twice the logit error the
decoder is held to: nll is a difference of two quantities that each move by at most the logit error), row means rtol 2e-5.
Measured on MI355X: 3e-7 .. 4e-7 of the logits' max (tiny, fp32 engine), 1.1e-6 (reference widths, fp16x3 engine)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import ref_model as M

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import score_ref as SR  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def logits_like_model(B, Q, T, seed):
    """Random logits with the spread of a trained decoder's: a few nats of noise plus a peak per position."""
    g = np.random.RandomState(seed)
    z = (g.randn(B, Q, T) * 2.5).astype(np.float32)
    peak = g.randint(0, Q, (B, T))
    np.put_along_axis(z, peak[:, None, :], np.take_along_axis(z, peak[:, None, :], 1) + g.rand(B, 1, T).astype(np.float32) * 8, 1)
    lab = np.where(g.rand(B, T) < 0.5, peak, g.randint(0, Q, (B, T))).astype(np.int32)
    return z, lab


def ranges_for(T):
    """Four rows: whole, t_begin > 0 with a ragged end, empty, first half."""
    return np.array([0, T // 3, 10, 0], np.int32), np.array([T, T - 5, 10, T // 2 + 1], np.int32)


# ------------------------------------------------------------------ kernels alone
@pytest.mark.parametrize('with_ranges', [False, True])
@pytest.mark.parametrize('T', [64, 200, 6656])
@pytest.mark.parametrize('Q', [4, 256, 1024])
def test_softmax_score_against_float64(K, Q, T, with_ranges):
    """Measured on MI355X (worst position over the 18 cases; the test prints every case): the float32 numpy evaluation is up
    to 4.97e-6 (nll) / 6.12e-6 (entropy) from float64 (Q 1024, T 6656), the kernel up to 1.74e-6 / 9.29e-7 on the same inputs;
    at Q 4 both are about 1e-6 (the same figure: the nll there is rounding of the final subtraction)."""
    B = 4
    z, lab = logits_like_model(B, Q, T, seed=Q + T)
    z[0, :, 3] = z[0, 0, 3]                                  # a position whose logits are all equal: index 0 is the greedy choice
    lab[0, 3] = 0
    z[1, 1, T // 2], z[1, 2, T // 2] = 30.0, 30.0            # a tie at the maximum: the lowest index wins
    lab[1, T // 2] = 2
    tb, te = ranges_for(T) if with_ranges else (None, None)
    ref = SR.score_ref(z, lab, tb, te)
    r32 = SR.score_ref(z, lab, tb, te, dtype=np.float32)
    zd, ld = torch.from_numpy(z).cuda(), torch.from_numpy(lab).cuda()
    tbd = None if tb is None else torch.from_numpy(tb).cuda()
    ted = None if te is None else torch.from_numpy(te).cuda()
    nll = torch.full((B, T), float('nan'), device='cuda')
    ent = torch.full((B, T), float('nan'), device='cuda')
    sums, counts = K.softmax_score(zd, ld, t_begin=tbd, t_end=ted, nll=nll, entropy=ent)
    sums, counts, nll, ent = sums.cpu().numpy(), counts.cpu().numpy(), nll.cpu().numpy(), ent.cpu().numpy()
    assert counts[:, 0].tolist() == ref['count'].tolist()
    assert counts[:, 1].tolist() == ref['hits'].tolist()
    assert (nll[~ref['mask']] == 0).all() and (ent[~ref['mask']] == 0).all()
    ulp = np.spacing(np.abs(z).max(axis=1).astype(np.float32)).astype(np.float64)
    for name, got in (('nll', nll), ('entropy', ent)):
        model = np.abs(r32[name].astype(np.float64) - ref[name]).max()
        err = np.abs(got.astype(np.float64) - ref[name])
        print('Q %d T %d ranges %s %s: float32 numpy %.3g, kernel %.3g' % (Q, T, with_ranges, name, model, err.max()))
        assert (err <= 4 * model + 4 * ulp).all(), (name, err.max(), model)
    scored = ref['count'] > 0
    np.testing.assert_allclose(sums[scored, 0] / ref['count'][scored], ref['nll_sum'][scored] / ref['count'][scored], rtol=2e-5)
    np.testing.assert_allclose(sums[scored, 1] / ref['count'][scored], ref['entropy_sum'][scored] / ref['count'][scored], rtol=2e-5)
    assert (sums[~scored] == 0).all()
    # the outputs are optional: the sums alone come out the same
    sums2, counts2 = K.softmax_score(zd, ld, t_begin=tbd, t_end=ted)
    assert np.array_equal(sums2.cpu().numpy().view(np.int64), sums.view(np.int64)) and np.array_equal(counts2.cpu().numpy(), counts)


@pytest.mark.parametrize('Q, T', [(256, 6656), (1024, 200), (4, 64)])
def test_row_sums_reproducible_and_row_independent(K, Q, T):
    B = 4
    z, lab = logits_like_model(B, Q, T, seed=7)
    tb, te = ranges_for(T)
    zd, ld, tbd, ted = (torch.from_numpy(a).cuda() for a in (z, lab, tb, te))
    s1, c1 = K.softmax_score(zd, ld, t_begin=tbd, t_end=ted)
    s2, c2 = K.softmax_score(zd, ld, t_begin=tbd, t_end=ted)
    assert torch.equal(s1.view(torch.int64), s2.view(torch.int64)) and torch.equal(c1, c2)
    for b in range(B):
        sb, cb = K.softmax_score(zd[b:b + 1].contiguous(), ld[b:b + 1].contiguous(), t_begin=tbd[b:b + 1].contiguous(),
                                 t_end=ted[b:b + 1].contiguous())
        assert torch.equal(sb.view(torch.int64), s1[b:b + 1].view(torch.int64)) and torch.equal(cb, c1[b:b + 1]), b


def test_softmax_score_refuses(K):
    z, lab = torch.zeros(1, 6, 64, device='cuda'), torch.zeros(1, 64, dtype=torch.int32, device='cuda')
    with pytest.raises(RuntimeError, match='multiple of 4'):
        K.softmax_score(z, lab)
    with pytest.raises(ValueError, match='int32'):
        K.softmax_score(torch.zeros(1, 8, 64, device='cuda'), lab.long())
    with pytest.raises(ValueError, match='t_end'):
        K.softmax_score(torch.zeros(2, 8, 64, device='cuda'), torch.zeros(2, 64, dtype=torch.int32, device='cuda'),
                        t_end=torch.zeros(1, dtype=torch.int32, device='cuda'))


@pytest.mark.parametrize('B, Tz, Kc', [(8, 104, 512), (3, 7, 32), (2, 5000, 10000)])
def test_code_histogram(K, B, Tz, Kc):
    g = np.random.RandomState(B + Tz)
    idx = g.randint(0, Kc, (B, Tz)).astype(np.int64)
    idx[0, :Tz // 2] = 3                                      # a hot code
    fe = g.randint(0, Tz + 1, B).astype(np.int32)
    fe[0] = Tz
    idxd = torch.from_numpy(idx).cuda()
    for f_end in (None, fe):
        counts = torch.zeros(Kc, dtype=torch.int32, device='cuda')
        flag = torch.zeros(1, dtype=torch.int32, device='cuda')
        fd = None if f_end is None else torch.from_numpy(f_end).cuda()
        K.code_histogram(idxd, counts, flag, f_end=fd)
        want, _ = SR.histogram_ref(idx, Kc, f_end)
        assert np.array_equal(counts.cpu().numpy(), want) and int(flag) == 0
        if f_end is None:
            assert np.array_equal(want, np.bincount(idx.reshape(-1), minlength=Kc))
        K.code_histogram(idxd, counts, flag, f_end=fd)       # it accumulates
        assert np.array_equal(counts.cpu().numpy(), 2 * want) and int(flag) == 0
    # an index outside [0, K) raises the flag and changes no count; guard words around the table stay untouched
    bad = idx.copy()
    bad[B - 1, 0], bad[0, Tz - 1] = Kc, -1
    buf = torch.full((Kc + 128,), -7, dtype=torch.int32, device='cuda')
    counts = buf[64:64 + Kc]
    counts.zero_()
    flag = torch.zeros(1, dtype=torch.int32, device='cuda')
    K.code_histogram(torch.from_numpy(bad).cuda(), counts, flag)
    want, outside = SR.histogram_ref(bad, Kc)
    assert outside and int(flag) != 0 and np.array_equal(counts.cpu().numpy(), want) and int(want.sum()) == B * Tz - 2
    assert (buf[:64] == -7).all() and (buf[64 + Kc:] == -7).all()


# ------------------------------------------------------------------ model level
def tiny_cfg():
    from test_model_gpu import tiny_cfg as f
    return f()


def two_parameter_sets(m, w, S, seed):
    """Live and EMA parameters with distinct values; the BatchNorm moving statistics (not averaged) are the live set's."""
    P = M.init_params(m, w, S, seed=seed, randomize_all=True)
    E = M.init_params(m, w, S, seed=seed + 100, randomize_all=True)
    for n in P:
        if not M.is_trainable(n):
            E[n] = P[n].clone()
    return P, E


def build_model(pkg, m, w, S, seed):
    P, E = two_parameter_sets(m, w, S, seed)
    model = pkg.model.VQVAE(m, w, S, device='cuda', seed=0)
    model.load_named(E)                     # -> live and EMA
    model.load_named(P, also_ema=False)     # -> live only
    assert not torch.equal(model.flat, model.ema)
    return model, P, E


def padded_batch(B, T, S, lengths, seed):
    x, spk, _ = M.synthetic_batch(B, T, S, seed)
    for b, n in enumerate(lengths):
        x[b, n:] = 0
    return x, spk


def check_against_oracle(model, x, spk, lengths, P, m, w, weights, bar):
    B, T = x.shape[0], x.shape[1]
    with torch.no_grad():
        ref = M.forward(x, spk, P, m, w)
    Q = w['quantization_channels']
    z = ref['logits'].reshape(B, T, Q).permute(0, 2, 1).double().numpy()
    lab = ref['labels'].reshape(B, T).numpy()
    want = SR.score_ref(z, lab, None, lengths)
    sc = model.evaluate(x[:, :, 0].contiguous().cuda(), spk.cuda(), lengths=lengths, weights=weights, per_position=True)
    ratio = 64
    assert torch.equal(sc.codes.cpu(), ref['q']), 'VQ codes differ from the oracle'
    q = ref['q'].numpy()
    counts = sum(np.bincount(q[b, :n // ratio], minlength=m['k']) for b, n in enumerate(lengths))
    assert np.array_equal(sc.code_counts.numpy(), counts)
    assert sc.frames.tolist() == [n // ratio for n in lengths] and sc.count.tolist() == list(lengths)
    nll = sc.nll.cpu().double().numpy()
    assert (nll[~want['mask']] == 0).all() and (sc.entropy.cpu().numpy()[~want['mask']] == 0).all()
    err, zmax = np.abs(nll - want['nll']).max(), np.abs(z).max()
    print('%s weights: per-position nll error %.3g = %.3g of the logits\' max %.3g (bound %.3g)' % (weights, err, err / zmax, zmax, bar))
    assert err <= bar * zmax
    np.testing.assert_allclose(sc.nll_sum.numpy() / sc.count.numpy(), want['nll_sum'] / want['count'], rtol=2e-5)
    np.testing.assert_allclose(sc.entropy_sum.numpy() / sc.count.numpy(), want['entropy_sum'] / want['count'], rtol=2e-5)
    # VQ distances: z_e is held to 2e-4 of its max (test_model_gpu.py); d = sum_D (z - e)^2 moves by at most 2 sqrt(D d) per unit of it
    d = ((ref['z_e'] - ref['e_k']) ** 2).sum(-1).double().numpy()                       # [B][Tz]
    dz = 2e-4 * float(ref['z_e'].abs().max())
    for b, n in enumerate(lengths):
        f = n // ratio
        assert abs(float(sc.vq_sum[b]) - d[b, :f].sum()) <= (2 * np.sqrt(m['latent_dim'] * d[b, :f]) * dz).sum() + 1e-6 * d[b, :f].sum()
    return sc


def test_evaluate_tiny_against_oracle(pkg):
    m, w = tiny_cfg()
    model, P, E = build_model(pkg, m, w, 10, seed=3)
    lengths = [512, 320, 128]
    x, spk = padded_batch(3, 512, 10, lengths, seed=21)
    check_against_oracle(model, x, spk, lengths, E, m, w, 'ema', bar=2e-4)
    check_against_oracle(model, x, spk, lengths, P, m, w, 'live', bar=2e-4)
    with pytest.raises(ValueError, match='lengths'):
        model.evaluate(x[:, :, 0].contiguous().cuda(), spk.cuda(), lengths=[512, 100, 64])
    with pytest.raises(ValueError, match='lengths'):
        model.evaluate(x[:, :, 0].contiguous().cuda(), spk.cuda(), lengths=[576, 64, 64])
    with pytest.raises(ValueError, match='lengths'):
        model.evaluate(x[:, :, 0].contiguous().cuda(), spk.cuda(), lengths=[512, 64])
    with pytest.raises(ValueError, match='weights'):
        model.evaluate(x[:, :, 0].contiguous().cuda(), spk.cuda(), weights='best')


def test_evaluate_reference_widths_default_engine(pkg):
    m, w = dict(M.DEFAULT_MODEL), dict(M.DEFAULT_WAVENET)
    model, _, _ = build_model(pkg, m, w, 10, seed=5)
    assert model.x3_guard
    lengths = [512, 256, 64]
    x, spk = padded_batch(3, 512, 10, lengths, seed=22)
    # two training steps on a batch of the same loudness give the guarded engine its plane scales (the first one measures them
    # on the fp32 engine); the oracle then scores with the EMA shadows those steps left
    xt, st, _ = M.synthetic_batch(3, 512, 10, 23)
    for _ in range(2):
        model.train_step(xt[:, :, 0].contiguous().cuda(), st.cuda())
    E = {n: v.cpu() for n, v in model.named_parameters(ema=True).items()}
    check_against_oracle(model, x, spk, lengths, E, m, w, 'ema', bar=5e-4)
    assert model._workspace(3, 512, 'score')['x3_used'], 'the evaluation fell back to the fp32 engine'


def test_prior_evaluate_against_restatement(pkg):
    from test_prior_gpu import random_params, ref_logits, tiny_prior
    cfg = tiny_prior()
    prior = pkg.prior.LatentPrior(cfg, 10, device='cuda', seed=0)
    P, E = random_params(prior, 1), random_params(prior, 2)
    prior.load_named(E)
    prior.load_named(P, also_ema=False)
    g = torch.Generator().manual_seed(4)
    codes = torch.randint(0, cfg['quantization_channels'], (3, 128), generator=g)
    spk = torch.randint(0, 10, (3,), generator=g)
    lengths = [128, 100, 7]
    for weights, W in (('ema', E), ('live', P)):
        with torch.no_grad():
            z = ref_logits(codes, spk, W, cfg).permute(0, 2, 1).double().numpy()
        want = SR.score_ref(z, codes.numpy(), None, lengths)
        sc = prior.evaluate(codes.int().cuda(), spk.cuda(), lengths=lengths, weights=weights, per_position=True)
        assert sc.count.tolist() == lengths and sc.code_counts is None
        err, zmax = np.abs(sc.nll.cpu().double().numpy() - want['nll']).max(), np.abs(z).max()
        print('prior %s: per-position nll error %.3g of the logits\' max' % (weights, err / zmax))
        assert err <= 2e-4 * zmax
        np.testing.assert_allclose(sc.nll_sum.numpy() / sc.count.numpy(), want['nll_sum'] / want['count'], rtol=2e-5)
        np.testing.assert_allclose(sc.entropy_sum.numpy() / sc.count.numpy(), want['entropy_sum'] / want['count'], rtol=2e-5)
    with pytest.raises(ValueError, match='lengths'):
        prior.evaluate(codes.int().cuda(), spk.cuda(), lengths=[128, 0, 7])


def snapshot(model):
    names = ('flat', 'ema', 'adam_m', 'adam_v', 'bn_mean', 'bn_var', 'x3_scale', 'x3_amax', 'x3_flag', 'x3_void')
    return {n: getattr(model, n).clone() for n in names}, model.global_step


def assert_unchanged(model, snap):
    tensors, gs = snap
    assert model.global_step == gs
    for n, t in tensors.items():
        assert torch.equal(getattr(model, n).view(torch.int32), t.view(torch.int32)), n + ' changed'


def test_evaluate_preserves_state(pkg, monkeypatch):
    m, w = tiny_cfg()
    model, _, _ = build_model(pkg, m, w, 10, seed=8)
    x, spk, _ = M.synthetic_batch(2, 512, 10, 5)
    xd, sd = x[:, :, 0].contiguous().cuda(), spk.cuda()
    model.train_step(xd, sd)
    model.train_step(xd, sd)
    snap = snapshot(model)
    model.evaluate(xd, sd, weights='ema')
    assert_unchanged(model, snap)
    model.evaluate(xd, sd, lengths=[512, 64], weights='live')
    assert_unchanged(model, snap)

    def boom(*a, **k):
        raise RuntimeError('halfway')
    monkeypatch.setattr(pkg.kernels, 'speaker_tile_fwd', boom)      # after the decoder's prologue and the encoder
    for weights in ('ema', 'live'):
        with pytest.raises(RuntimeError, match='halfway'):
            model.evaluate(xd, sd, weights=weights)
        assert_unchanged(model, snap)
    monkeypatch.undo()


def test_loud_evaluation_leaves_guard_scales(pkg):
    """Guarded engine, reference widths: an evaluation batch 100 x louder than the training batch (the planes scaled for the
    quiet batch overflow: the pass is repeated on the fp32 engine) leaves x3_scale / x3_amax untouched."""
    m, w = dict(M.DEFAULT_MODEL), dict(M.DEFAULT_WAVENET)
    model = pkg.model.VQVAE(m, w, 10, device='cuda', seed=0)
    assert model.x3_guard
    x, spk, _ = M.synthetic_batch(1, 512, 10, 9)
    xd, sd = x[:, :, 0].contiguous().cuda(), spk.cuda()
    model.train_step(xd * 0.01, sd)
    model.train_step(xd * 0.01, sd)
    snap = snapshot(model)
    sc = model.evaluate(xd, sd, weights='live')
    assert np.isfinite(sc.nll_sum.numpy()).all() and sc.count.tolist() == [512]
    assert_unchanged(model, snap)


def unique_bytes(ws):
    seen = {}
    for v in ws.values():
        for t in (v if isinstance(v, (list, tuple)) else v.values() if isinstance(v, dict) else [v]):
            if torch.is_tensor(t):
                seen[t.data_ptr()] = max(seen.get(t.data_ptr(), 0), t.numel() * t.element_size())
    return sum(seen.values())


TRAIN_KEYS = {'B', 'T', 'Tl', 'Tz', 'X', '_poison', 'bskip', 'cond', 'condenc', 'dX', 'dcond', 'dcondenc', 'dnet', 'dnet_ring', 'dp',
              'dpre', 'dpre_ring', 'dscale', 'dz', 'e_k', 'gated', 'gp', 'gr', 'h1', 'idx', 'inputs', 'labels', 'logits', 'mind', 'net',
              'r', 'ratio', 'scale', 'sg', 'shift', 'skip', 'th', 'wdg', 'wgb', 'wgb_top', 'wop', 'wop_all', 'wp', 'wp_all', 'wres',
              'wskip', 'xp', 'xp_all', 'y6', 'z_e'}
ENCODE_KEYS = {'B', 'T', 'Tl', 'Tz', 'X', '_poison', 'cond', 'e_k', 'idx', 'inputs', 'labels', 'mind', 'ratio', 'scale', 'shift', 'z_e'}


def test_score_workspace(pkg):
    m, w = tiny_cfg()
    model = pkg.model.VQVAE(m, w, 10, device='cuda', seed=0)
    B, T, L, R = 2, 512, len(w['dilation_rates']), w['residual_filters']
    enc = model._workspace(B, T, False)
    assert set(enc) == ENCODE_KEYS
    train = model._workspace(B, T, True)
    assert set(train) == TRAIN_KEYS
    assert len(train['net']) == L + 1 and len({t.data_ptr() for t in train['net']}) == L + 1
    for name in ('gated', 'th', 'sg'):
        assert len({t.data_ptr() for t in train[name]}) == L and tuple(train[name][0].shape) == (B, R, T)
    assert tuple(train['logits'].shape) == (B, 256, T) and tuple(train['dpre'].shape) == (B, 2 * R, T)
    assert tuple(enc['cond'].shape) == (B, model.Cc, T // 64)
    score = model._workspace(B, T, 'score')
    assert score is not train and model._workspace(B, T, 'score') is score
    for name, v in score.items():
        if isinstance(v, list) and v and torch.is_tensor(v[0]) and v[0].dtype == torch.float32 and name != 'X':
            assert len({t.data_ptr() for t in v}) <= 2, name + ': a list of per-layer fp32 buffers'
    assert len(score['net']) == L + 1 and len(score['gated']) == L
    assert not ({'th', 'sg', 'dnet', 'dpre', 'dnet_ring', 'dpre_ring', 'xp_all', 'dp', 'gr', 'r', 'dX', 'y6'} & set(score))
    print('workspace bytes (tiny, B 2, T 512): train %d, score %d' % (unique_bytes(train), unique_bytes(score)))
    assert unique_bytes(score) < unique_bytes(train)


# ------------------------------------------------------------------ command lines
def test_cli_evaluate_and_train_hook(pkg, tmp_path):
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
    rels = write_dataset(root, [1000, 700, 1500], speakers=['p%d' % (225 + i) for i in range(109)])   # synthetic training: 109 speakers
    (tmp_path / 'held.txt').write_text('\n'.join(rels) + '\n')
    env = dict(os.environ, PYTHONPATH=ROOT)
    cwd = str(tmp_path)
    train = [sys.executable, os.path.join(ROOT, 'train.py'), '-dataset', 'synthetic', '-length', '512', '-batch', '2', '-step', '4',
             '-interval', '1', '-params', str(tmp_path / 'm.json')]
    out = subprocess.run(train + ['-save', 'plain/weights'], cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert 'eval' not in out.stdout
    plain = [json.loads(ln) for ln in (tmp_path / 'plain' / 'summaries.jsonl').read_text().splitlines()]
    parent_keys = {'global_step', 'learning_rate', 'q(z|x)', 'distances_min', 'z_e', 'z_e_u', 'z_e_v', 'speaker_embedding',
                   'speaker_embedding_u', 'speaker_embedding_v', 'embedding', 'embedding_u', 'embedding_v', 'e_k',
                   'reconstruction_loss', 'vq_loss', 'commitment_loss'}
    assert len(plain) == 4 and all(set(ln) == parent_keys for ln in plain)
    out = subprocess.run(train + ['-save', 'saved_model/weights', '-eval_list', str(tmp_path / 'held.txt'), '-eval_interval', '2',
                                  '-eval_batches', '1', '-data_root', root],
                         cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert '[eval bits ' in out.stdout
    lines = [json.loads(ln) for ln in (tmp_path / 'saved_model' / 'summaries.jsonl').read_text().splitlines()]
    assert [ln['global_step'] for ln in lines] == [1, 2, 3, 4] and ['eval' in ln for ln in lines] == [False, True, False, True]
    assert lines[1]['eval']['samples'] == 2 * 512 and 0 < lines[1]['eval']['bits_per_sample'] < 16
    assert all(set(ln) - {'eval'} == parent_keys for ln in lines)
    ckpt = tmp_path / 'saved_model' / 'weights-4.pt'
    rep_path = tmp_path / 'eval.json'
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'evaluate.py'), '-restore', str(ckpt), '-dataset', 'VCTK', '-list',
                          str(tmp_path / 'held.txt'), '-data_root', root, '-batch', '2', '-params', str(tmp_path / 'm.json'),
                          '-per_utterance', '-out', str(rep_path)], cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    rep = json.loads(rep_path.read_text())
    assert json.loads(out.stdout.strip().splitlines()[-1]) == rep
    assert rep['step'] == 4 and rep['weights'] == 'ema' and rep['utterances'] == 3 and rep['skipped'] == 0 and rep['codes'] == 32
    by_file = {r['file']: r for r in rep['per_utterance']}
    assert [by_file[r]['samples'] for r in rels] == [960, 640, 1472]
    assert rep['samples'] == 960 + 640 + 1472
    # the same totals in-process, on the same files
    D, S = pkg.data, pkg.scoring
    held = D.HeldOutList('VCTK', str(tmp_path / 'held.txt'), relative_path=root, ratio=64)
    model = pkg.model.VQVAE(m, w, held.num_speakers, device='cuda', seed=0)
    model.load_state_dict(torch.load(str(ckpt), map_location='cpu', weights_only=True))
    totals = S.score_batches(model, D.padded_batches(held.utterances()[0], 2), torch.device('cuda'), weights='ema')
    want = totals.report('sample', latent_dim=model.D)
    # counts are equal; the float sums agree to the forward pass's own run-to-run noise (the encoder's short layers add their
    # split-K slices with fp32 atomics, so two processes do not make the same logits bit for bit; measured: 2e-9 relative)
    for k, v in want.items():
        if isinstance(v, float):
            print('%s: evaluate.py %r, in-process %r' % (k, rep[k], v))
            assert rep[k] == pytest.approx(v, rel=1e-6), k
        else:
            assert rep[k] == v, k
    # a speaker table of another size is refused
    with open(os.path.join(root, 'vctk_speakers.txt'), 'a') as f:
        f.write('p999, 109\n')
    bad = subprocess.run([sys.executable, os.path.join(ROOT, 'evaluate.py'), '-restore', str(ckpt), '-list', str(tmp_path / 'held.txt'),
                          '-data_root', root, '-params', str(tmp_path / 'm.json')], cwd=cwd, env=env, capture_output=True, text=True,
                         timeout=600)
    assert bad.returncode == 2 and '109 speakers' in bad.stderr
