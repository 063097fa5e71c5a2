"""CPU tests of tests/gen_ref.py: the float64 parallel references that test_generation_long_gpu.py holds the generators to.

The oracle's fp32 stepping generators (FIFO queues) stand in for the kernels: sampled with supplied uniforms over 320 steps of
a stack whose deepest ring (dilation 64) wraps, their per-step probabilities must be the float64 teacher-forced pass's
(rtol 2e-4, atol 1e-7: the bars of the GPU tests) and check_sampled must excuse nothing.  With one dilation off by one in the
reference alone the comparison must fail: a wrong helper cannot make the GPU tests vacuous."""
import math
import os
import sys

import numpy as np
import pytest
import torch

from oracle import ref_model as M

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_ref as G  # noqa: E402

DIL = [1, 2, 4, 8, 16, 32, 64, 1, 2]
B, N = 2, 320


def decoder_cfg(ks):
    m, w = G.tiny_cfg()
    w.update(dilation_rates=list(DIL), num_cycles=1, num_cycle_layers=len(DIL), kernel_size=ks)
    return m, w


def prior_cfg(pre_k):
    cfg = G.prior_tests().tiny_prior(k=32, pre_k=pre_k)
    cfg.update(dilation_rates=list(DIL), num_cycles=1, num_cycle_layers=len(DIL))
    return cfg


def prior_params(cfg, nspk, seed):
    """Every variable of a prior random (the names and shapes of prior.LatentPrior.named_parameters)."""
    g = torch.Generator().manual_seed(seed)
    k, R, S, Df = cfg['quantization_channels'], cfg['residual_filters'], cfg['skip_filters'], cfg['dilation_filters']
    Cs, ks, pk = cfg['speaker_embedding'], cfg['kernel_size'], cfg['preprocess']['kernel_size']

    def w(*shape):
        lim = math.sqrt(3.0 / int(np.prod(shape[:-1])))
        return ((torch.rand(shape, generator=g) * 2 - 1) * lim).float()

    def b(n):
        return (0.1 * torch.randn(n, generator=g)).float()

    P = {'prior/speaker_embedding': w(nspk, Cs) * 2, 'prior/preprocess/kernel': w(pk, k, R), 'prior/preprocess/bias': b(R),
         'prior/skip/kernel': w(1, R, S), 'prior/skip/bias': b(S)}
    for i in range(len(cfg['dilation_rates'])):
        s = M.layer_scope(i, cfg['num_cycle_layers']).replace('decoder/', 'prior/')
        P[s + '/gated/kernel'], P[s + '/gated/bias'] = w(ks, R, 2 * Df), b(2 * Df)
        P[s + '/gated/local_condition/kernel'] = w(1, Cs, 2 * Df)
        P[s + '/skip/kernel'], P[s + '/skip/bias'] = w(1, Df, S), b(S)
        P[s + '/residual/kernel'], P[s + '/residual/bias'] = w(1, Df, R), b(R)
    P['prior/postprocess1/kernel'], P['prior/postprocess1/bias'] = w(1, S, S), b(S)
    P['prior/postprocess1/local_condition/kernel'] = w(1, Cs, S)
    P['prior/postprocess2/kernel'], P['prior/postprocess2/bias'] = w(1, S, k), b(k)
    return P


def step_decoder(P, w, enc, u):
    """The oracle's fp32 FastGenerator in sample mode with supplied uniforms -> (indices, audio, probabilities of every step)."""
    g = M.FastGenerator(P, w, B)
    a = np.zeros([B, 1], np.float32)
    idx, audio, probs = np.zeros([B, N], np.int64), np.zeros([B, N], np.float32), []
    with torch.no_grad():
        for i in range(N):
            pr = g.step(torch.from_numpy(a), enc[:, i // 64]).numpy()
            pred, dec = M.R.sample_with_uniforms(pr, u[:, i].numpy())
            idx[:, i], audio[:, i] = pred, dec
            probs.append(pr)
            a = dec[:, None].astype(np.float32)
    return idx, audio, np.stack(probs, 1)


def step_prior(P, cfg, spk, u):
    pt = G.prior_tests()
    g = pt.RefPriorGen(P, cfg, B)
    cond = P['prior/speaker_embedding'][spk]
    k = cfg['quantization_channels']
    prev, idx, probs = [-1] * B, np.zeros([B, N], np.int64), []
    with torch.no_grad():
        for i in range(N):
            pr = g.step(prev, cond).numpy()
            cdf = np.cumsum(pr, axis=1)
            prev = [min(int(cdf[b].searchsorted(u[b, i].item())), k - 1) for b in range(B)]
            idx[:, i] = prev
            probs.append(pr)
    return idx, np.stack(probs, 1)


def off_by_one(dil):
    d = list(dil)
    d[d.index(64)] = 63
    return d


def fails(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize('ks', [3, 2])
def test_decoder_reference_matches_stepping_oracle(ks):
    m, w = decoder_cfg(ks)
    P = M.init_params(m, w, 10, seed=11, randomize_all=True)
    g = torch.Generator().manual_seed(ks)
    Cc = m['latent_dim'] + m['speaker_embedding']
    enc = 0.5 * torch.randn(B, N // 64, Cc, generator=g)
    u = torch.rand(B, N, generator=g)
    idx, audio, probs = step_decoder(P, w, enc, u)
    assert N > 2 * ((ks - 1) * 64 + 1)                    # the deepest ring wraps twice
    assert all(len(np.unique(r)) >= 100 for r in idx), 'degenerate history'
    p64 = G.decoder_probs64(P, w, audio, enc, idx=idx)
    assert p64.shape == (B, N, 256) and p64.dtype == np.float64
    np.testing.assert_allclose(probs, p64, rtol=2e-4, atol=1e-7)
    assert G.check_sampled(p64, u, idx, G.ring_depths(ks, DIL)) == 0
    # negative control: the reference alone with dilation 64 -> 63
    wrong = dict(w, dilation_rates=off_by_one(DIL))
    q64 = G.decoder_probs64(P, wrong, audio, enc, idx=idx)
    np.testing.assert_allclose(q64[:, :63], p64[:, :63], rtol=1e-12)   # that tap is still in the zero pre-history: no difference yet
    assert fails(lambda: np.testing.assert_allclose(probs, q64, rtol=2e-4, atol=1e-7))
    assert fails(lambda: G.check_sampled(q64, u, idx, G.ring_depths(ks, DIL)))
    # ... and a wrong index is not the audio's label
    bad = idx.copy()
    bad[1, 200] ^= 1
    assert fails(lambda: G.decoder_probs64(P, w, audio, enc, idx=bad))


@pytest.mark.parametrize('pre_k', [1, 3])
def test_prior_reference_matches_stepping_restatement(pre_k):
    cfg = prior_cfg(pre_k)
    P = prior_params(cfg, 10, 5 + pre_k)
    spk = torch.tensor([2, 9])
    u = torch.rand(B, N, generator=torch.Generator().manual_seed(pre_k))
    idx, probs = step_prior(P, cfg, spk, u)
    assert all(len(np.unique(r)) >= 16 for r in idx), 'degenerate history'     # half of the 32 codes
    p64 = G.prior_probs64(P, cfg, idx, spk)
    assert p64.shape == (B, N, 32) and p64.dtype == np.float64
    np.testing.assert_allclose(probs, p64, rtol=2e-4, atol=1e-7)
    assert G.check_sampled(p64, u, idx, G.ring_depths(3, DIL)) == 0
    q64 = G.prior_probs64(P, dict(cfg, dilation_rates=off_by_one(DIL)), idx, spk)
    assert fails(lambda: np.testing.assert_allclose(probs, q64, rtol=2e-4, atol=1e-7))
    assert fails(lambda: G.check_sampled(q64, u, idx, G.ring_depths(3, DIL)))


def test_check_sampled_rules():
    """The excuse is |u - cdf| < 2e-6 and nothing else; the last index is clamped to Q-1."""
    p = np.array([[[0.25, 0.25, 0.5], [0.25, 0.25, 0.5], [0.25, 0.25, 0.5], [0.25, 0.25, 0.5]]])
    u = torch.tensor([[0.1, 0.25 + 1e-6, 0.6, 1.5]], dtype=torch.float64)
    assert G.check_sampled(p, u, np.array([[0, 1, 2, 2]])) == 0
    assert G.check_sampled(p, u, np.array([[0, 0, 2, 2]])) == 1                 # u on the edge between 0 and 1: excused
    with pytest.raises(AssertionError, match=r'step 2 row 0: generator 1, float64 reference 2 .*2 % 5 = 2'):
        G.check_sampled(p, u, np.array([[0, 1, 1, 2]]), depths=[5, 3])
    with pytest.raises(AssertionError, match='step 0 row 0'):
        G.check_sampled(p, u, np.array([[1, 1, 2, 2]]))


def test_checkpoints():
    assert G.checkpoints(2112, 3, 512) == [1, 2, 3, 512, 513, 514, 1024, 1025, 1026, 1027, 2050, 2051, 2052, 2112]
    assert G.checkpoints(2112, 2, 512) == [1, 2, 3, 512, 513, 514, 515, 1026, 1027, 1028, 2112]
    assert G.checkpoints(600, 3, 512) == [1, 2, 3, 512, 513, 514, 600]
    assert G.ring_depths(3, [1, 512]) == [3, 1025] and G.ring_depths(2, [4], persistent=False) == [4]
