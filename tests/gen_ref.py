"""Float64 parallel references for the two stepping generators (FastGenerator / PriorGenerator; csrc/ar_persist.hip and
csrc/ar_decode.hip) -- plain helpers, no GPU.

A generator steps: sample t is drawn from a distribution that depends on the samples before it, read back out of per-layer
rings.  The references here do not step.  They take the sequence a generator produced, run the TRAINING graph over all of it
at once (a causal dilated convolution, teacher-forced by shift_right) on float64 copies of the parameters, and return the
distribution of every step.  They share nothing with the generators' queue logic: a tap read from the wrong ring slot shows as
a distribution that is not the one the kernel sampled from.

  decoder_probs64  oracle.ref_model.wavenet_build on the generated audio
  prior_probs64    ref_logits of test_prior_gpu.py on the generated codes
  check_sampled    every sampled index is searchsorted(cumsum(p64), u), up to u sitting on a cdf edge
  checkpoints      the steps around which a ring's taps go live and its slots wrap
"""
import importlib.util
import os

import numpy as np
import torch

from oracle import ref_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
EDGE = 2e-6      # |u - cdf| below which a differing index is fp32 noise (the number of test_fast_generation_matches_oracle)


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def prior_tests():
    return _load('prior_gpu_tests', os.path.join(HERE, 'test_prior_gpu.py'))


def tiny_cfg():
    return _load('make_golden', os.path.join(HERE, 'golden', 'make_golden.py')).tiny_cfg()


def to64(P):
    return {n: v.detach().double() for n, v in P.items()}


def decoder_probs64(P, wcfg, audio, enc, idx=None):
    """audio [B,n] (what the generator fed itself), enc [B,Tz,Cc] with n a multiple of Tz -> probabilities float64 [B,n,Q].
    wavenet_build's shift_right makes the input of step t the sample of step t-1 (zero at t = 0).  idx [B,n]: the generator's
    indices; the labels wavenet_build forms from the audio must be them (the mu-law round trip of the generator's own input)."""
    B, n = audio.shape
    x = torch.as_tensor(audio).detach().cpu().double().reshape(B, n, 1)
    with torch.no_grad():
        logits, labels = M.wavenet_build(x, torch.as_tensor(enc).detach().cpu().double(), to64(P), wcfg)
        p = torch.softmax(logits.reshape(B, n, -1), dim=-1)
    assert p.dtype == torch.float64
    if idx is not None:
        want = np.asarray(torch.as_tensor(idx).cpu()).astype(np.int64)
        got = labels.reshape(B, n).numpy().astype(np.int64)
        bad = np.argwhere(got != want)
        assert bad.size == 0, 'mu_law_encode(audio) is not the index at (row, step) %s: %d vs %d' % (
            tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])
    return p.numpy()


def prior_probs64(P, cfg, codes, spk):
    """codes int [B,n] (n a multiple of 64), spk int64 [B] -> probabilities float64 [B,n,k]; the only condition is the speaker."""
    with torch.no_grad():
        logits = prior_tests().ref_logits(torch.as_tensor(codes).cpu().long(), torch.as_tensor(spk).cpu().long(), to64(P), cfg)
        p = torch.softmax(logits, dim=-1)
    assert p.dtype == torch.float64
    return p.numpy()


def check_sampled(p64, u, idx, depths=()):
    """p64 [B,n,Q], u [B,n], idx [B,n]: for every row and step want = min(searchsorted(cumsum(p64), u), Q-1).  A step with
    idx != want is excused only if u lies within EDGE of a cdf value; any other fails, naming the step, the row, both indices
    and the step modulo each ring depth.  Returns the number of excused steps."""
    p64 = np.asarray(p64, dtype=np.float64)
    u = np.asarray(torch.as_tensor(u).cpu(), dtype=np.float64)
    idx = np.asarray(torch.as_tensor(idx).cpu()).astype(np.int64)
    B, n, Q = p64.shape
    assert u.shape == (B, n) and idx.shape == (B, n)
    cdf = np.cumsum(p64, axis=-1)
    want = np.minimum((cdf < u[:, :, None]).sum(-1), Q - 1)          # searchsorted, side='left'
    near = np.abs(cdf - u[:, :, None]).min(-1) < EDGE
    differ = idx != want
    bad = np.argwhere(differ & ~near)
    if bad.size:
        b, t = (int(v) for v in bad[0])
        raise AssertionError('step %d row %d: generator %d, float64 reference %d (u %.9g, nearest cdf edge %.3g away); '
                             '%d of %d steps wrong; step modulo ring depth: %s' % (
                                 t, b, idx[b, t], want[b, t], u[b, t], np.abs(cdf[b, t] - u[b, t]).min(), len(bad), B * n,
                                 ', '.join('%d %% %d = %d' % (t, d, t % d) for d in sorted(set(depths)))))
    return int(differ.sum())


def ring_depths(ks, dilations, persistent=True):
    """Slots of each layer's ring: (ks-1)d + 1 in the persistent kernel (the layer input doubles as the exchange buffer),
    (ks-1)d on the launch-per-phase path."""
    return [(ks - 1) * d + (1 if persistent else 0) for d in dilations]


def checkpoints(n, ks, D):
    """Chunk ends t (ascending) such that the last step s = t-1 of a chunk is each of: the first three steps; c-1, c, c+1 for
    c = D (the near tap of the deepest layer goes live), (ks-1)D (its far tap goes live; the launch-per-phase ring wraps),
    depth = (ks-1)D + 1 (the persistent ring wraps) and 2 depth (it wraps again); n-1.  Steps at or beyond n are dropped."""
    depth = (ks - 1) * D + 1
    last = {0, 1, 2, n - 1}
    for c in (D, (ks - 1) * D, depth, 2 * depth):
        last |= {c - 1, c, c + 1}
    return sorted(s + 1 for s in last if 0 <= s < n)
