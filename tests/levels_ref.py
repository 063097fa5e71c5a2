"""The oracle at a mu-law level -- plain helpers, no GPU.

The oracle's decoder (oracle.ref_model.wavenet_build) calls R.mu_law_encode without a level, as the reference does
(wavenet.py:33,37), while R.mu_law_encode itself takes quantization_channels.  The reference at a level is therefore the
oracle itself with that argument bound: `wavenet_build` here runs M.wavenet_build with R.mu_law_encode bound to the level
of the config FOR THE DURATION OF THAT CALL ONLY (the oracle's encoders, Encoder_Magenta among them, keep their own 255),
and `at_level()` makes M.forward / M.train_step and tests/gen_ref.py (which look M.wavenet_build up at call time) use it.

  levels_of       the level of a class count: Q at 512 and 1024, otherwise 256
  wavenet_build   M.wavenet_build at the level of wcfg['quantization_channels']
  at_level        context: M.wavenet_build is the function above
  decode          R.mu_law_decode_np(idx, Q)
  speech          a speech-like fp32 signal in [-1, 1] (what the cases would catch is computed on it)
"""
import contextlib
import functools

import numpy as np

from oracle import ref_model as M

R = M.R
LEVELS = (256, 512, 1024)
_oracle_build = M.wavenet_build


def levels_of(Q):
    return int(Q) if int(Q) in (512, 1024) else 256


def wavenet_build(x, local_condition, P, wcfg, collect=None, global_condition=None):
    levels = levels_of(wcfg['quantization_channels'])
    saved = R.mu_law_encode
    R.mu_law_encode = functools.partial(saved, quantization_channels=levels)
    try:
        return _oracle_build(x, local_condition, P, wcfg, collect=collect, global_condition=global_condition)
    finally:
        R.mu_law_encode = saved


@contextlib.contextmanager
def at_level():
    saved = M.wavenet_build
    M.wavenet_build = wavenet_build
    try:
        yield
    finally:
        M.wavenet_build = saved


def decode(idx, Q):
    return R.mu_law_decode_np(np.asarray(idx, dtype=np.float32), Q)


def speech(n, seed=0):
    """Voiced-like: a few harmonics under a slow envelope plus a little noise, peak about 0.5, most samples small."""
    rng = np.random.RandomState(seed)
    t = np.arange(n, dtype=np.float64) / 16000.0
    f0 = 120.0 + 30.0 * np.sin(2 * np.pi * 1.5 * t)
    ph = 2 * np.pi * np.cumsum(f0) / 16000.0
    x = sum(a * np.sin(k * ph + p) for k, a, p in ((1, 0.25, 0.0), (2, 0.12, 0.7), (3, 0.08, 1.9), (5, 0.04, 0.3)))
    env = 0.15 + 0.85 * np.abs(np.sin(2 * np.pi * 2.0 * t)) ** 2
    x = x * env + 0.003 * rng.randn(n)
    return np.clip(x, -1.0, 1.0).astype(np.float32)


def with_levels(wcfg, Q):
    return dict(wcfg, quantization_channels=int(Q))
