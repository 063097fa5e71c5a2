"""CPU tests of the time-jitter regulariser: the properties of the numpy restatement the GPU tests compare
against (jitter_ref.py), the command-line check of train.py and the configuration key."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jitter_ref as JR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('Tz', [1, 2, 3, 104])
def test_reference_source_frames(Tz):
    rng = np.random.default_rng(Tz)
    u = rng.random((5, Tz), dtype=np.float32)
    t = np.arange(Tz)[None, :]
    for p in (0.0, 0.12, 0.5, 1.0):
        src = JR.src_of(u, p)
        assert src.dtype == np.int32 and src.shape == u.shape
        assert (np.abs(src - t) <= 1).all() and (src >= 0).all() and (src < Tz).all()
    assert (JR.src_of(u, 0.0) == t).all()                                 # p = 0: the identity
    if Tz >= 2:
        assert (JR.src_of(u, 1.0) != t).all()                             # p = 1: every frame moves
        left = np.full((1, Tz), 0.0, np.float32)                          # u < lo everywhere: every frame looks left,
        assert JR.src_of(left, 0.5).tolist() == [[1] + list(range(Tz - 1))]     # frame 0 reflects to frame 1
        right = np.full((1, Tz), 0.99, np.float32)                        # u >= hi everywhere: frame Tz-1 reflects to Tz-2
        assert JR.src_of(right, 0.5).tolist() == [list(range(1, Tz)) + [Tz - 2]]
    else:
        assert (JR.src_of(u, 1.0) == 0).all()


def test_thresholds_are_rounded_once_and_compared_in_fp32():
    lo, hi = JR.thresholds(0.12)
    assert lo.dtype == np.float32 and hi.dtype == np.float32
    assert lo == np.float32(0.06) and hi == np.float32(0.94)
    u = np.array([[np.nextafter(lo, np.float32(0)), lo, 0.5, np.nextafter(hi, np.float32(0)), hi]], np.float32)
    assert JR.src_of(u, 0.12).tolist() == [[1, 1, 2, 3, 3]]              # just below lo moves (reflected), lo itself stays;
    #                                                                      just below hi stays, hi itself moves (reflected)


@pytest.mark.parametrize('Tz', [1, 2, 3, 104])
def test_backward_is_the_adjoint_of_forward(Tz):
    rng = np.random.default_rng(100 + Tz)
    u = rng.random((3, Tz), dtype=np.float32)
    src = JR.src_of(u, 0.7)
    z, g = rng.standard_normal((3, 6, Tz)), rng.standard_normal((3, 6, Tz))
    a, b = float(np.sum(JR.fwd(z, src) * g)), float(np.sum(z * JR.bwd(g, src)))
    assert abs(a - b) <= 1e-12 * max(abs(a), abs(b), 1e-300)
    dz = JR.bwd(g.astype(np.float32), src)
    assert dz.dtype == np.float32
    # frames nobody read get +0.0, and a row's gradient never leaves the row
    read = np.zeros((3, Tz), bool)
    np.put_along_axis(read, src.astype(np.int64), True, axis=1)
    assert (dz[np.broadcast_to(~read[:, None, :], dz.shape)] == 0).all()


def test_moved_share_at_p_012():
    """10^6 draws: the moved share is binomial with sigma = sqrt(0.12 * 0.88 / 1e6) = 3.2e-4, so 2e-3 is about six sigma."""
    u = np.random.default_rng(7).random((1000, 1000), dtype=np.float32)
    lo, hi = JR.thresholds(0.12)
    left, right = float((u < lo).mean()), float((u >= hi).mean())
    assert abs(left - 0.06) < 2e-3 and abs(right - 0.06) < 2e-3
    src = JR.src_of(u, 0.12)
    moved = float((src != np.arange(1000)[None, :]).mean())
    assert abs(moved - 0.12) < 2e-3


@pytest.mark.parametrize('value', ['1.5', '-0.1'])
def test_bad_time_jitter_exits_before_anything_is_loaded(tmp_path, value):
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'train.py'), '-time_jitter', value], cwd=str(tmp_path),
                         env=dict(os.environ, HIP_VISIBLE_DEVICES='', CUDA_VISIBLE_DEVICES=''), capture_output=True, text=True, timeout=120)
    assert out.returncode == 2, (out.returncode, out.stderr[-500:])
    assert '-time_jitter must be a probability' in out.stderr


def test_config_key_and_entry_points(pkg):
    """Absent key = off; values outside [0, 1] are refused; the prior refuses the key.  (The constructors need a GPU; what
    they call to read the key does not.)"""
    VQVAE, K = pkg.model.VQVAE, pkg.kernels
    probe = VQVAE.__new__(VQVAE)
    assert probe.time_jitter == 0.0 and probe.jitter_seed == 0
    cfg = {'latent_dim': 16, 'k': 32, 'speaker_embedding': 16, 'beta': 0.25, 'encoder_filters': 48}
    probe._setup_front(cfg, 10)
    assert probe.time_jitter == 0.0
    probe._setup_front(dict(cfg, time_jitter=0.12), 10)
    assert probe.time_jitter == 0.12
    for bad in (1.5, -0.1, float('nan')):
        with pytest.raises(ValueError, match='time_jitter'):
            VQVAE.__new__(VQVAE)._setup_front(dict(cfg, time_jitter=bad), 10)
    assert K.jitter_thresholds(0.12) == tuple(float(v) for v in JR.thresholds(0.12))
    assert K.jitter_thresholds(0.0) == (0.0, 1.0) and K.jitter_thresholds(1.0) == (0.5, 0.5)
    prior_cfg = {'quantization_channels': 32, 'speaker_embedding': 16, 'time_jitter': 0.1}
    P = pkg.prior.LatentPrior
    with pytest.raises(ValueError, match='time_jitter'):
        P.__new__(P)._setup_front(prior_cfg, 10)
    import torch
    with pytest.raises(ValueError, match='GPU'):
        K.time_jitter_fwd(torch.zeros(1, 2, 3), torch.zeros(1, 3), torch.zeros(1, 2, 3), torch.zeros(1, 3, dtype=torch.int32), p=0.5, D=2)
    with pytest.raises(ValueError, match='GPU'):
        K.time_jitter_bwd(torch.zeros(1, 2, 3), torch.zeros(1, 3, dtype=torch.int32), torch.zeros(1, 2, 3), D=2)
