"""CPU tests of clipping by global norm: the chunk table of the norm pass (kernels.grad_norm_plan), the
properties of the float64 restatement the GPU tests compare against (clip_ref.py), the command-line checks of train.py /
train_prior.py, and the presence of the feature's entry points."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_ref as CR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def segment_lengths(chunk):
    return [1, 3, 4, 5, chunk - 1, chunk, chunk + 1, 2 * chunk + 7]


@pytest.mark.parametrize('chunk', [16, None], ids=['chunk16', 'default'])
def test_grad_norm_plan_covers_every_element_once(K, chunk):
    chunk = chunk or K.GRAD_NORM_CHUNK
    bounds = np.concatenate(([0], np.cumsum(segment_lengths(chunk))))
    plan = K.grad_norm_plan(bounds, chunk)
    assert plan.n_seg == 8 and plan.n_chunks == len(plan.start) == len(plan.length) == len(plan.seg)
    cover = np.zeros(bounds[-1], np.int32)
    for s, n, k in zip(plan.start, plan.length, plan.seg):
        assert 1 <= n <= chunk
        assert bounds[k] <= s and s + n <= bounds[k + 1], 'chunk (%d, %d) crosses segment %d' % (s, n, k)
        cover[s:s + n] += 1
    assert np.all(cover == 1)
    assert np.all(np.diff(plan.start) > 0) and np.all(np.diff(plan.seg) >= 0)
    assert plan.end == bounds[-1]


def test_grad_norm_plan_refuses_an_empty_segment(K):
    with pytest.raises(ValueError, match='empty'):
        K.grad_norm_plan([0, 5, 5, 9], 4)
    with pytest.raises(ValueError):
        K.grad_norm_plan([0], 4)
    with pytest.raises(ValueError, match='empty'):
        K.grad_norm_plan_runs([(0, 4, 0), (8, 4, 2)], 3, 4)
    with pytest.raises(ValueError, match='overlap'):
        K.grad_norm_plan_runs([(0, 6, 0), (4, 4, 1)], 2, 4)


def test_grad_norm_plan_segments_need_not_be_contiguous(K):
    """A reference variable that is a column block of a grouped kernel: one run per row, all in one segment."""
    runs = [(r * 10, 6, 0) for r in range(3)] + [(r * 10 + 6, 4, 1) for r in range(3)]
    plan = K.grad_norm_plan_runs(runs, 2, 4)
    assert list(plan.seg) == [0] * 6 + [1] * 3
    cover = np.zeros(30, np.int32)
    for s, n in zip(plan.start, plan.length):
        cover[s:s + n] += 1
    assert np.all(cover == 1)


def test_reference_scale_is_exactly_one_under_the_threshold():
    rng = np.random.default_rng(5)
    g = rng.standard_normal(1000).astype(np.float32)
    _, norm = CR.segment_norms(g, [0, 400, 1000])
    n32 = float(np.float32(norm))
    assert CR.clip_scale(norm, n32) == 1.0                   # norm == clip
    assert CR.clip_scale(norm, 2 * norm) == 1.0
    assert CR.clip_scale(norm, float('inf')) == 1.0
    assert CR.clip_scale(norm, float(np.nextafter(np.float32(n32), np.float32(0)))) < 1.0


@pytest.mark.parametrize('grad_scale', [1.0, 0.5])
def test_reference_clipped_gradient_has_norm_clip(grad_scale):
    rng = np.random.default_rng(6)
    g = (rng.standard_normal(5000) * 3.0).astype(np.float32)
    norms, norm = CR.segment_norms(g, [0, 7, 4096, 5000], grad_scale)
    assert abs(np.sqrt(np.sum(norms ** 2)) - norm) <= 1e-12 * norm
    clip = 0.37 * norm
    s = CR.clip_scale(norm, clip)
    clipped = CR.scaled_grad(g, grad_scale) * s
    got = float(np.sqrt(np.sum(clipped ** 2)))
    assert abs(got - clip) <= 2.0 ** -22 * clip              # the fp32 roundings of norm and clip


@pytest.mark.parametrize('script,pre', [('train.py', []), ('train_prior.py', ['-restore', 'none.pt'])])
@pytest.mark.parametrize('value', ['0', '-1', 'nan'])
def test_bad_clip_norm_exits_before_anything_is_loaded(tmp_path, script, pre, value):
    out = subprocess.run([sys.executable, os.path.join(ROOT, script)] + pre + ['-clip_norm', value], cwd=str(tmp_path),
                         env=dict(os.environ, HIP_VISIBLE_DEVICES='', CUDA_VISIBLE_DEVICES=''), capture_output=True, text=True, timeout=120)
    assert out.returncode == 2, (out.returncode, out.stderr[-500:])
    assert '-clip_norm must be > 0' in out.stderr          # the script's own check, not argparse's "unrecognized arguments"


def test_threshold_is_checked_as_the_fp32_the_kernels_receive(K):
    assert K.clip_as_fp32(1e-50) == 0.0 and K.clip_as_fp32(1e-45) > 0.0
    assert K.clip_as_fp32(float('inf')) == float('inf') and K.clip_as_fp32(1e39) == float('inf')
    assert K.clip_as_fp32(float('nan')) != K.clip_as_fp32(float('nan'))
    assert K.clip_as_fp32(0.5) == 0.5


def test_feature_entry_points_exist(pkg):
    assert callable(getattr(pkg.model.VQVAE, 'grad_norms', None))
    assert isinstance(pkg.model.VQVAE.clip_norm, property)
    assert callable(getattr(pkg.prior.LatentPrior, 'grad_norms', None))
    for name in ('vqw_grad_norm_segmented', 'vqw_adam_ema_step_scaled'):
        assert name in pkg._lib.SIGNATURES
        assert hasattr(pkg._lib.lib(), name)


def test_norm_entry_validates_its_arguments(pkg):
    import ctypes
    lib = pkg._lib.lib()
    p = ctypes.c_void_p(256)          # never dereferenced: every call below is refused before a launch
    assert lib.vqw_grad_norm_segmented(None, p, 1, 1, p, 1.0, 1.0, p, None) != 0
    assert b'null pointer' in lib.vqw_last_error()
    for clip in (0.0, -1.0, float('nan')):
        assert lib.vqw_grad_norm_segmented(p, p, 1, 1, p, 1.0, clip, p, None) != 0
        assert b'clip' in lib.vqw_last_error()
    assert lib.vqw_grad_norm_segmented(p, p, 1, 0, p, 1.0, 1.0, p, None) != 0
    assert b'n_seg' in lib.vqw_last_error()
    assert lib.vqw_adam_ema_step_scaled(None, None, None, None, None, 4, 1e-3, 0.9, 0.999, 1e-8, 0.999, 1.0, None, None, None) != 0
    assert b'null pointer' in lib.vqw_last_error()
