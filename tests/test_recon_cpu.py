"""CPU tests of teacher-forced reconstruction: the export and the argument checks of vqw_softmax_sample, the wrapper's refusal of
CPU tensors, the command lines' refusal of bad flag combinations (generate.py -teacher_forced, train.py -audio_interval), and
the float64 restatement over a whole tensor (recon_ref.py) against sampling_ref on a hand-made case."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import recon_ref as RR  # noqa: E402
import sampling_ref as S  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ C ABI
def test_library_exports_and_header_declares(pkg):
    lib = pkg._lib.lib()
    assert hasattr(lib, 'vqw_softmax_sample')
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'vqwave.h')).read(), flags=re.S)
    decl = re.search(r'int\s+vqw_softmax_sample\s*\(([^;]*)\)\s*;', hdr)
    assert decl is not None
    assert len(decl.group(1).split(',')) == len(pkg._lib.SIGNATURES['vqw_softmax_sample'][1]) == 13


def test_softmax_sample_refuses_bad_arguments(pkg):
    """Every refusal comes back as a non-zero return with its text, before any launch (no GPU is needed to be refused)."""
    L = pkg._lib
    lib = L.lib()
    one = ctypes.c_void_p(64)                              # a non-null pointer that is never dereferenced

    def call(logits=one, uniforms=one, rows=None, mode=1, idx=one, audio=None, probs=None, B=1, Q=256, T=64):
        rc = lib.vqw_softmax_sample(logits, uniforms, rows, None, None, mode, idx, audio, probs, B, Q, T, None)
        return rc, lib.vqw_last_error().decode()

    def rows(t=1.0, k=0, p=1.0):
        s = (L.ArSampling * 1)()
        s[0].temperature, s[0].top_k, s[0].top_p = t, k, p
        return s

    for kw, text in [
        (dict(logits=None), 'null pointer'), (dict(idx=None), 'null pointer'),
        (dict(B=0), 'bad shape'), (dict(T=0), 'bad shape'), (dict(B=-1), 'bad shape'),
        (dict(Q=0), 'multiple of 4'), (dict(Q=1028), 'at most 1024'), (dict(Q=6), 'multiple of 4'), (dict(Q=2048), 'at most 1024'),
        (dict(mode=2), 'mode 2'), (dict(mode=-1), 'mode -1'),
        (dict(uniforms=None), 'needs uniforms'),
        (dict(mode=0, rows=rows(t=0.5)), 'mode 1 (sample) only'), (dict(mode=0, rows=rows(k=3)), 'mode 1 (sample) only'),
        (dict(mode=0, rows=rows(p=0.9)), 'mode 1 (sample) only'),
        (dict(rows=rows(t=0.0)), 'temperature'), (dict(rows=rows(k=-1)), 'top_k'), (dict(rows=rows(p=1.5)), 'top_p'),
        (dict(audio=one, Q=512), 'audio'), (dict(audio=one, Q=128, mode=0), 'audio'),
    ]:
        rc, msg = call(**kw)
        assert rc != 0 and text in msg, (kw, rc, msg)


def test_wrapper_refuses_cpu_tensors_and_bad_settings(pkg):
    import torch
    K = pkg.kernels
    z = torch.zeros(1, 8, 64)
    with pytest.raises(ValueError, match='GPU'):
        K.softmax_sample(z, mode='greedy')
    with pytest.raises(ValueError, match='GPU'):
        K.softmax_sample(z, uniforms=torch.zeros(1, 64))
    with pytest.raises(ValueError, match='mode'):
        K.softmax_sample(z, mode='beam')
    with pytest.raises(ValueError, match='sample'):
        K.softmax_sample(z, mode='greedy', top_k=3)
    with pytest.raises(ValueError, match='top_p'):
        K.softmax_sample(z, top_p=0.0)
    with pytest.raises(ValueError, match='batch of 1'):
        K.softmax_sample(z, temperature=[1.0, 0.5])


# ------------------------------------------------------------------ command lines
def run(script, flags, cwd):
    return subprocess.run([sys.executable, os.path.join(ROOT, script)] + flags, cwd=str(cwd), capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize('flags, match', [
    (['-audio', 'none.wav', '-prior', 'prior-1.pt'], '-teacher_forced'),
    (['-audio', 'none.wav', '-prompt_samples', '64'], '-teacher_forced'),
    (['-audio', 'none.wav', '-prior', 'prior-1.pt', '-prompt_frames', '2'], '-teacher_forced'),
    ([], 'needs -audio'),
    (['-audio', 'none.wav', '-mode', 'greedy', '-top_k', '5'], 'sample'),
])
def test_generate_refuses_teacher_forced_combinations(tmp_path, flags, match):
    out = run('generate.py', ['-restore', str(tmp_path / 'nowhere-1.pt'), '-speakers', 'p225', '-teacher_forced'] + flags, tmp_path)
    assert out.returncode != 0
    assert match in out.stderr, out.stderr[-2000:]
    assert 'Traceback' not in out.stderr, out.stderr[-2000:]      # refused by the parser, not by a failing load


@pytest.mark.parametrize('flags, match', [
    (['-audio_interval', '2'], '-audio_interval needs -eval_list'),
    (['-audio_interval', '-1'], '-audio_interval'),
    (['-audio_interval', '2', '-audio_count', '0'], '-audio_count'),
])
def test_train_refuses_audio_flags(tmp_path, flags, match):
    out = run('train.py', ['-dataset', 'synthetic', '-step', '1', '-params', str(tmp_path / 'nowhere.json')] + flags, tmp_path)
    assert out.returncode != 0
    assert match in out.stderr, out.stderr[-2000:]
    assert 'Traceback' not in out.stderr, out.stderr[-2000:]


def test_help_lists_the_flags():
    assert '-teacher_forced' in subprocess.check_output([sys.executable, os.path.join(ROOT, 'generate.py'), '-h'], text=True)
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, 'train.py'), '-h'], text=True)
    for f in ('-audio_interval', '-audio_count', '-audio_dir'):
        assert f in out


# ------------------------------------------------------------------ the restatement over a tensor
def test_recon_ref_agrees_with_sampling_ref():
    g = np.random.RandomState(3)
    B, Q, T = 3, 8, 6
    z = (g.randn(B, Q, T) * 2).astype(np.float32)
    z[0, 2, 1] = z[0, 5, 1] = z[0, :, 1].max() + 1           # a tie at the maximum
    u = g.rand(B, T).astype(np.float32)
    settings = [(1.0, 0, 1.0), (0.7, 3, 1.0), (1.3, 5, 0.8)]
    tb, te = np.array([0, 2, 4]), np.array([T, 5, 4])        # whole, inner, empty
    r = RR.sample_ref(z, u, settings, tb, te)
    assert r['mask'].sum(1).tolist() == [6, 3, 0]
    for b in range(B):
        for t in range(T):
            if not tb[b] <= t < te[b]:
                assert r['idx'][b, t] == -1 and r['last'][b, t] == -1 and not r['probs'][b, t].any() and not r['edge'][b, t]
                continue
            p, keep, q, i = S.restate(z[b, :, t].astype(np.float64), *settings[b], u=float(u[b, t]))
            assert r['idx'][b, t] == i and np.array_equal(r['probs'][b, t], q) and r['last'][b, t] == keep.nonzero()[0][-1]
            assert r['edge'][b, t] == S.fp32_edge(p, keep, q, settings[b][1], settings[b][2], float(u[b, t]))
            assert abs(r['probs'][b, t].sum() - 1) < 1e-12
    # defaults: settings None is every row at (1, 0, 1); without ranges every position is in
    d = RR.sample_ref(z, u)
    assert d['mask'].all() and (d['idx'] >= 0).all()
    assert d['idx'][0].tolist() == r['idx'][0].tolist()
    # greedy: np.argmax, the lower index of the tie; probs is the softmax
    gr = RR.sample_ref(z, None, None, tb, te, mode='greedy')
    assert gr['idx'][0, 1] == 2 and gr['idx'][2].tolist() == [-1] * T
    assert np.array_equal(gr['idx'][0], z[0].argmax(0))
    np.testing.assert_allclose(gr['probs'][0, 3], S.softmax_t(z[0, :, 3], 1.0), rtol=0, atol=1e-15)
    # u = 0 draws the smallest kept index, u = 1 the largest
    lo, hi = RR.sample_ref(z, np.zeros((B, T)), settings), RR.sample_ref(z, np.ones((B, T)), settings)
    assert (lo['idx'][0] == 0).all() and np.array_equal(hi['idx'], hi['last'])
