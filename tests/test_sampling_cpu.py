"""CPU tests of temperature / top-k / top-p sampling: the generators' validation helper (generator.sampling_settings), the
CLI's refusal of bad flags, the C layout and error returns of the vqw_ar_sampling entry points, and the float64
restatement (sampling_ref.py) that the GPU tests hold the kernels to, checked on hand-made distributions."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampling_ref as S  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ validation helper
def test_settings_accept_and_default(pkg):
    f = pkg.generator.sampling_settings
    assert f(3, 'sample') is None
    assert f(3, 'greedy') is None
    assert f(2, 'greedy', 1.0, 0, 1.0) is None
    assert f(2, 'sample', [1, 1.0], [0, 0], [1, 1.0]) is None
    assert f(2, 'sample', 0.7) == [(0.7, 0, 1.0), (0.7, 0, 1.0)]
    assert f(1, 'sample', 1.0, 50, 0.9) == [(1.0, 50, 0.9)]
    assert f(1, 'sample', top_k=100000) == [(1.0, 100000, 1.0)]          # K >= Q is "off" in the kernels
    assert f(1, 'sample', top_p=1e-6) == [(1.0, 0, 1e-6)]
    assert f(1, 'sample', temperature=1e-3, top_k=np.int64(3), top_p=np.float32(0.5)) == [(1e-3, 3, 0.5)]


def test_settings_broadcast_per_row(pkg):
    import torch
    f = pkg.generator.sampling_settings
    got = f(3, 'sample', temperature=[1.0, 0.5, 2.0], top_k=7, top_p=(1.0, 0.9, 0.8))
    assert got == [(1.0, 7, 1.0), (0.5, 7, 0.9), (2.0, 7, 0.8)]
    got = f(2, 'sample', temperature=torch.tensor([1.0, 0.25]), top_k=np.array([0, 3]))
    assert got == [(1.0, 0, 1.0), (0.25, 3, 1.0)]
    assert all(isinstance(t, float) and isinstance(k, int) for t, k, _ in got)


@pytest.mark.parametrize('kw, match', [
    (dict(temperature=0.0), 'temperature'), (dict(temperature=-1.0), 'temperature'),
    (dict(temperature=math.inf), 'temperature'), (dict(temperature=math.nan), 'temperature'),
    (dict(temperature='1'), 'temperature'),
    (dict(top_k=-1), 'top_k'), (dict(top_k=2.5), 'top_k'),
    (dict(top_p=0.0), 'top_p'), (dict(top_p=1.5), 'top_p'), (dict(top_p=-0.1), 'top_p'), (dict(top_p=math.nan), 'top_p'),
    (dict(temperature=[1.0, 1.0, 1.0]), 'batch of 2'), (dict(top_k=[1]), 'batch of 2'), (dict(top_p=[]), 'batch of 2'),
    (dict(temperature=[1.0, 0.0]), 'temperature'),
])
def test_settings_refuse(pkg, kw, match):
    with pytest.raises(ValueError, match=match):
        pkg.generator.sampling_settings(2, 'sample', **kw)


@pytest.mark.parametrize('kw', [dict(temperature=0.5), dict(top_k=1), dict(top_p=0.9), dict(top_k=[0, 5])])
def test_settings_refuse_non_defaults_with_greedy(pkg, kw):
    with pytest.raises(ValueError, match='sample'):
        pkg.generator.sampling_settings(2, 'greedy', **kw)


# ------------------------------------------------------------------ CLI
@pytest.mark.parametrize('flags, match', [
    (['-temperature', '0'], 'temperature'), (['-top_k', '-1'], 'top_k'), (['-top_p', '1.5'], 'top_p'),
    (['-prior_temperature', '-2'], 'temperature'), (['-prior_top_p', '0'], 'top_p'), (['-prior_top_k', '-3'], 'top_k'),
    (['-mode', 'greedy', '-top_k', '5'], 'sample'),
])
def test_generate_refuses_bad_flags_before_building(tmp_path, flags, match):
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'generate.py'), '-restore', str(tmp_path / 'nowhere-1.pt'),
                          '-audio', str(tmp_path / 'none.wav'), '-speakers', 'p225'] + flags,
                         cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert out.returncode != 0
    assert match in out.stderr, out.stderr[-2000:]
    assert 'Traceback' not in out.stderr, out.stderr[-2000:]      # refused by the parser, not by a failing load


def test_generate_help_lists_sampling_flags():
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, 'generate.py'), '-h'], text=True)
    for f in ('-temperature', '-top_k', '-top_p', '-prior_temperature', '-prior_top_k', '-prior_top_p'):
        assert f in out


# ------------------------------------------------------------------ C ABI
def test_sampling_struct_matches_c_layout(pkg, tmp_path):
    L = pkg._lib
    prog = tmp_path / 'sz.c'
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vqwave.h"\nint main(){printf("%zu %zu %zu %zu\\n",'
                    'sizeof(vqw_ar_sampling), offsetof(vqw_ar_sampling, temperature), offsetof(vqw_ar_sampling, top_k),'
                    'offsetof(vqw_ar_sampling, top_p));return 0;}\n')
    exe = tmp_path / 'sz'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(prog), '-o', str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(L.ArSampling), L.ArSampling.temperature.offset, L.ArSampling.top_k.offset,
                   L.ArSampling.top_p.offset]


def test_sampled_entry_points_report_errors(pkg):
    L = pkg._lib
    lib = L.lib()
    s = (L.ArSampling * 1)()
    s[0].temperature, s[0].top_k, s[0].top_p = 0.5, 3, 0.9
    assert lib.vqw_ar_decode_run_sampled_async(None, None, 1, 64, 1, 1, None, s, None, None, None, None) != 0
    assert b'null' in lib.vqw_last_error()
    assert lib.vqw_ar_decode_run_group_sampled_async(None, 1, None, 1, 64, 1, 1, None, None, None, None, None, None) != 0
    assert b'null' in lib.vqw_last_error()


# ------------------------------------------------------------------ the restatement (steps 2-4) on hand-made distributions
def test_kept_set_top_k_ties_go_to_the_lower_index():
    p = np.array([0.1, 0.3, 0.3, 0.2, 0.1])
    assert S.kept_set(p, 1).nonzero()[0].tolist() == [1]                  # K = 1: argmax, first maximum
    assert S.kept_set(p, 2).nonzero()[0].tolist() == [1, 2]
    assert S.kept_set(p, 3).nonzero()[0].tolist() == [1, 2, 3]
    assert S.kept_set(p, 4).nonzero()[0].tolist() == [0, 1, 2, 3]         # the tie at 0.1: index 0 before 4
    for k in (0, 5, 6, 1000):                                              # off
        assert S.kept_set(p, k).all()
    z = np.log(np.array([0.2, 0.5, 0.5, 0.1]))
    for _ in range(3):
        _, keep, q, idx = S.restate(z, top_k=1, u=0.3)
        assert keep.nonzero()[0].tolist() == [1] and idx == 1 and q[1] == 1.0


def test_kept_set_top_p():
    p = np.array([0.25, 0.25, 0.5])
    assert S.kept_set(p, 0, 1.0).all()                                     # P = 1: off
    assert S.kept_set(p, 0, 0.5).nonzero()[0].tolist() == [2]              # reached exactly by the first class
    assert S.kept_set(p, 0, 0.75).nonzero()[0].tolist() == [0, 2]          # reached exactly, the tie goes to index 0
    assert S.kept_set(p, 0, 0.76).all()
    assert S.kept_set(p, 0, 1e-9).nonzero()[0].tolist() == [2]             # at least one class
    flat = np.full(5, 0.2)
    assert S.kept_set(flat, 0, 0.5).nonzero()[0].tolist() == [0, 1, 2]     # ties at the cut: lower indices first
    assert S.kept_set(flat, 0, 0.4).nonzero()[0].tolist() == [0, 1]


def test_kept_set_top_k_then_top_p_renormalised():
    p = np.array([0.1, 0.3, 0.3, 0.2, 0.1])
    # top-3 = {1, 2, 3}, mass 0.8 -> 0.375, 0.375, 0.25: P = 0.7 keeps {1, 2}, P = 0.37 keeps {1}
    assert S.kept_set(p, 3, 0.7).nonzero()[0].tolist() == [1, 2]
    assert S.kept_set(p, 3, 0.37).nonzero()[0].tolist() == [1]
    assert S.kept_set(p, 3, 0.8).nonzero()[0].tolist() == [1, 2, 3]
    assert S.kept_set(p, 1, 0.1).nonzero()[0].tolist() == [1]


def test_draw_in_ascending_index_order():
    p = np.array([0.1, 0.3, 0.3, 0.2, 0.1])
    keep = S.kept_set(p, 3)                                                # {1, 2, 3}: q = 0.375, 0.375, 0.25
    q = np.where(keep, p, 0.0) / p[keep].sum()
    assert S.draw(q, keep, 0.0) == 1                                       # the smallest kept index
    assert S.draw(q, keep, 0.37) == 1
    assert S.draw(q, keep, 0.3751) == 2
    assert S.draw(q, keep, 0.74) == 2
    assert S.draw(q, keep, 0.9) == 3
    assert S.draw(q, keep, 1.0) == 3
    assert S.draw(q, keep, 2.0) == 3                                       # above the last cdf value: the largest kept
    exact = np.array([0.25, 0.25, 0.5])                                    # side 'left': cdf == u stops there
    assert [S.draw(exact, np.ones(3, bool), u) for u in (0.25, 0.5, 0.5000001, 1.0)] == [0, 1, 2, 2]
    # with nothing truncated the draw is searchsorted(cumsum(p), u, 'left') of utils.py:20-25
    for u in np.linspace(0.01, 0.99, 37):
        assert S.draw(p, np.ones(5, bool), u) == int(np.searchsorted(np.cumsum(p), u, 'left'))


def test_temperature_sharpens_and_flattens():
    z = np.array([1.0, 2.0, 0.5, 2.0])
    p1, _, _, _ = S.restate(z)
    np.testing.assert_allclose(p1, np.exp(z - 2.0) / np.exp(z - 2.0).sum())
    cold, _, _, i = S.restate(z, temperature=0.05, u=0.49)
    assert cold[1] > 0.49 and cold[3] > 0.49 and i == 1
    hot, _, _, _ = S.restate(z, temperature=100.0)
    assert hot.max() - hot.min() < 0.01
