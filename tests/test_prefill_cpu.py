"""CPU tests of prompted generation (prefill): the window arithmetic of model.prefill_window, the generators' argument checks,
the C entry points' argument checks and generate.py's prompt flags (refused before anything is loaded)."""
import ctypes
import json
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cfg(name):
    with open(os.path.join(ROOT, name)) as f:
        return json.load(f)


# ------------------------------------------------------------------ window arithmetic
def test_window_at_reference_and_prior_widths(pkg):
    pw = pkg.model.prefill_window
    w = cfg('wavenet_parameters.json')
    ks, dil, pre_k = w['kernel_size'], w['dilation_rates'], w['preprocess']['kernel_size']
    assert pw(0, ks, dil, pre_k, 64) == (6170, 0, 0)
    p = cfg('prior_parameters.json')
    assert pw(0, p['kernel_size'], p['dilation_rates'], p['preprocess']['kernel_size'], 64)[0] == 4093
    W = 6170
    assert pw(1, ks, dil, pre_k, 64) == (W, 0, 64)
    assert pw(3000, ks, dil, pre_k, 64) == (W, 0, 3008)              # T < W: from step 0; the end rounded up to a frame
    assert pw(W, ks, dil, pre_k, 64) == (W, 0, 6208)
    assert pw(W + 63, ks, dil, pre_k, 64) == (W, 0, 6272)            # T - W = 63 rounds down to 0
    assert pw(W + 64, ks, dil, pre_k, 64) == (W, 64, 6272)
    assert pw(48000, ks, dil, pre_k, 64) == (W, 41792, 48000)        # T >> W: the window is capped
    for T in (7000, 48000, 160000, 160001):
        _, s0, end = pw(T, ks, dil, pre_k, 64)
        assert s0 % 64 == 0 and end % 64 == 0 and s0 <= T - W < s0 + 64 and T <= end < T + 64
        assert end - s0 <= W + 127


def test_window_tiny_and_other_ratios(pkg):
    pw = pkg.model.prefill_window
    dil = [1, 2, 4, 8, 1, 2, 4, 8]
    assert pw(0, 3, dil, 32, 64) == (92, 0, 0)
    assert pw(37, 3, dil, 32, 64) == (92, 0, 64)
    assert pw(1000, 3, dil, 32, 64) == (92, 896, 1024)
    assert pw(1000, 3, dil, 32, 1) == (92, 908, 1000)
    assert pw(1000, 2, dil, 32, 160) == (62, 800, 1120)
    for bad in ((-1, 64), (5, 0)):
        with pytest.raises(ValueError):
            pw(bad[0], 3, dil, 32, bad[1])


def test_window_covers_every_state_read(pkg):
    """Restate the dependency cone: layer l's queued steps [T-(ks-1)d_l, T) need layer-0 inputs back to
    T - (ks-1) sum_{j<=l} d_j - (pre_k-1) (one prompt value earlier: the input of step t is a[t-1]).  All of them lie strictly
    after s0, whose input the window's left edge zeroes."""
    pw = pkg.model.prefill_window
    for ks, dil, pre_k, ratio in ((3, [1, 2, 4, 8, 1, 2, 4, 8], 32, 64), (3, [2 ** i for i in range(10)] * 3, 32, 64),
                                  (2, [1, 2, 4], 1, 1), (4, [1, 3, 9], 5, 7)):
        for T in range(0, 400, 7):
            W, s0, end = pw(T, ks, dil, pre_k, ratio)
            oldest_input = T
            for l in range(len(dil)):
                first_step = T - (ks - 1) * sum(dil[:l + 1])            # oldest queued step of layer l, then its inputs
                oldest_input = min(oldest_input, first_step - (pre_k - 1))
            if T > W:
                assert oldest_input > s0, (ks, dil, T)


# ------------------------------------------------------------------ generator argument checks (no GPU needed: refused first)
class _Model:
    Cc, Q, pre_k = 32, 32, 3


def _fast(pkg, cls):
    g = object.__new__(cls)
    g.model, g.B, g._hs, g._parts, g._t = _Model(), 2, [], [2], 0
    return g


@pytest.mark.parametrize('prompt, enc, match', [
    (torch.zeros(2, 10, dtype=torch.float64), torch.zeros(2, 32, 4), 'prompt'),
    (torch.zeros(3, 10), torch.zeros(3, 32, 4), 'prompt'),
    (torch.zeros(10), torch.zeros(2, 32, 4), 'prompt'),
    ([[0.0] * 10] * 2, torch.zeros(2, 32, 4), 'prompt'),
    (torch.zeros(2, 10), torch.zeros(2, 16, 4), 'encoding'),
    (torch.zeros(2, 10), torch.zeros(2, 32, 4, dtype=torch.float16), 'encoding'),
    (torch.zeros(2, 257), torch.zeros(2, 32, 4), 'longer than the encoding'),
    (torch.zeros(2, 10), torch.zeros(2, 32, 4), 'GPU'),
])
def test_fast_generator_refuses_bad_prefill(pkg, prompt, enc, match):
    g = _fast(pkg, pkg.generator.FastGenerator)
    with pytest.raises(ValueError, match=match):
        g.prefill(prompt, enc)


def test_prior_generator_refuses_bad_prefill(pkg):
    g = _fast(pkg, pkg.generator.PriorGenerator)
    spk = torch.zeros(2, dtype=torch.int64)
    for codes in (torch.zeros(2, 5, dtype=torch.int64), torch.zeros(3, 5, dtype=torch.int32), torch.zeros(5, dtype=torch.int32),
                  torch.zeros(2, 5, dtype=torch.int32)):           # the last one: on the CPU
        with pytest.raises(ValueError, match='codes'):
            g.prefill(codes, spk)
    assert g._t == 0


# ------------------------------------------------------------------ C entry points
def test_c_prefill_entry_points_check_arguments(pkg):
    lib = pkg._lib.lib()
    assert lib.vqw_ar_decode_prefill_layer(None, 0, None, 0, 0, 0, None) != 0
    assert b'null handle' in lib.vqw_last_error()
    assert lib.vqw_ar_decode_prefill_finish(None, 0, None, None, None) != 0
    assert b'null handle' in lib.vqw_last_error()
    assert pkg._lib.SIGNATURES['vqw_ar_decode_prefill_layer'][1][1] is ctypes.c_int


# ------------------------------------------------------------------ generate.py flags
@pytest.mark.parametrize('extra, match', [
    (['-audio', 'a.wav', '-prompt_samples', '-1'], '>= 0'),
    (['-audio', 'a.wav', '-prompt_frames', '-2', '-prior', 'p.pt'], '>= 0'),
    (['-prior', 'p.pt', '-prompt_samples', '64'], '-prompt_frames'),
    (['-prior', 'p.pt', '-prompt_frames', '2'], 'needs -prior and -audio'),
    (['-audio', 'a.wav', '-prompt_frames', '2'], 'needs -prior and -audio'),
])
def test_generate_refuses_bad_prompt_flags(tmp_path, extra, match):
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'generate.py'), '-restore', 'none/weights-1.pt', '-speakers', 'p225']
                         + extra, cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and match in out.stderr, out.stderr[-1000:]
