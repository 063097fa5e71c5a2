"""CPU tests of the mu-law levels 256 / 512 / 1024: the reference wrapper (tests/levels_ref.py), the threshold tables and the
tool that makes them, what the GPU cases would catch, and the C boundary of the new entry points."""
import ctypes
import importlib.util
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import ref_model as M

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import levels_ref as LR  # noqa: E402

R = M.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, 'include', 'vqwave.h')
CSRC = os.path.join(ROOT, 'vq-vae-wavenet_amd', 'csrc')
NEW = ['vqw_mu_law_encode_f32_levels', 'vqw_mu_law_encode_i32_levels', 'vqw_mu_law_decode_f32_levels', 'vqw_wavenet_inputs_levels',
       'vqw_softmax_sample_levels', 'vqw_ar_decode_set_levels', 'vqw_ar_wide_set_levels']


def tool():
    spec = importlib.util.spec_from_file_location('gen_mu_law_table', os.path.join(ROOT, 'tools', 'gen_mu_law_table.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope='module')
def tables():
    """{Q: the Q - 1 thresholds}, computed once by the tool's own bisection."""
    T = tool()
    return {Q: T.thresholds(Q) for Q in LR.LEVELS}


def committed(Q):
    """The thresholds of the committed header of level Q."""
    text = open(os.path.join(CSRC, tool().header_name(Q))).read()
    return np.array([int(v, 16) for v in re.findall(r'0x([0-9A-F]{8})u', text)], dtype=np.uint32).view(np.float32)


def tiny_problem(Q, B=2, T=128, seed=3):
    m, w = gen_tiny()
    w = LR.with_levels(w, Q)
    P = M.init_params(m, w, 10, seed=seed, randomize_all=True)
    x, spk, _ = M.synthetic_batch(B, T, 10, 1234)
    lc = torch.randn(B, T // 64, m['latent_dim'] + m['speaker_embedding'], generator=torch.Generator().manual_seed(1))
    return x, lc, P, w


def gen_tiny():
    import gen_ref
    return gen_ref.tiny_cfg()


# ------------------------------------------------------------------ the reference wrapper
def test_wrapper_at_256_is_the_oracle():
    x, lc, P, w = tiny_problem(256)
    with torch.no_grad():
        a, la = M.wavenet_build(x, lc, P, w)
        b, lb = LR.wavenet_build(x, lc, P, w)
    assert torch.equal(a, b) and torch.equal(la, lb)


def test_wrapper_at_512_forms_512_level_labels_and_restores():
    x, lc, P, w = tiny_problem(512)
    saved = R.mu_law_encode
    with torch.no_grad():
        logits, labels = LR.wavenet_build(x, lc, P, w)
    assert R.mu_law_encode is saved
    assert logits.shape == (x.shape[0] * x.shape[1], 512)
    want = R.mu_law_encode_np(x.numpy().reshape(-1), 512, True)
    assert np.array_equal(labels.numpy(), want) and want.max() > 255
    # the oracle's encoders keep 255 inside at_level(): only wavenet_build is replaced, and only for the context
    col = {}
    with LR.at_level():
        assert M.wavenet_build is LR.wavenet_build
        with torch.no_grad():
            LR.wavenet_build(x, lc, P, w, collect=col)
            mag = R.mu_law_encode(R.shift_right(x))
    assert M.wavenet_build is not LR.wavenet_build
    # (the torch and the numpy form of the oracle's encode agree to rounding; the two levels differ by up to 0.05)
    shifted = R.shift_right(x).numpy()
    assert torch.allclose(mag, torch.from_numpy(R.mu_law_encode_np(shifted, 256)), atol=1e-6, rtol=0)
    assert torch.allclose(col['inputs'], torch.from_numpy(R.mu_law_encode_np(shifted, 512)), atol=1e-6, rtol=0)
    assert float(np.abs(R.mu_law_encode_np(shifted, 256) - R.mu_law_encode_np(shifted, 512)).max()) > 1e-2


def test_wrapper_restores_after_an_exception():
    x, lc, P, w = tiny_problem(512)
    saved, saved_build = R.mu_law_encode, M.wavenet_build
    broken = dict(P)
    del broken['decoder/preprocess/kernel']
    with pytest.raises(KeyError):
        with LR.at_level():
            LR.wavenet_build(x, lc, broken, w)
    assert R.mu_law_encode is saved and M.wavenet_build is saved_build


# ------------------------------------------------------------------ the tables
def test_tool_regenerates_the_three_headers_byte_for_byte(tables, tmp_path):
    T = tool()
    for Q in LR.LEVELS:
        want = open(os.path.join(CSRC, T.header_name(Q))).read()
        assert T.header_text(tables[Q], Q) == want, 'the committed %s is not what the tool writes' % T.header_name(Q)
    assert T.header_name(256) == 'mu_law_table.h' and T.macro_name(256) == 'VQW_MU_LAW_THR_BITS_LIST'
    out = tmp_path / 'h.h'                                  # the command line itself, without --levels: the 256 header
    subprocess.check_call([sys.executable, os.path.join(ROOT, 'tools', 'gen_mu_law_table.py'), '-o', str(out)])
    assert out.read_bytes() == open(os.path.join(CSRC, 'mu_law_table.h'), 'rb').read()


@pytest.mark.parametrize('Q', LR.LEVELS)
def test_thresholds_against_the_oracle(tables, Q):
    thr = committed(Q)
    assert thr.shape == (Q - 1,) and np.array_equal(thr.view(np.uint32), tables[Q].view(np.uint32))
    assert np.all(np.diff(thr) > 0)
    L = np.arange(1, Q, dtype=np.int32)
    assert np.array_equal(R.mu_law_encode_np(thr, Q, True), L)
    below = np.nextafter(thr, np.float32(-2.0), dtype=np.float32)
    assert np.array_equal(R.mu_law_encode_np(below, Q, True), L - 1)
    rng = np.random.RandomState(Q)
    x = np.concatenate([rng.uniform(-1.2, 1.2, 600000), rng.laplace(0, 0.05, 400000)]).astype(np.float32)
    got = np.searchsorted(thr, np.clip(x, -1, 1), side='right').astype(np.int32)
    assert np.array_equal(got, R.mu_law_encode_np(x, Q, True))
    assert R.mu_law_encode_np(np.float32(-1), Q, True) == 0 and R.mu_law_encode_np(np.float32(1), Q, True) == Q - 1
    dec = R.mu_law_decode_np(np.arange(Q, dtype=np.float32), Q)
    assert len(set(dec.tolist())) == Q
    assert np.array_equal(R.mu_law_encode_np(dec, Q, True), np.arange(Q, dtype=np.int32))


def test_what_the_cases_would_catch(tables):
    """A kernel left at 255 cannot pass a label check at 512, nor one left at 511 a check at 1024: on a speech-like input
    more than half of the labels differ."""
    x = LR.speech(32000)
    lab = {Q: np.searchsorted(tables[Q], x, side='right') for Q in LR.LEVELS}
    for lo, hi in ((256, 512), (512, 1024)):
        share = float((lab[lo] != lab[hi]).mean())
        print('labels at %d levels that differ from the %d-level labels: %.3f' % (hi, lo, share))
        assert share > 0.5


# ------------------------------------------------------------------ the C boundary
def test_new_symbols_are_declared_and_exported(pkg):
    L = pkg._lib
    src = re.sub(r'/\*.*?\*/', '', open(HDR).read(), flags=re.S)
    for name in NEW:
        decl = re.search(r'\bint\s+%s\s*\(([^;]*)\)\s*;' % name, src)
        assert decl, '%s is not declared in vqwave.h' % name
        assert name in L.SIGNATURES, '%s is not declared in _lib.py' % name
        res, args = L.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(decl.group(1).split(','))
        assert hasattr(L.lib(), name)
    assert L.lib().vqw_abi_version() == 1


def test_new_entry_points_refuse_by_name(pkg):
    """Errors are reported, not raised, name the value and come before any device call (there is no device here)."""
    lib = pkg._lib.lib()
    err = lambda: lib.vqw_last_error().decode()                      # noqa: E731
    buf = (ctypes.c_float * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for bad in (0, 255, 300, 2048, -512):
        for name in ('vqw_mu_law_encode_f32_levels', 'vqw_mu_law_encode_i32_levels', 'vqw_mu_law_decode_f32_levels'):
            assert getattr(lib, name)(p, p, 8, bad, None) != 0 and name in err() and 'levels=%d' % bad in err()
        assert lib.vqw_wavenet_inputs_levels(p, p, p, 1, 8, bad, None) != 0 and 'levels=%d' % bad in err()
        assert lib.vqw_softmax_sample_levels(p, None, None, None, None, 0, p, p, None, 1, 512, 1, bad, None) != 0
        assert 'vqw_softmax_sample_levels' in err() and 'levels=%d' % bad in err()
        for name in ('vqw_ar_decode_set_levels', 'vqw_ar_wide_set_levels'):
            assert getattr(lib, name)(None, bad) != 0 and name in err() and 'levels=%d' % bad in err()
    for lv in (256, 512, 1024):
        for name in ('vqw_mu_law_encode_f32_levels', 'vqw_mu_law_encode_i32_levels', 'vqw_mu_law_decode_f32_levels'):
            assert getattr(lib, name)(None, p, 8, lv, None) != 0 and 'null pointer' in err()
            assert getattr(lib, name)(p, None, 8, lv, None) != 0 and 'null pointer' in err()
        assert lib.vqw_wavenet_inputs_levels(None, p, p, 1, 8, lv, None) != 0 and 'null pointer' in err()
        assert lib.vqw_wavenet_inputs_levels(p, None, None, 1, 8, lv, None) != 0 and 'null pointer' in err()
        assert lib.vqw_wavenet_inputs_levels(p, p, p, 0, 8, lv, None) != 0 and 'bad shape' in err()
        assert lib.vqw_softmax_sample_levels(None, None, None, None, None, 0, p, None, None, 1, lv, 1, lv, None) != 0
        assert 'null pointer' in err()
        for name in ('vqw_ar_decode_set_levels', 'vqw_ar_wide_set_levels'):
            assert getattr(lib, name)(None, lv) != 0 and 'null handle' in err()
    # audio is the decode of `levels` classes: another Q is refused and named, by the new entry and (as ever) by the old one
    assert lib.vqw_softmax_sample_levels(p, None, None, None, None, 0, p, p, None, 1, 256, 1, 512, None) != 0
    assert '512 classes (Q=256)' in err()
    assert lib.vqw_softmax_sample(p, None, None, None, None, 0, p, p, None, 1, 512, 1, None) != 0
    assert 'vqw_softmax_sample:' in err() and '256 classes (Q=512)' in err()


def test_ops_accept_the_three_levels_only(pkg):
    x = torch.zeros(4)
    for bad in (300, 255, 128, 2048):
        with pytest.raises(NotImplementedError):
            pkg.ops.mu_law_encode(x, bad)
        with pytest.raises(NotImplementedError):
            pkg.ops.mu_law_encode(x, bad, to_int=True)
        with pytest.raises(NotImplementedError):
            pkg.ops.mu_law_decode(x, bad)
    assert [pkg.ops.mu_law_levels(q) for q in (256, 512, 1024, 64, 300, 768)] == [256, 512, 1024, 256, 256, 256]


def test_model_level_follows_the_config(pkg):
    """WaveNet.levels: Q at 512 and 1024, otherwise 256; the prior has no mu-law whatever its class count."""
    m, w = gen_tiny()
    for Q, want in ((256, 256), (512, 512), (1024, 1024), (128, 256)):
        model = pkg.model.VQVAE(dict(m), LR.with_levels(w, Q), 10, device='cpu', seed=0)
        assert model.levels == want and model.Q == Q
    import launch_trace as LT
    prior = pkg.prior.LatentPrior(dict(LT.PRIOR), LT.SPEAKERS, device='cpu')
    assert prior.Q == 512 and prior.levels == 256
