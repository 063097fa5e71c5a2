"""CPU tests of the DTW / MCD references (tests/dtw_ref.py), of the library's refusals (which come before any device call)
and of score_conversion.py's checks and pair-building rule (a subprocess, no GPU)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import dtw_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, 'score_conversion.py')


# ----------------------------------------------------------------------------- dtw32 against dtw64
@pytest.mark.parametrize('d0,D', [(1, 12), (0, 13)])
def test_dtw32_follows_the_float64_path(d0, D):
    """Same path length, and the cost within the rounding of the float32 operations along ONE path: a local cost carries
    at most (D + 2) / 2 + 1 <= 9 half-ulps (sub 1, square 2, D - 1 adds, sqrt halves them and adds 1) and the N - 1
    accumulating adds one each, so |cost32 - cost64| <= (N + 16) 2^-24 cost64.  That holds only if both take the same path:
    the inputs are chosen so that no cell ON the float64 path has its two best predecessors within 1e-5 relative, which is
    asserted first: a changed seed cannot turn a tie-break difference into a tolerance question."""
    for name, a, b in R.random_cases():
        c64, path, n64, margin = R.dtw64(a, b, d0, D)
        assert margin > 1e-5, (name, margin)
        c32, n32 = R.dtw32(a, b, d0, D)
        assert c32.dtype == np.float32
        assert n32 == n64 == len(path), name
        assert path[0] == (0, 0) and path[-1] == (a.shape[1] - 1, b.shape[1] - 1)
        assert all(0 <= i1 - i0 <= 1 and 0 <= j1 - j0 <= 1 and (i1, j1) != (i0, j0) for (i0, j0), (i1, j1) in zip(path, path[1:]))
        assert abs(float(c32) - c64) <= (n64 + 16) * 2.0 ** -24 * c64, (name, float(c32), c64)


def test_integer_known_answers():
    for name, a, b, cost, steps in R.integer_cases():
        c32, n32 = R.dtw32(a, b)
        assert (float(c32), n32) == (cost, steps), name
        c64, _, n64, _ = R.dtw64(a, b)
        assert (c64, n64) == (cost, steps), name


def test_single_frame_is_the_plain_sum():
    name, a, b = R.random_cases()[1]                 # 1 x 7
    c = R.local_cost32(a, b, 1, 12)[0]
    want = c[0]
    for v in c[1:]:
        want = np.float32(want + v)
    assert R.dtw32(a, b) == (want, 7)
    assert R.dtw32(b, a) == (want, 7)


def test_the_cases_catch_wrong_kernels():
    """Every plausible wrong kernel differs from dtw32 on at least one of the inputs the GPU cases use."""
    cases = [(a, b) for _, a, b in R.random_cases()] + [(a, b) for _, a, b, _, _ in R.integer_cases()]
    want = [R.dtw32(a, b) for a, b in cases]
    variants = {'tie order (i-1,j) first': dict(order=(1, 0, 2)), 'tie order (i,j-1) first': dict(order=(2, 1, 0)),
                '<= for <': dict(strict=False), 'no boundary': dict(boundary=False), 'c0 included': dict(d0=0, D=13)}
    for what, kw in variants.items():
        caught = [n for n, ((a, b), w) in enumerate(zip(cases, want)) if R.dtw32(a, b, **kw) != w]
        assert caught, 'no case tells a kernel with %s from the contract' % what


def test_mfcc64_is_the_oracle_mfcc():
    import torch
    from oracle import ref_ops
    x = R.band_limited_audio(3, 4000)
    want = ref_ops.mfcc(torch.from_numpy(x)[None])[0].numpy().T          # float32 [13][frames]
    got = R.mfcc64(x)
    assert got.shape == want.shape == (13, 25)
    assert np.abs(got - want).max() < 2e-4 * max(1.0, np.abs(want).max())


# ----------------------------------------------------------------------------- the library's refusals
def test_refusals_name_the_value(pkg):
    L = pkg._lib
    lib = L.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def refused(*shape, a=p, b=p, cost=p, steps=p):
        assert lib.vqw_cepstral_dtw(a, b, None, None, cost, steps, *shape, None) != 0
        return lib.vqw_last_error().decode()
    assert 'null pointer' in refused(1, 13, 1, 12, 4, 4, a=None)
    assert 'null pointer' in refused(1, 13, 1, 12, 4, 4, b=None)
    assert 'null pointer' in refused(1, 13, 1, 12, 4, 4, cost=None)
    assert 'null pointer' in refused(1, 13, 1, 12, 4, 4, steps=None)
    assert 'P=0' in refused(0, 13, 1, 12, 4, 4)
    assert 'D=0' in refused(1, 13, 1, 0, 4, 4)
    assert 'd0=-1' in refused(1, 13, -1, 12, 4, 4)
    assert 'd0=2' in refused(1, 13, 2, 12, 4, 4) and 'C=13' in lib.vqw_last_error().decode()
    assert 'Ta=0' in refused(1, 13, 1, 12, 0, 4)
    assert 'Ta=4097' in refused(1, 13, 1, 12, 4097, 4)
    assert 'Tb=0' in refused(1, 13, 1, 12, 4, 0)
    assert 'Tb=4097' in refused(1, 13, 1, 12, 4, 4097)


def test_front_end_refuses_cpu_tensors(pkg):
    import torch
    with pytest.raises(ValueError, match='GPU'):
        pkg.kernels.cepstral_dtw(torch.zeros(1, 13, 4), torch.zeros(1, 13, 4))
    with pytest.raises(ValueError, match='same P and C'):
        pkg.kernels.cepstral_dtw(torch.zeros(1, 13, 4), torch.zeros(2, 13, 4))
    assert pkg.scoring.frames_of(1) == 1 and pkg.scoring.frames_of(160) == 1 and pkg.scoring.frames_of(161) == 2
    assert abs(pkg.scoring.MCD_K - 6.141851463713754) < 1e-12


# ----------------------------------------------------------------------------- score_conversion.py, no GPU
def run_cli(*argv):
    env = dict(os.environ, HIP_VISIBLE_DEVICES='', CUDA_VISIBLE_DEVICES='')
    return subprocess.run([sys.executable, CLI] + [str(a) for a in argv], capture_output=True, text=True, timeout=120, env=env)


def write_wav(path, n, seed=0, sr=16000):
    from scipy.io import wavfile
    os.makedirs(os.path.dirname(path), exist_ok=True)
    wavfile.write(str(path), sr, (R.band_limited_audio(seed, n) * 32767).astype(np.int16))


@pytest.fixture(scope='module')
def corpus(tmp_path_factory):
    """data/p225/p225_001.wav, p225_002.wav; p226 has sentence 001 only; p227 lies flat beside the list's second source."""
    root = tmp_path_factory.mktemp('mcd')
    data, conv = root / 'data', root / 'converted'
    write_wav(data / 'p225' / 'p225_001.wav', 2048, 1)
    write_wav(data / 'p225' / 'p225_002.wav', 2560, 2)
    write_wav(data / 'p226' / 'p226_001.wav', 3072, 3)
    write_wav(data / 'p225' / 'p227_002.wav', 2048, 4)
    for name in ('7_p225_001_p226', '7_p225_001_p227', '7_p225_002_p226', '7_p225_002_p227'):
        write_wav(conv / (name + '.wav'), 2048, 5)
    (root / 'list.txt').write_text('# held out\np225/p225_001.wav\n\np225/p225_002.wav\n')
    return root


def test_cli_refuses_both_or_neither(corpus):
    r = run_cli()
    assert r.returncode == 2 and 'exactly one of -pairs and -converted_dir (got neither)' in r.stderr
    r = run_cli('-pairs', corpus / 'list.txt', '-converted_dir', corpus / 'converted')
    assert r.returncode == 2 and '(got both)' in r.stderr
    r = run_cli('-converted_dir', corpus / 'converted', '-list', corpus / 'list.txt')
    assert r.returncode == 2 and 'needs -list, -speakers and -step' in r.stderr
    r = run_cli('-pairs', corpus / 'nothing.txt')
    assert r.returncode == 2 and 'no such file' in r.stderr


def test_cli_builds_pairs_by_the_vctk_rule(corpus):
    data, conv = corpus / 'data', corpus / 'converted'
    r = run_cli('-converted_dir', conv, '-list', corpus / 'list.txt', '-speakers', 'p226', 'p227', '-step', 7, '-data_root', data, '-dry_run')
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout)
    # p226 has no sentence 002, p227 no sentence 001: two of the four are missing; p226 is found in ../p226/, p227 beside the source
    assert got['missing'] == 2
    assert got['pairs'] == [[str(conv / '7_p225_001_p226.wav'), str(data / 'p226' / 'p226_001.wav')],
                            [str(conv / '7_p225_002_p227.wav'), str(data / 'p225' / 'p227_002.wav')]]
    assert got['frames'] == [[13, 20], [13, 13]]                       # 2048 and 3072 samples (3072 -> 19.2 frames)
    r = run_cli('-converted_dir', conv, '-list', corpus / 'list.txt', '-speakers', 'p300', '-step', 7, '-data_root', data, '-dry_run')
    assert r.returncode == 2 and 'no pair to score (2 without a target recording)' in r.stderr
    r = run_cli('-converted_dir', conv, '-list', corpus / 'list.txt', '-speakers', 'p226', '-step', 8, '-data_root', data, '-dry_run')
    assert r.returncode == 2 and '8_p225_001_p226.wav: no such file' in r.stderr


def test_cli_refuses_a_long_file_by_name(corpus):
    long_wav = corpus / 'data' / 'long' / 'p300_001.wav'
    write_wav(long_wav, 4097 * 160 + 512, 6)
    pairs = corpus / 'pairs.txt'
    pairs.write_text('converted/7_p225_001_p226.wav data/p226/p226_001.wav\nconverted/7_p225_001_p227.wav data/long/p300_001.wav\n')
    r = run_cli('-pairs', pairs, '-data_root', corpus)
    assert r.returncode == 2 and 'p300_001.wav has 4100 frames' in r.stderr and 'at most 4096 frames' in r.stderr
    pairs.write_text('converted/7_p225_001_p226.wav\n')
    r = run_cli('-pairs', pairs, '-data_root', corpus)
    assert r.returncode == 2 and 'line 1' in r.stderr
