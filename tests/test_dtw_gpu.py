"""GPU tests of vqw_cepstral_dtw, ops.dtw, scoring.mcd and score_conversion.py: every kernel result bit for bit against the
float32 restatement tests/dtw_ref.py:dtw32 (whose own agreement with a float64 dynamic programme, known answers and power
to tell wrong kernels apart are checked on the CPU in tests/test_dtw_ref_cpu.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dtw_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, 'score_conversion.py')

# scoring.mcd against the float64 pipeline (mfcc64 + dtw64): the worst relative difference of the MCD over the four pairs of
# dtw_ref.mcd_pairs() measured on an MI355X, and the bar at four times that (box-to-box variation of fp32 rounding only)
MCD_REL_MEASURED = 1.122e-7       # per pair: 3.9e-8, 3.9e-8, 1.122e-7, 1.5e-8
MCD_REL_BAR = 4 * MCD_REL_MEASURED


def gpu_dtw(K, a, b, na=None, nb=None, d0=1, D=12):
    """a [P][C][Ta], b [P][C][Tb] numpy -> (cost float32 [P], steps int32 [P]) numpy, through kernels.cepstral_dtw."""
    i32 = lambda n: None if n is None else torch.tensor(n, dtype=torch.int32, device='cuda')      # noqa: E731
    cost, steps = K.cepstral_dtw(torch.from_numpy(np.ascontiguousarray(a)).cuda(), torch.from_numpy(np.ascontiguousarray(b)).cuda(),
                                 na=i32(na), nb=i32(nb), d0=d0, D=D)
    torch.cuda.synchronize()
    return cost.cpu().numpy(), steps.cpu().numpy()


def same_bits(got, want):
    return np.asarray(got, dtype=np.float32).view(np.uint32).tolist() == np.asarray(want, dtype=np.float32).view(np.uint32).tolist()


# ----------------------------------------------------------------------------- single pairs
@pytest.mark.parametrize('case', range(len(R.SHAPES)), ids=['%dx%d' % s for s in R.SHAPES])
def test_single_pair_bit_for_bit(K, case):
    _, a, b = R.random_cases()[case]
    want = R.dtw32(a, b)
    cost, steps = gpu_dtw(K, a[None], b[None])
    assert same_bits(cost, [want[0]]) and steps.tolist() == [want[1]], (cost, steps, want)


@pytest.mark.parametrize('d0,D', [(0, 13), (1, 12), (2, 7), (5, 2), (0, 16)])
def test_channel_windows_on_16_channels(K, d0, D):
    """D = 12 and D = 13 have kernels of their own; every other D takes the general one (four terms at a time, then a tail)."""
    a, b = R.random_cepstra(31, 16, 70), R.random_cepstra(32, 16, 261)
    want = R.dtw32(a, b, d0, D)
    cost, steps = gpu_dtw(K, a[None], b[None], d0=d0, D=D)
    assert same_bits(cost, [want[0]]) and steps.tolist() == [want[1]], (cost, steps, want)


def test_integer_known_answers(K):
    for name, a, b, want_cost, want_steps in R.integer_cases():
        cost, steps = gpu_dtw(K, a[None], b[None])
        assert (float(cost[0]), int(steps[0])) == (want_cost, want_steps), name


def test_lds_bound_4096_frames(K):
    """Ta = Tb = 4096: all 96 KiB of the three diagonals, sixteen strides of the 256 threads on the longest diagonal."""
    a = R.random_cepstra(5, 13, 4096)
    b = R.stretched(a, 4096, 3500, 6)
    want = R.dtw32(a, b)
    assert want[1] > 4096                              # the path leaves the diagonal
    cost, steps = gpu_dtw(K, a[None], b[None])
    assert same_bits(cost, [want[0]]) and steps.tolist() == [want[1]], (cost, steps, want)


# ----------------------------------------------------------------------------- batches
@pytest.fixture(scope='module')
def ragged():
    """70 pairs, Ta = 90, Tb = 83, every pair shorter than that on both sides and NaN from its length on."""
    P, Ta, Tb = 70, 90, 83
    g = np.random.RandomState(77)
    na, nb = g.randint(1, Ta, size=P), g.randint(1, Tb, size=P)
    na[:3], nb[:3] = (1, 1, 89), (1, 82, 1)
    a, b = np.full((P, 13, Ta), np.nan, dtype=np.float32), np.full((P, 13, Tb), np.nan, dtype=np.float32)
    want = []
    for p in range(P):
        a[p, :, :na[p]] = R.random_cepstra(1000 + p, 13, na[p])
        b[p, :, :nb[p]] = R.stretched(a[p, :, :na[p]], nb[p], max(1, na[p] - 3), 2000 + p) if p % 2 else R.random_cepstra(3000 + p, 13, nb[p])
        want.append(R.dtw32(a[p, :, :na[p]], b[p, :, :nb[p]]))
    return a, b, na.tolist(), nb.tolist(), want


def test_ragged_batch_reads_nothing_past_the_lengths(K, ragged):
    a, b, na, nb, want = ragged
    cost, steps = gpu_dtw(K, a, b, na, nb)
    assert np.isfinite(cost).all()
    assert same_bits(cost, [w[0] for w in want])
    assert steps.tolist() == [w[1] for w in want]


def test_batch_independence(K, ragged):
    """Pairs 65..69 of the batch of 70, alone as pairs 0..4 of a batch of five, and one by one: the same bits."""
    a, b, na, nb, _ = ragged
    cost, steps = gpu_dtw(K, a, b, na, nb)
    c5, s5 = gpu_dtw(K, a[65:], b[65:], na[65:], nb[65:])
    assert same_bits(c5, cost[65:]) and s5.tolist() == steps[65:].tolist()
    c1, s1 = gpu_dtw(K, a[67:68], b[67:68], na[67:68], nb[67:68])
    assert same_bits(c1, cost[67:68]) and s1.tolist() == steps[67:68].tolist()


def test_lengths_are_clamped(K):
    a, b = R.random_cepstra(41, 13, 20)[None].repeat(3, 0), R.random_cepstra(42, 13, 30)[None].repeat(3, 0)
    cost, steps = gpu_dtw(K, a, b, [0, -7, 99], [31, 0, 5])
    want = [R.dtw32(a[0][:, :1], b[0]), R.dtw32(a[0][:, :1], b[0][:, :1]), R.dtw32(a[0], b[0][:, :5])]
    assert same_bits(cost, [w[0] for w in want]) and steps.tolist() == [w[1] for w in want]


def test_ops_dtw_takes_what_ops_mfcc_returns(pkg, K):
    """ops.dtw: channels-last [P][T][C], lengths as lists; the same bits as the kernel front end."""
    _, a, b = R.random_cases()[3]
    want = R.dtw32(a[:, :4], b[:, :200])
    at, bt = torch.from_numpy(a.T.copy())[None].cuda(), torch.from_numpy(b.T.copy())[None].cuda()
    cost, steps = pkg.ops.dtw(at, bt, na=[4], nb=[200])
    assert same_bits(cost.cpu().numpy(), [want[0]]) and steps.tolist() == [want[1]]
    full = R.dtw32(a, b, 0, 13)
    cost, steps = pkg.ops.dtw(at, bt, d0=0, D=13)
    assert same_bits(cost.cpu().numpy(), [full[0]]) and steps.tolist() == [full[1]]


# ----------------------------------------------------------------------------- refusals
def test_refusals_by_message(pkg, K):
    a, b = torch.zeros(2, 13, 8, device='cuda'), torch.zeros(2, 13, 9, device='cuda')
    for kw, msg in ((dict(D=0), 'D=0 must be at least 1'), (dict(d0=-1), 'd0=-1 must not be negative'),
                    (dict(d0=2, D=12), r'd0=2 \.\. d0\+D=14 exceed C=13'), (dict(d0=0, D=14), 'exceed C=13')):
        with pytest.raises(RuntimeError, match=msg):
            K.cepstral_dtw(a, b, **kw)
    long = torch.zeros(1, 13, 4097, device='cuda')
    with pytest.raises(RuntimeError, match=r'Ta=4097 must be in 1\.\.4096'):
        K.cepstral_dtw(long, a[:1])
    with pytest.raises(RuntimeError, match=r'Tb=4097 must be in 1\.\.4096'):
        K.cepstral_dtw(a[:1], long)
    L = pkg._lib
    cost, steps = torch.zeros(2, device='cuda'), torch.zeros(2, dtype=torch.int32, device='cuda')
    for args, msg in (((None, L.ptr(b), None, None, L.ptr(cost), L.ptr(steps), 2, 13, 1, 12, 8, 9), 'null pointer'),
                      ((L.ptr(a), L.ptr(b), None, None, L.ptr(cost), None, 2, 13, 1, 12, 8, 9), 'null pointer'),
                      ((L.ptr(a), L.ptr(b), None, None, L.ptr(cost), L.ptr(steps), 0, 13, 1, 12, 8, 9), 'P=0 must be at least 1'),
                      ((L.ptr(a), L.ptr(b), None, None, L.ptr(cost), L.ptr(steps), 2, 13, 1, 12, 0, 9), r'Ta=0 must be in 1\.\.4096')):
        with pytest.raises(RuntimeError, match=msg):
            L.check(L.lib().vqw_cepstral_dtw(*args, L.stream()))
    with pytest.raises(ValueError, match='int32'):
        K.cepstral_dtw(a, b, na=torch.ones(2, device='cuda'))
    with pytest.raises(ValueError, match='at least 2 elements'):
        K.cepstral_dtw(a, b, nb=torch.ones(1, dtype=torch.int32, device='cuda'))
    with pytest.raises(ValueError, match='sample counts'):
        pkg.scoring.mcd(torch.zeros(2, 800, device='cuda'), torch.zeros(2, 800, device='cuda'), nx=[800, 801])


# ----------------------------------------------------------------------------- scoring.mcd
@pytest.fixture(scope='module')
def mcd_batch(pkg):
    """The four pairs zero-padded into one batch, their sample counts and scoring.mcd's result."""
    pairs = R.mcd_pairs()
    nx, ny = [len(x) for x, _ in pairs], [len(y) for _, y in pairs]
    x, y = np.zeros((len(pairs), max(nx)), dtype=np.float32), np.zeros((len(pairs), max(ny)), dtype=np.float32)
    for p, (u, v) in enumerate(pairs):
        x[p, :nx[p]], y[p, :ny[p]] = u, v
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    return pairs, xd, yd, nx, ny, pkg.scoring.mcd(xd, yd, nx, ny)


def test_mcd_of_audio_against_itself_is_zero(pkg, mcd_batch):
    _, xd, _, nx, _, _ = mcd_batch
    r = pkg.scoring.mcd(xd, xd.clone(), nx, nx)
    assert r.mcd.tolist() == [0.0] * 4 and r.cost.tolist() == [0.0] * 4
    assert r.steps.tolist() == r.frames_x.tolist() == r.frames_y.tolist() == [-(-n // 160) for n in nx]


def test_mcd_is_gpu_mfcc_then_dtw32(pkg, mcd_batch):
    """scoring.mcd = ops.mfcc on both sides, the first ceil(n / 160) frames, dtw32 on the host, K cost / steps in float64:
    bit for bit, and a pair scored alone (its own length, no padding) gives the same bits as in the batch."""
    pairs, xd, yd, nx, ny, got = mcd_batch
    cx, cy = pkg.ops.mfcc(xd).cpu().numpy(), pkg.ops.mfcc(yd).cpu().numpy()          # [P][frames][13]
    for p in range(len(pairs)):
        fx, fy = -(-nx[p] // 160), -(-ny[p] // 160)
        cost, steps = R.dtw32(cx[p, :fx].T, cy[p, :fy].T)
        assert (got.frames_x[p], got.frames_y[p], got.steps[p]) == (fx, fy, steps)
        assert same_bits([got.cost[p]], [cost])
        assert got.mcd[p] == R.MCD_K * float(cost) / steps
    alone = pkg.scoring.mcd(torch.from_numpy(pairs[1][0])[None].cuda(), torch.from_numpy(pairs[1][1])[None].cuda())
    assert same_bits(alone.cost, got.cost[1:2]) and alone.steps.tolist() == got.steps[1:2].tolist() and alone.mcd[0] == got.mcd[1]


def test_mcd_against_the_float64_pipeline(mcd_batch):
    """The oracle's MFCC in float64 (dtw_ref.mfcc64) and the float64 dynamic programme with a backtrack: the same path
    length, and the MCD within MCD_REL_BAR relative.  The pairs' float64 paths have tie margins above 2e-4 (asserted), far
    above what fp32 rounding moves an accumulated cost by, so the two pipelines align alike.  Measured on an MI355X: the worst
    relative difference over the four pairs is 1.122e-7 (MCD_REL_MEASURED; the pairs: 3.9e-8, 3.9e-8, 1.122e-7, 1.5e-8); the
    bar is four times that, 4.49e-7."""
    pairs, _, _, _, _, got = mcd_batch
    worst = 0.0
    for p, (x, y) in enumerate(pairs):
        cost, path, steps, margin = R.dtw64(R.mfcc64(x), R.mfcc64(y))
        assert margin > 2e-4, (p, margin)
        want = R.MCD_K * cost / steps
        rel = abs(got.mcd[p] - want) / want
        print('pair %d: mcd %.9f (float64 %.9f) steps %d (%d) relative difference %.3e' % (p, got.mcd[p], want, got.steps[p], steps, rel))
        assert got.steps[p] == steps == len(path)
        worst = max(worst, rel)
    print('worst relative difference %.3e (bar %.3e)' % (worst, MCD_REL_BAR))
    assert worst <= MCD_REL_BAR


# ----------------------------------------------------------------------------- score_conversion.py
def test_cli_round_trip(pkg, tmp_path):
    """Four wavs with VCTK's naming, both forms of the command line as fresh child processes, against scoring.mcd."""
    from scipy.io import wavfile
    from generate import read_wav
    data, conv = tmp_path / 'data' / 'wav48', tmp_path / 'converted'
    pairs = R.mcd_pairs()
    files = [(conv / '7_p225_001_p226.wav', pairs[0][0][:8192]), (data / 'p226' / 'p226_001.wav', pairs[0][1][:9000]),
             (conv / '7_p225_002_p226.wav', pairs[1][0][:6144]), (data / 'p226' / 'p226_002.wav', pairs[1][1][:5000])]
    for path, wav in files:
        os.makedirs(path.parent, exist_ok=True)
        wavfile.write(str(path), 16000, wav)                      # float32, as generate.py writes
    (tmp_path / 'list.txt').write_text('p225/p225_001.wav\np225/p225_002.wav\np225/p225_003.wav\n')
    (tmp_path / 'pairs.txt').write_text(''.join('%s %s\n' % (files[i][0], files[i + 1][0]) for i in (0, 2)))
    wavs = [read_wav(str(path)) for path, _ in files]
    assert [len(w) for w in wavs] == [8192, 8704, 6144, 4608]
    x, y = np.zeros((2, 8192), dtype=np.float32), np.zeros((2, 8704), dtype=np.float32)
    x[0], y[0], x[1, :6144], y[1, :4608] = wavs[0], wavs[1], wavs[2], wavs[3]
    want = pkg.scoring.mcd(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), [8192, 6144], [8704, 4608])
    report = pkg.scoring.mcd_report([want], missing=0)
    forms = (['-pairs', str(tmp_path / 'pairs.txt'), '-per_pair', '-out', str(tmp_path / 'mcd.json')],
             ['-converted_dir', str(conv), '-list', str(tmp_path / 'list.txt'), '-speakers', 'p226', '-step', '7', '-data_root', str(data),
              '-per_pair', '-batch', '1'])
    for n, argv in enumerate(forms):
        r = subprocess.run([sys.executable, CLI] + argv, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        got = json.loads(r.stdout.strip().splitlines()[-1])
        rows = got.pop('per_pair')
        assert got == dict(report, missing=n)                     # the second form finds no p226_003.wav
        assert [row['converted'] for row in rows] == [str(files[0][0]), str(files[2][0])]
        assert [row['target'] for row in rows] == [str(files[1][0]), str(files[3][0])]
        assert [row['mcd'] for row in rows] == want.mcd.tolist() and [row['steps'] for row in rows] == want.steps.tolist()
        assert [row['frames_y'] for row in rows] == [55, 29]
    assert json.loads((tmp_path / 'mcd.json').read_text())['pairs'] == 2
