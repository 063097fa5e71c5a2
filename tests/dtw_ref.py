"""References for vqw_cepstral_dtw / scoring.mcd (no GPU needed) and the inputs the CPU and GPU tests share.

dtw32   the contract of include/vqwave.h restated in numpy float32, one rounded operation at a time, diagonal by diagonal:
        what the kernel must reproduce bit for bit.  `order`, `strict`, `boundary` exist to build WRONG variants (a swapped
        tie order, <= for <, predecessors outside the matrix read as (0, 0)) for the test of what the cases catch.
dtw64   the textbook dynamic programme in float64 with a direction matrix and a real backtrack.
mfcc64  the oracle's MFCC (oracle/ref_ops.py: mfcc) with every operation in float64.
"""
import math

import numpy as np

PREDS = ((1, 1), (1, 0), (0, 1))            # (di, dj) of the diagonal, (i-1, j) and (i, j-1) neighbours, in the contract's order
MCD_K = 10.0 * math.sqrt(2.0) / math.log(10.0)


def local_cost32(a, b, d0, D):
    """c(i, j) float32 [Ta][Tb] of cepstra a [C][Ta], b [C][Tb]: sub, mul, add (ascending d from 0.0f) and sqrt, each float32."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    s = np.zeros((a.shape[1], b.shape[1]), dtype=np.float32)
    for d in range(d0, d0 + D):
        x = a[d][:, None] - b[d][None, :]
        s = s + x * x
    assert s.dtype == np.float32
    return np.sqrt(s)


def dtw32(a, b, d0=1, D=12, order=(0, 1, 2), strict=True, boundary=True):
    """-> (cost np.float32, steps int).  a [C][Ta], b [C][Tb]; all frames are compared (slice for shorter lengths)."""
    c = local_cost32(a, b, d0, D)
    Ta, Tb = c.shape
    Dp = np.zeros((Ta, Tb), dtype=np.float32)
    n = np.zeros((Ta, Tb), dtype=np.int32)
    for k in range(Ta + Tb - 1):
        i = np.arange(max(0, k - (Tb - 1)), min(Ta - 1, k) + 1)
        j = k - i
        best = np.zeros(i.size, dtype=np.float32)
        bn = np.zeros(i.size, dtype=np.int32)
        have = np.zeros(i.size, dtype=bool)
        for w in order:
            di, dj = PREDS[w]
            inside = (i >= di) & (j >= dj)
            v = np.where(inside, Dp[i - di, j - dj], np.float32(0.0)).astype(np.float32)
            vn = np.where(inside, n[i - di, j - dj], 0).astype(np.int32)
            exists = inside if boundary else np.ones(i.size, dtype=bool)
            take = exists & (~have | ((v < best) if strict else (v <= best)))
            best, bn = np.where(take, v, best), np.where(take, vn, bn)
            have = have | exists
        Dp[i, j] = np.where(have, c[i, j] + best, c[i, j])
        n[i, j] = np.where(have, bn + 1, 1)
    assert Dp.dtype == np.float32
    return Dp[-1, -1], int(n[-1, -1])


def dtw64(a, b, d0=1, D=12):
    """-> (cost float, path [(i, j)] from (0, 0) to (Ta-1, Tb-1), len(path), margin).  The same step pattern and tie order
    in float64, cell by cell, directions stored and walked back.  margin: over the path's cells with two or more
    predecessors, the smallest (second best - best) / second best of their accumulated costs (inf if there is none)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    x = a[d0:d0 + D, :, None] - b[d0:d0 + D, None, :]
    c = np.sqrt((x * x).sum(axis=0))
    Ta, Tb = c.shape
    Dp = np.full((Ta, Tb), np.inf)
    dirs = np.full((Ta, Tb), -1, dtype=np.int8)
    for i in range(Ta):
        for j in range(Tb):
            best, w = None, -1
            for q, (di, dj) in enumerate(PREDS):
                if i >= di and j >= dj and (best is None or Dp[i - di, j - dj] < best):
                    best, w = Dp[i - di, j - dj], q
            Dp[i, j] = c[i, j] if best is None else c[i, j] + best
            dirs[i, j] = w
    path, i, j, margin = [], Ta - 1, Tb - 1, math.inf
    while True:
        path.append((i, j))
        if dirs[i, j] < 0:
            break
        cands = sorted(Dp[i - di, j - dj] for di, dj in PREDS if i >= di and j >= dj)
        if len(cands) > 1 and cands[1] > 0:
            margin = min(margin, (cands[1] - cands[0]) / cands[1])
        di, dj = PREDS[dirs[i, j]]
        i, j = i - di, j - dj
    assert (i, j) == (0, 0)
    path.reverse()
    return float(Dp[-1, -1]), path, len(path), margin


def mfcc64(wav):
    """oracle/ref_ops.py mfcc (frame 400, step 160, pad_end, periodic hann, |rfft|, 80 mel bins, log(. + 1e-6), DCT-II, the
    first 13) in float64: wav [T] -> [13][ceil(T / 160)], the kernels' (channel, frame) layout."""
    from oracle import ref_ops as R
    wav = np.asarray(wav, dtype=np.float64)
    L, S, M = 400, 160, 80
    frames = -(-wav.size // S)
    xp = np.concatenate([wav, np.zeros(max((frames - 1) * S + L - wav.size, 0))])
    fr = np.stack([xp[f * S:f * S + L] for f in range(frames)])
    window = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(L) / L)
    spec = np.abs(np.fft.rfft(fr * window, n=L))
    feature = np.log(spec @ R.linear_to_mel_weight_matrix(M, spec.shape[-1]).astype(np.float64) + 1e-6)
    basis = np.cos(np.pi * np.arange(M)[None, :] * (2.0 * np.arange(M)[:, None] + 1.0) / (2.0 * M))
    return (2.0 * (feature @ basis) / math.sqrt(2.0 * M))[:, :13].T.copy()


# ----------------------------------------------------------------------------- shared inputs
def random_cepstra(seed, C, T, scale=1.0):
    """A smooth random trajectory, float32 [C][T]: a random walk per coefficient plus noise (neighbouring frames are alike, as
    in speech, so the alignment has real choices to make)."""
    g = np.random.RandomState(seed)
    return (scale * (np.cumsum(g.randn(C, T), axis=1) * 0.5 + g.randn(C, T))).astype(np.float32)


def integer_cepstra(seed, C, T):
    """Integer-valued float32 [C][T] in -8..8 whose consecutive frames differ above c0: every square and sum is exact in fp32."""
    g = np.random.RandomState(seed)
    x = g.randint(-8, 9, size=(C, T))
    for t in range(1, T):
        while (x[1:, t] == x[1:, t - 1]).all():
            x[:, t] = g.randint(-8, 9, size=C)
    return x.astype(np.float32)


SHAPES = ((1, 1), (1, 7), (7, 1), (5, 300), (257, 257), (300, 270))     # the last three: diagonals longer than the 256 threads
SEEDS = (100, 100, 100, 101, 100, 100)      # per shape: the first seed whose float64 path has a tie margin above 1e-4


def random_cases():
    """[(name, a [13][Ta], b [13][Tb])] for SHAPES, seeds fixed (tests/test_dtw_ref_cpu.py checks their tie margins)."""
    return [('%dx%d' % (Ta, Tb), random_cepstra(s, 13, Ta), random_cepstra(s + 1000, 13, Tb)) for s, (Ta, Tb) in zip(SEEDS, SHAPES)]


def integer_cases():
    """[(name, a, b, cost, steps)] with known answers (C = 13, d0 = 1, D = 12)."""
    T = 37
    a = integer_cepstra(7, 13, T)
    flat = np.tile(np.arange(13, dtype=np.float32)[:, None], (1, 300))
    one = integer_cepstra(8, 13, 1)
    many = integer_cepstra(9, 13, 23)
    # integer-valued frames at distances 0, 3, 4 and 5 (3-4-5 in two coefficients): the plain sum is exact
    many[1:] = one[1:]
    many[1] += np.array([0, 3, 0, 3] * 6)[:23]
    many[2] += np.array([0, 0, 4, 4] * 6)[:23]
    plain = float(sum((0, 3, 4, 5)[t % 4] for t in range(23)))
    return [('identical', a, a.copy(), 0.0, T),
            ('doubled', a, np.repeat(a, 2, axis=1), 0.0, 2 * T),
            ('all_equal_300x270', flat, flat[:, :270].copy(), 0.0, 300),
            ('all_equal_5x300', flat[:, :5].copy(), flat, 0.0, 300),
            ('all_equal_257x257', flat[:, :257].copy(), flat[:, :257].copy(), 0.0, 257),
            ('single_frame', one, many, plain, 23)]


def band_limited_audio(seed, n, amplitude=0.1):
    """Random audio float32 [n] at 16 kHz: noise shaped below 4 kHz under a slowly varying envelope (frames differ in level and
    colour) over a white floor 40 dB down.  Without the floor the mel bins above 4 kHz would hold nothing but the rounding
    noise of the fp32 transform, which log(. + 1e-6) turns into cepstral differences no recording has."""
    g = np.random.RandomState(seed)
    spec = np.fft.rfft(g.randn(n))
    f = np.fft.rfftfreq(n, 1.0 / 16000.0)
    spec *= (f < 4000.0) / (1.0 + (f / 800.0) ** 2)
    x = np.fft.irfft(spec, n)
    env = 0.55 + 0.45 * np.sin(2.0 * np.pi * (np.arange(n) / 16000.0 * g.uniform(2.0, 5.0) + g.uniform()))
    x = x / np.abs(x).max() * env + 0.01 * g.randn(n)
    return (amplitude * x).astype(np.float32)


def warped(x, factor, seed, noise=0.002):
    """x played `factor` times as long (linear interpolation) plus a little independent noise: 'the same sentence' by
    another speaker, as far as the alignment is concerned."""
    n = int(round(x.size * factor))
    y = np.interp(np.arange(n) / factor, np.arange(x.size), x.astype(np.float64))
    return (y + noise * np.random.RandomState(seed).randn(n)).astype(np.float32)


# (seed, samples of x, length factor of y): per shape the first seed whose float64 pipeline's path has a tie margin above 2e-4
MCD_PAIRS = ((11, 16000, 1.18), (11, 19200, 0.87), (16, 22400, 1.07), (11, 25600, 0.93))


def mcd_pairs():
    """[(x, y)] float32 audio of different lengths for the scoring.mcd tests."""
    out = []
    for seed, n, factor in MCD_PAIRS:
        x = band_limited_audio(seed, n)
        out.append((x, warped(x, factor, seed + 50)))
    return out


def stretched(a, T, span, seed, noise=0.25):
    """b [C][T]: the first `span` frames of a stretched to T frames (frames repeat) plus noise, so the best path wanders off
    the diagonal and comes back instead of running straight down it."""
    idx = np.floor(np.linspace(0, span - 1, T)).astype(np.int64)
    return (a[:, idx] + noise * np.random.RandomState(seed).randn(a.shape[0], T)).astype(np.float32)
