#!/usr/bin/env python3
"""Conversion scoring timings on one GPU: the alignment alone -- `ops.dtw` (the `vqw_cepstral_dtw` launch and the
two transposes in front of it) and `kernels.cepstral_dtw` (the launch alone) for P = 1, 64 and 256 pairs of 200, 500 and 1000
frames on each side, 12 coefficients -- and `scoring.mcd` end to end (two MFCC launches, the alignment, the copy of the
results to the host) for the same pair counts of 5 s of audio.  HIP events around windows of `--iters` calls; the median
(min .. max) of three rounds.  Per line also the time per anti-diagonal, ms / (2 T - 1): the kernel's cost model is one
barrier per anti-diagonal, so this is the figure that should stay flat over T while the diagonals fit the 256 threads.
One JSON line each, also written to `--out`.

    python tools/mcd_bench.py [--iters 5] [--out profiles/mcd_bench_lines.json]
"""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def rounds_ms(fn, iters, rounds=3, warmup=2):
    """(median, min, max) over `rounds` of (event time of `iters` calls of fn()) / iters, in ms."""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=5, help='calls per timed window')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mcd_bench_lines.json'))
    args = ap.parse_args()
    import torch
    import dtw_ref as R
    pkg = importlib.import_module('vq-vae-wavenet_amd')
    assert torch.cuda.is_available(), 'mcd_bench.py needs a GPU'
    torch.cuda.set_device(0)
    lines = []

    def report(**kw):
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    for T in (200, 500, 1000):
        base = R.random_cepstra(1, 13, T)
        pair = np.stack([base, R.stretched(base, T, T - T // 8, 2)])
        for P in (1, 64, 256):
            # every pair a different shift of the same trajectory: the paths differ, the work per pair does not
            a = torch.from_numpy(np.stack([np.roll(pair[0], p, axis=1) for p in range(P)])).cuda()
            b = torch.from_numpy(np.stack([np.roll(pair[1], 3 * p, axis=1) for p in range(P)])).cuda()
            at, bt = a.transpose(1, 2).contiguous(), b.transpose(1, 2).contiguous()
            steps = None
            for what, fn in (('ops.dtw', lambda: pkg.ops.dtw(at, bt)), ('kernels.cepstral_dtw', lambda: pkg.kernels.cepstral_dtw(a, b))):
                med, lo, hi = rounds_ms(fn, args.iters)
                steps = fn()[1]
                report(what=what, P=P, frames=T, ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4),
                       us_per_pair=round(med * 1e3 / P, 2), us_per_diagonal=round(med * 1e3 / (2 * T - 1), 3),
                       mean_path_steps=round(float(steps.float().mean()), 1), rounds=3, iters=args.iters)
    n = 80000                                                    # 5 s: 500 frames
    x1 = R.band_limited_audio(1, n)
    y1 = R.warped(x1, 1.0, 2)
    for P in (1, 64, 256):
        x = torch.from_numpy(np.stack([np.roll(x1, 160 * p) for p in range(P)])).cuda()
        y = torch.from_numpy(np.stack([np.roll(y1, 480 * p) for p in range(P)])).cuda()
        med, lo, hi = rounds_ms(lambda: pkg.scoring.mcd(x, y), args.iters)
        r = pkg.scoring.mcd(x, y)
        report(what='scoring.mcd', P=P, samples=n, frames=500, ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4),
               us_per_pair=round(med * 1e3 / P, 2), pairs_per_s=round(P / (med * 1e-3), 1), mcd_mean=round(float(r.mcd.mean()), 4),
               rounds=3, iters=args.iters)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(''.join(json.dumps(ln) + '\n' for ln in lines))


if __name__ == '__main__':
    main()
