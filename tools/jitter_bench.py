#!/usr/bin/env python3
"""Cost of the time-jitter regulariser on one GPU at bench.py's shape (B = 8, T = 6656, reference widths).

  * the two kernels alone at the step's latent shape (z_q [8][64][104] into / out of the first 64 rows of the [8][Cc][104]
    condition buffers, 213 KB): HIP events around windows of `--iters` launches, the median of 5 windows, in us;
  * ms per training step (deferred range guard, as train.py runs it) with time_jitter 0 and `--p` (0.12): `--rounds` rounds
    that run the two modes one after another, `--steps` steps each, host clock around the steps + finish_steps + a device
    synchronise; median, min and max over the rounds, and the share of frames that moved in the last step.
One JSON line each.

    python tools/jitter_bench.py [--steps 20] [--rounds 3] [--iters 200] [--p 0.12]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--p', type=float, default=0.12)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--length', type=int, default=6656)
    args = ap.parse_args()
    import torch
    import bench
    from clip_bench import median_ms
    if not torch.cuda.is_available():
        raise SystemExit('jitter_bench.py needs a GPU')
    pkg = importlib.import_module('vq-vae-wavenet_amd')
    K = pkg.kernels
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    m, w = bench.default_configs()
    model = pkg.model.VQVAE(m, w, 109, device=dev, seed=0)
    model.defer_guard = True
    x, spk = bench.synthetic_batch(args.batch, args.length, 109, 1234, dev)
    emit = lambda **kw: print(json.dumps(kw), flush=True)  # noqa: E731

    B, D, Cc, Tz = args.batch, model.D, model.Cc, args.length // 64
    zq, dzq = torch.randn(B, D, Tz, device=dev), torch.empty(B, D, Tz, device=dev)
    cond, dcond = torch.zeros(B, Cc, Tz, device=dev), torch.randn(B, Cc, Tz, device=dev)
    u, src = torch.rand(B, Tz, device=dev), torch.zeros(B, Tz, dtype=torch.int32, device=dev)
    f = median_ms(lambda i: K.time_jitter_fwd(zq, u, cond, src, p=args.p, D=D, out_bstride=Cc * Tz), args.iters)
    b = median_ms(lambda i: K.time_jitter_bwd(dcond, src, dzq, D=D, dout_bstride=Cc * Tz), args.iters)
    g = median_ms(lambda i: model.jitter_uniforms(B, Tz, i), args.iters)
    kb = 4e-3 * B * D * Tz
    for what, r in (('vqw_time_jitter_fwd', f), ('vqw_time_jitter_bwd', b), ('jitter_uniforms (seed + torch.rand)', g)):
        emit(what=what, us=1e3 * r[0], min=1e3 * r[1], max=1e3 * r[2], B=B, D=D, Tz=Tz, KB=kb, iters=args.iters)

    def steps(n):
        t0 = time.perf_counter()
        for _ in range(n):
            ws = model.train_step(x, spk)
        model.finish_steps()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n, ws

    modes = [('off', 0.0), ('on', args.p)]
    for _, p in modes:                           # workspaces, guard scales, the jitter buffers
        model.time_jitter = p
        steps(4)
    ms, moved = {name: [] for name, _ in modes}, {}
    for _ in range(args.rounds):
        for name, p in modes:
            model.time_jitter = p
            t, ws = steps(args.steps)
            ms[name].append(t)
            moved[name] = model.jitter_moved(ws)
    for name, p in modes:
        emit(what='train step, time_jitter %s' % name, time_jitter=p, ms_per_step=statistics.median(ms[name]), min=min(ms[name]),
             max=max(ms[name]), rounds=args.rounds, steps=args.steps, jitter_moved=moved[name], x3_fallbacks=model.x3_fallbacks)


if __name__ == '__main__':
    main()
