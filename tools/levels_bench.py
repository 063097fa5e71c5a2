#!/usr/bin/env python3
"""What the mu-law level costs (quantization_channels 256 / 512 / 1024 in wavenet_parameters.json), DESIGN 3.16.

ONE process, one model per level at the reference widths (R 256, S 512, 30 layers):
  (a) ms per training step at bench.py's shape (B = 8, T = 6656, deferred range guard, as train.py runs it): `--rounds`
      rounds that alternate the three levels, `--steps` steps each, host clock around the steps + finish_steps + a device
      synchronise; median, min and max over the rounds.
  (b) the label / input kernel alone (kernels.wavenet_inputs at that shape) per level: HIP events around windows of
      `--iters` launches, the median of 5 windows (tools/clip_bench.median_ms).
  (c) us per step of FastGenerator (1 row, `--fast_steps` steps) and WideGenerator (256 rows, `--wide_steps` steps) per
      level, mode 'sample' with supplied uniforms, host clock around one generate() call plus a device synchronise, rounds
      alternating the levels.
One JSON line per result, printed and written to profiles/levels_bench_lines.json (`--out`).

    python tools/levels_bench.py [--rounds 3] [--steps 10] [--iters 50] [--fast_steps 1536] [--wide_steps 192] [--out FILE]
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
sys.path.insert(0, os.path.join(ROOT, 'tools'))
LEVELS = (256, 512, 1024)
RATIO = 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--fast_steps', type=int, default=1536)
    ap.add_argument('--wide_steps', type=int, default=192)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--length', type=int, default=6656)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'levels_bench_lines.json'))
    args = ap.parse_args()
    import torch
    import bench
    from clip_bench import median_ms
    if not torch.cuda.is_available():
        raise SystemExit('levels_bench.py needs a GPU')
    pkg = importlib.import_module('vq-vae-wavenet_amd')
    K = pkg.kernels
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    lines = []

    def emit(**kw):
        print(json.dumps(kw), flush=True)
        lines.append(kw)

    m, w = bench.default_configs()
    x, spk = bench.synthetic_batch(args.batch, args.length, 109, 1234, dev)
    models = {}
    for Q in LEVELS:
        models[Q] = pkg.model.VQVAE(m, dict(w, quantization_channels=Q), 109, device=dev, seed=0)
        models[Q].defer_guard = True
        assert models[Q].levels == Q

    def steps(model, n):
        t0 = time.perf_counter()
        for _ in range(n):
            ws = model.train_step(x, spk)
        model.finish_steps()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n, ws

    # (a) the training step
    used = {}
    for Q in LEVELS:
        _, ws = steps(models[Q], 5)                # workspaces, guard scales
        used[Q] = bool(ws['x3_used'])
    ms = {Q: [] for Q in LEVELS}
    for _ in range(args.rounds):
        for Q in LEVELS:
            ms[Q].append(steps(models[Q], args.steps)[0])
    for Q in LEVELS:
        emit(what='train step, %d levels' % Q, levels=Q, ms_per_step=statistics.median(ms[Q]), min=min(ms[Q]), max=max(ms[Q]),
             delta_ms_vs_256=statistics.median(ms[Q]) - statistics.median(ms[256]), rounds=args.rounds, steps=args.steps,
             batch=args.batch, length=args.length, x3_used=used[Q], x3_fallbacks=models[Q].x3_fallbacks,
             logits_MB=4e-6 * args.batch * args.length * Q)

    # (b) the label / input kernel alone
    inputs = torch.empty(args.batch, args.length, device=dev)
    labels = torch.empty(args.batch, args.length, dtype=torch.int32, device=dev)
    for Q in LEVELS:
        r = median_ms(lambda i: K.wavenet_inputs(x, inputs, labels, levels=Q), args.iters)
        emit(what='wavenet_inputs kernel, %d levels' % Q, levels=Q, us=1e3 * r[0], min=1e3 * r[1], max=1e3 * r[2],
             n=args.batch * args.length, iters=args.iters)

    # (c) the generators
    def gen_inputs(model, B, n):
        g = torch.Generator().manual_seed(B)
        enc = (0.5 * torch.randn(B, model.Cc, -(-n // RATIO), generator=g)).to(dev)
        return enc, torch.rand(B, n, generator=g).to(dev)

    for kind, B, n in (('fast', 1, args.fast_steps), ('wide', 256, args.wide_steps)):
        make = pkg.generator.FastGenerator if kind == 'fast' else pkg.generator.WideGenerator
        gens = {Q: make(models[Q], batch=B) for Q in LEVELS}
        data = {Q: gen_inputs(models[Q], B, n) for Q in LEVELS}

        def run(Q):
            enc, u = data[Q]
            gens[Q].reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            gens[Q].generate(enc, n, mode='sample', uniforms=u, ratio=RATIO)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e6 / n
        for Q in LEVELS:                           # graph capture, first touch of the weights
            run(Q)
        us = {Q: [] for Q in LEVELS}
        for _ in range(args.rounds):
            for Q in LEVELS:
                us[Q].append(run(Q))
        for Q in LEVELS:
            emit(what='%s generator, B = %d, %d levels' % (kind, B, Q), generator=kind, B=B, levels=Q,
                 us_per_step=statistics.median(us[Q]), min=min(us[Q]), max=max(us[Q]), steps=n, rounds=args.rounds)
            gens[Q].close()

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        for ln in lines:
            f.write(json.dumps(ln) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
