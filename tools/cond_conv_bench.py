#!/usr/bin/env python3
"""Cost of the decoder's conditioning conv on one GPU at bench.py's shape (B = 8, T = 6656, reference widths).

  * the three kernels alone at the step's latent shape (z_q [8][64][104] -> the first C = 128 rows of the [8][Cc][104]
    condition buffer and back): HIP events around windows of `--iters` launches, the median of 5 windows, in us;
  * ms per training step (deferred range guard, as train.py runs it) with condition_conv 0, 64 (Cc = 128: the projections on
    their own kernels) and 128 (Cc = 192: the projections on the fp32 conv engine): `--rounds` rounds that run the three
    models one after another, `--steps` steps each, host clock around the steps + finish_steps + a device synchronise;
    median, min and max over the rounds.
One JSON line each; `--out FILE` also writes them to FILE (profiles/cond_conv_bench_lines.json).

    python tools/cond_conv_bench.py [--steps 20] [--rounds 3] [--iters 200] [--out profiles/cond_conv_bench_lines.json]
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
    ap.add_argument('--channels', type=int, default=128)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--length', type=int, default=6656)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    import bench
    from clip_bench import median_ms
    if not torch.cuda.is_available():
        raise SystemExit('cond_conv_bench.py needs a GPU')
    pkg = importlib.import_module('vq-vae-wavenet_amd')
    K = pkg.kernels
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    m, w = bench.default_configs()
    x, spk = bench.synthetic_batch(args.batch, args.length, 109, 1234, dev)
    lines = []

    def emit(**kw):
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    B, D, C, k, Tz = args.batch, m['latent_dim'], args.channels, 3, args.length // 64
    Cc = C + m['speaker_embedding']
    z, dz = torch.randn(B, D, Tz, device=dev), torch.empty(B, D, Tz, device=dev)
    cond, dcond = torch.zeros(B, Cc, Tz, device=dev), torch.randn(B, Cc, Tz, device=dev)
    wt, bias = torch.randn(k, D, C, device=dev), torch.randn(C, device=dev)
    dw, db = torch.zeros(k, D, C, device=dev), torch.zeros(C, device=dev)
    scratch = torch.empty(K.cond_conv_wgrad_scratch(B, D, C, Tz, k), device=dev)
    f = median_ms(lambda i: K.cond_conv_fwd(z, wt, bias, cond, out_bstride=Cc * Tz), args.iters)
    g = median_ms(lambda i: K.cond_conv_dgrad(wt, dcond, dz, dout_bstride=Cc * Tz), args.iters)
    h = median_ms(lambda i: K.cond_conv_wgrad(z, dcond, dw, db, scratch, dout_bstride=Cc * Tz), args.iters)
    for what, r, mflop in (('vqw_cond_conv_fwd', f, 2e-6 * B * Tz * k * D * C), ('vqw_cond_conv_dgrad', g, 2e-6 * B * Tz * k * D * C),
                           ('vqw_cond_conv_wgrad (two launches)', h, 2e-6 * B * Tz * (k * D * C + C))):
        emit(what=what, us=1e3 * r[0], min=1e3 * r[1], max=1e3 * r[2], B=B, D=D, C=C, k=k, Tz=Tz, MFLOP=mflop, iters=args.iters)

    def steps(model, n):
        t0 = time.perf_counter()
        for _ in range(n):
            model.train_step(x, spk)
        model.finish_steps()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    models = []
    for c in (0, 64, 128):
        model = pkg.model.VQVAE(dict(m, condition_conv=c), w, 109, device=dev, seed=0)
        model.defer_guard = True
        steps(model, 4)                              # workspaces, guard scales
        models.append((c, model))
    ms = {c: [] for c, _ in models}
    for _ in range(args.rounds):
        for c, model in models:
            ms[c].append(steps(model, args.steps))
    for c, model in models:
        emit(what='train step, condition_conv %d' % c, condition_conv=c, Cc=model.Cc, cond_proj=bool(model.cond_proj),
             ms_per_step=statistics.median(ms[c]), min=min(ms[c]), max=max(ms[c]), rounds=args.rounds, steps=args.steps,
             x3_fallbacks=model.x3_fallbacks)
    if args.out:
        with open(args.out, 'w') as fh:
            json.dump(lines, fh, indent=1)
            fh.write('\n')


if __name__ == '__main__':
    main()
