#!/usr/bin/env python3
"""Cost of gradient accumulation on one GPU (WaveNet.accumulate).

  (a) vqw_grad_accumulate alone at the reference model's n_flat (35.2 M floats, 140.6 MB per stream) in its three forms -- the
      copy acc = grad (2 streams: 8 B per parameter), the add acc = acc + grad and the closing grad = acc + grad (3 streams:
      12 B per parameter) -- in us and GB/s, with the Adam + EMA kernel (9 streams of traffic over its five buffers: 36 B per
      parameter) timed in the same run as the yardstick.  HIP events around windows of `--iters` launches, the median of 5
      windows (min and max beside it).  Two or three buffers of 140.6 MB do not fit the 256 MB Infinity Cache together, and in
      a step the backward pass has streamed gigabytes between two calls: every launch also runs over buffers rotated among 4
      sets (`rotating`: every read from HBM).
  (b) ms per MICRO-step at bench.py's shape (B = 8, T = 6656, deferred range guard, as train.py runs it) with accumulate 1 and
      4: `--rounds` rounds that alternate the two modes, `--steps` micro-steps each (a multiple of 4: whole windows), host clock
      around the steps + finish_steps + a device synchronise; median, min and max over the rounds.
One JSON line each.

    python tools/accum_bench.py [--steps 20] [--rounds 3] [--iters 50]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--length', type=int, default=6656)
    args = ap.parse_args()
    if args.steps % 4:
        ap.error('--steps must be a multiple of 4 (whole windows of accumulate = 4)')
    import torch
    import bench
    from clip_bench import median_ms
    if not torch.cuda.is_available():
        raise SystemExit('accum_bench.py needs a GPU')
    pkg = importlib.import_module('vq-vae-wavenet_amd')
    K = pkg.kernels
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    m, w = bench.default_configs()
    model = pkg.model.VQVAE(m, w, 109, device=dev, seed=0)
    model.defer_guard = True
    x, spk = bench.synthetic_batch(args.batch, args.length, 109, 1234, dev)
    emit = lambda **kw: print(json.dumps(kw), flush=True)  # noqa: E731

    def steps(n):
        t0 = time.perf_counter()
        for _ in range(n):
            model.train_step(x, spk)
        model.finish_steps()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    # (b) first: the model's buffers are untouched by the kernel timings
    steps(5)                                   # workspaces, guard scales
    model.accumulate = 4
    steps(4)                                   # the accumulator
    ms = {1: [], 4: []}
    for _ in range(args.rounds):
        for n_acc in (1, 4):
            model.accumulate = n_acc
            ms[n_acc].append(steps(args.steps))
    for n_acc in (1, 4):
        emit(what='train micro-step, accumulate %d' % n_acc, accumulate=n_acc, ms_per_micro_step=statistics.median(ms[n_acc]),
             min=min(ms[n_acc]), max=max(ms[n_acc]), rounds=args.rounds, steps=args.steps, global_step=model.global_step,
             x3_fallbacks=model.x3_fallbacks)
    model.accumulate = 1

    # (a) the kernel alone
    n = model.n_flat
    mb = 4e-6 * n
    model.grad.mul_(1e-3)
    sets = [(model.grad, model._acc, torch.empty_like(model.grad))] + \
        [(model.grad.clone(), model._acc.clone(), torch.empty_like(model.grad)) for _ in range(3)]
    adam_sets = [(model.flat, model.adam_m, model.adam_v, model.ema)] + \
        [tuple(t.clone() for t in (model.flat, model.adam_m, model.adam_v, model.ema)) for _ in range(3)]
    forms = [('copy acc = grad', 2, lambda g, a, o: K.grad_accumulate(a, g)),
             ('add acc = acc + grad', 3, lambda g, a, o: K.grad_accumulate(a, g, acc=a)),
             ('close grad = acc + grad', 3, lambda g, a, o: K.grad_accumulate(g, g, acc=a)),
             ('add out = acc + grad, out distinct', 3, lambda g, a, o: K.grad_accumulate(o, g, acc=a))]

    def adam(i, rot):       # lr_t = 0: the parameters stay where they are
        p, am, av, e = adam_sets[i % 4 if rot else 0]
        K.adam_ema_step(p, sets[i % 4 if rot else 0][0], am, av, e, lr_t=0.0)
    for rot in (False, True):
        tag = ', rotating over 4 buffer sets' if rot else ', same buffers'
        a_ms = median_ms(lambda i: adam(i, rot), args.iters)
        rate = 9 * mb / a_ms[0]                  # GB/s (MB per ms)
        emit(what='adam_ema kernel' + tag, us=1e3 * a_ms[0], min=1e3 * a_ms[1], max=1e3 * a_ms[2], MB=9 * mb, GBps=rate, n=n)
        for what, streams, fn in forms:
            for t in sets:                       # the adds grow what they add to: every form starts from a zero accumulator
                t[1].zero_()
            r = median_ms(lambda i: fn(*sets[i % 4 if rot else 0]), args.iters)
            emit(what='grad_accumulate, ' + what + tag, us=1e3 * r[0], min=1e3 * r[1], max=1e3 * r[2], MB=streams * mb,
                 GBps=streams * mb / r[0], share_of_adam_rate=streams * mb / r[0] / rate, n=n)


if __name__ == '__main__':
    main()
