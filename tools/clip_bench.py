#!/usr/bin/env python3
"""Cost of clipping by global norm on one GPU at bench.py's shape (B = 8, T = 6656, reference widths).

  * ms per training step (deferred range guard, as train.py runs it) with clip_norm None, inf (measure only) and a threshold
    of 1 % of the measured norm (every step clips: `last_scale` < 1): `--rounds` rounds that run the three modes one after another, `--steps` steps
    each, host clock around the steps + finish_steps + a device synchronise; median, min and max over the rounds;
  * the two launches of the norm pass alone, on the model's gradient buffer (140.6 MB: it fits the 256 MB Infinity Cache, as
    it partly does in a step, where the backward pass has just written it) and rotating over 4 buffers of that size (every
    read from HBM), with the arithmetic floor 140.6 MB / rate of the Adam + EMA kernel in the same run;
  * the Adam + EMA kernel alone (36 B per parameter), with and without the device-side scale.
HIP events around windows of `--iters` launches, the median of 5 windows.  One JSON line each.

    python tools/clip_bench.py [--steps 20] [--rounds 3] [--iters 50]
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


def median_ms(fn, iters, windows=5, warmup=3):
    """Median over `windows` of (event time of `iters` calls of fn(i)) / iters, in ms."""
    import torch
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(iters):
            fn(i)
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--length', type=int, default=6656)
    args = ap.parse_args()
    import torch
    import bench
    if not torch.cuda.is_available():
        raise SystemExit('clip_bench.py needs a GPU')
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

    steps(5)                                   # workspaces, guard scales
    model.clip_norm = float('inf')
    steps(3)                                   # the chunk table; the norm the threshold comes from
    gn = model.grad_norms()
    modes = [('off', None), ('measure', float('inf')), ('clip', 0.01 * gn['global'])]    # (the norm falls as the batch is learnt: 1 % of it clips every step)
    ms = {name: [] for name, _ in modes}
    scale = {}
    for _ in range(args.rounds):
        for name, clip in modes:
            model.clip_norm = clip
            ms[name].append(steps(args.steps))
            if clip is not None:
                scale[name] = model.grad_norms()['scale']
    for name, clip in modes:
        emit(what='train step, clip_norm %s' % name, clip_norm=clip, ms_per_step=statistics.median(ms[name]), min=min(ms[name]),
             max=max(ms[name]), rounds=args.rounds, steps=args.steps, last_scale=scale.get(name), x3_fallbacks=model.x3_fallbacks)
    model.clip_norm = None

    n = model.n_flat
    state = model._grad_norm_state()
    plan, out = state['plan'], torch.empty(state['plan'].n_seg + 2, device=dev)
    mb = 4e-6 * n
    adam = lambda sc: (lambda i: K.adam_ema_step(model.flat, model.grad, model.adam_m, model.adam_v, model.ema, lr_t=0.0,  # noqa: E731
                                                 scale=sc))          # lr_t = 0: the parameters stay where they are
    model.grad.mul_(1e-3)
    one = torch.ones(1, device=dev)
    a_ms = median_ms(adam(None), args.iters)
    as_ms = median_ms(adam(one), args.iters)
    rate = 9 * mb / a_ms[0]                      # GB/s (MB per ms)
    emit(what='adam_ema kernel', ms=a_ms[0], min=a_ms[1], max=a_ms[2], MB=9 * mb, GBps=rate)
    emit(what='adam_ema kernel, device scale', ms=as_ms[0], min=as_ms[1], max=as_ms[2], MB=9 * mb, GBps=9 * mb / as_ms[0])
    warm = median_ms(lambda i: K.grad_norm(model.grad, plan, out=out), args.iters)
    bufs = [model.grad] + [model.grad.clone() for _ in range(3)]
    cold = median_ms(lambda i: K.grad_norm(bufs[i % 4], plan, out=out), args.iters)
    for what, r in (('norm pass (2 launches), same buffer', warm), ('norm pass (2 launches), rotating over 4 buffers', cold)):
        emit(what=what, ms=r[0], min=r[1], max=r[2], MB=mb, GBps=mb / r[0], floor_ms_at_adam_rate=mb / rate, chunks=plan.n_chunks,
             segments=plan.n_seg, shorter_than_adam=r[0] < a_ms[0])


if __name__ == '__main__':
    main()
