#!/usr/bin/env python3
"""Cost of the codebook by moving averages on one GPU at bench.py's shape (B = 8, T = 6656, reference widths).

  * the two kernels alone at the step's latent shape (z_e [8][64][104], 832 frames, K = 512 codes of D = 64): HIP events around
    windows of `--iters` launches, the median of 5 windows, in us -- vqw_vq_cluster_stats with the step's own codes and with every
    frame on ONE code (the longest sequential sum), vqw_vq_codebook_ema_step, and the draw of the picks;
  * ms per training step (deferred range guard, as train.py runs it) with codebook_ema 0 and `--decay` / `--restart` (0.99 /
    0.05): `--rounds` rounds that run the two modes one after another, `--steps` steps each, host clock around the steps +
    finish_steps + a device synchronise; median, min and max over the rounds, and codebook_info() of the last step.
One JSON line each.  (The "on" rounds move the codebook; every "off" round starts from the parameters the run began with.)

    python tools/codebook_bench.py [--steps 20] [--rounds 3] [--iters 200] [--decay 0.99] [--restart 0.05]
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
    ap.add_argument('--decay', type=float, default=0.99)
    ap.add_argument('--restart', type=float, default=0.05)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--length', type=int, default=6656)
    args = ap.parse_args()
    import torch
    import bench
    from clip_bench import median_ms
    if not torch.cuda.is_available():
        raise SystemExit('codebook_bench.py needs a GPU')
    pkg = importlib.import_module('vq-vae-wavenet_amd')
    K = pkg.kernels
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    m, w = bench.default_configs()
    model = pkg.model.VQVAE(m, w, 109, device=dev, seed=0)
    model.defer_guard = True
    x, spk = bench.synthetic_batch(args.batch, args.length, 109, 1234, dev)
    emit = lambda **kw: print(json.dumps(kw), flush=True)  # noqa: E731

    B, D, Kc, Tz = args.batch, model.D, model.Kc, args.length // 64
    ws = model.forward(x, spk)                                     # the step's own z_e and codes
    torch.cuda.synchronize()
    z_e, idx = ws['z_e'].clone(), ws['idx'].clone()
    one = torch.zeros_like(idx)
    cnt, pick = torch.zeros(Kc, dtype=torch.int32, device=dev), torch.randint(0, B * Tz, (Kc,), dtype=torch.int32, device=dev)
    tot, cand = torch.empty(Kc, D, device=dev), torch.empty(Kc, D, device=dev)
    emb, n_, m_ = model.P['embedding'].clone(), torch.ones(Kc, device=dev), model.P['embedding'].clone()
    info = torch.zeros(8, dtype=torch.int32, device=dev)
    s = median_ms(lambda i: K.vq_cluster_stats(z_e, idx, cnt=cnt, sum=tot, pick=pick, cand=cand, K=Kc), args.iters)
    used = int((cnt > 0).sum())
    s1 = median_ms(lambda i: K.vq_cluster_stats(z_e, one, cnt=cnt, sum=tot, pick=pick, cand=cand, K=Kc), args.iters)
    K.vq_cluster_stats(z_e, idx, cnt=cnt, sum=tot, pick=pick, cand=cand, K=Kc)
    e = median_ms(lambda i: K.vq_codebook_ema_step(emb, n_, m_, cnt=cnt, sum=tot, cand=cand, decay=args.decay, restart=args.restart,
                                                   info=info), args.iters)
    g = median_ms(lambda i: model.codebook_uniforms(Kc, i), args.iters)
    for what, r, extra in (('vqw_vq_cluster_stats', s, {'codes_used': used}), ('vqw_vq_cluster_stats, one code', s1, {'codes_used': 1}),
                           ('vqw_vq_codebook_ema_step', e, {}), ('codebook_uniforms (seed + torch.rand)', g, {})):
        emit(what=what, us=1e3 * r[0], min=1e3 * r[1], max=1e3 * r[2], B=B, D=D, Tz=Tz, K=Kc, iters=args.iters, **extra)

    def steps(n):
        t0 = time.perf_counter()
        for _ in range(n):
            ws = model.train_step(x, spk)
        model.finish_steps()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n, ws

    start = {k: v.clone() for k, v in model.state_dict().items()}
    modes = [('off', 0.0, 0.0), ('on', args.decay, args.restart)]

    def switch(decay, restart):
        model.codebook_restart = 0.0
        model.codebook_ema, model.codebook_restart = decay, restart
        model.load_state_dict(start)                             # (feature on: n = 1, m = the embedding again)

    for _, decay, restart in modes:                              # workspaces, guard scales, the statistics' buffers
        switch(decay, restart)
        steps(4)
    ms, last = {name: [] for name, _, _ in modes}, {}
    for _ in range(args.rounds):
        for name, decay, restart in modes:
            switch(decay, restart)
            t, ws = steps(args.steps)
            ms[name].append(t)
            last[name] = model.codebook_info() if decay > 0 else None
    for name, decay, restart in modes:
        emit(what='train step, codebook_ema %s' % name, codebook_ema=decay, codebook_restart=restart,
             ms_per_step=statistics.median(ms[name]), min=min(ms[name]), max=max(ms[name]), rounds=args.rounds, steps=args.steps,
             codebook_info=last[name], x3_fallbacks=model.x3_fallbacks)


if __name__ == '__main__':
    main()
