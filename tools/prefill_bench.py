#!/usr/bin/env python3
"""Prompted generation: ms per prefill at the reference widths (wavenet_parameters.json) for 1 and 8 rows and prompts of
0.5 s, 3 s and 10 s (FastGenerator.prefill), and the latent prior's prefill (prior_parameters.json, one row) for 64, 256 and
1024 codes (PriorGenerator.prefill).  Next to each: what stepping the same prompt costs (us per generated step x T, the step
time measured on the same handle).  Timed with HIP events around the whole call (median of --reps after one warm-up call).
One JSON line per measurement.

    python tools/prefill_bench.py [--reps 5] [--steps 400]
"""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed_ms(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--steps', type=int, default=400, help='generated steps behind the per-step cost')
    args = ap.parse_args()
    pkg = importlib.import_module('vq-vae-wavenet_amd')
    torch.cuda.set_device(0)
    g = torch.Generator().manual_seed(0)
    cfg, wcfg = pkg.model.load_configs(os.path.join(ROOT, 'model_parameters.json'))
    model = pkg.model.VQVAE(cfg, wcfg, 109, device='cuda', seed=0)
    W = pkg.model.prefill_window(0, model.ks, model.dil, model.pre_k, 64)[0]
    for rows in (1, 8):
        gen = pkg.generator.FastGenerator(model, batch=rows)
        Tz = 160000 // 64 + 8
        enc = (torch.randn(rows, model.Cc, Tz, generator=g) * 0.5).cuda()
        audio = (torch.rand(rows, 160000, generator=g) * 1.6 - 0.8).cuda()
        gen.reset()
        step_ms = timed_ms(lambda: gen.generate(enc, args.steps), 1)
        us_step = step_ms * 1e3 / args.steps
        for sec in (0.5, 3, 10):
            T = int(sec * 16000)
            prompt = audio[:, :T].contiguous()
            ms = timed_ms(lambda: gen.prefill(prompt, enc), args.reps)
            print(json.dumps({'what': 'prefill', 'rows': rows, 'prompt_s': sec, 'T': T, 'window': min(T, W), 'ms': round(ms, 3),
                              'us_per_step': round(us_step, 1), 'stepping_ms': round(us_step * T / 1e3, 1)}), flush=True)
        gen.close()
    with open(os.path.join(ROOT, 'prior_parameters.json')) as f:
        pcfg = json.load(f)
    prior = pkg.prior.LatentPrior(pcfg, 109, device='cuda', seed=0)
    Wp = pkg.model.prefill_window(0, prior.ks, prior.dil, prior.pre_k, 64)[0]
    spk = torch.zeros(1, dtype=torch.int64, device='cuda')
    pgen = pkg.generator.PriorGenerator(prior, batch=1)
    pgen.reset()
    step_ms = timed_ms(lambda: pgen.sample(args.steps, spk), 1)
    us_step = step_ms * 1e3 / args.steps
    codes = torch.randint(0, prior.Q, (1, 1024), generator=g).int().cuda()
    for T in (64, 256, 1024):
        c = codes[:, :T].contiguous()
        ms = timed_ms(lambda: pgen.prefill(c, spk), args.reps)
        print(json.dumps({'what': 'prior_prefill', 'rows': 1, 'codes': T, 'window': min(T, Wp), 'ms': round(ms, 3),
                          'us_per_step': round(us_step, 1), 'stepping_ms': round(us_step * T / 1e3, 1)}), flush=True)
    pgen.close()


if __name__ == '__main__':
    main()
