#!/usr/bin/env python3
"""Latent prior (prior.py) timings on one GPU: ms per training step and code frames per second at B = 16, T = 1024 with the
default prior_parameters.json, on the default engine and on VQW_ENGINE=fp32 (each in a fresh child process: the engine is
chosen at construction); prior sampling in us per code for 1 and 8 rows (generator.PriorGenerator).  One JSON line each.
--part masked: the same step with lengths=None and with lengths drawn uniformly in [256, 1024], in alternating
rounds of --steps steps (medians over --rounds rounds), and the loss kernel alone in us for both (HIP events, median of 20).

    python tools/prior_bench.py [--steps 20] [--warmup 5] [--codes 512] [--rounds 3]
"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def train(args):
    import torch
    pkg = importlib.import_module('vq-vae-wavenet_amd')
    with open(os.path.join(ROOT, 'prior_parameters.json')) as f:
        cfg = json.load(f)
    torch.cuda.set_device(0)
    B, T, k = 16, 1024, cfg['quantization_channels']
    prior = pkg.prior.LatentPrior(cfg, 109, device='cuda', seed=0)
    prior.defer_guard = True            # as train_prior.py runs it
    g = torch.Generator().manual_seed(0)
    codes = torch.randint(0, k, (B, T), generator=g).int().cuda()
    spk = torch.randint(0, 109, (B,), generator=g).cuda()
    for _ in range(args.warmup):
        prior.train_step(codes, spk)
    prior.finish_steps()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(args.steps):
        prior.train_step(codes, spk)
    prior.finish_steps()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t) * 1e3 / args.steps
    print(json.dumps({'what': 'prior_train_step', 'engine': os.environ.get('VQW_ENGINE', pkg.model.DEFAULT_ENGINE), 'B': B, 'T': T,
                      'ms_per_step': round(ms, 3), 'frames_per_s': round(B * T / ms * 1e3), 'x3_steps': prior.x3_steps,
                      'x3_fallbacks': prior.x3_fallbacks}), flush=True)


def masked(args):
    import statistics
    import torch
    pkg = importlib.import_module('vq-vae-wavenet_amd')
    K = pkg.kernels
    with open(os.path.join(ROOT, 'prior_parameters.json')) as f:
        cfg = json.load(f)
    torch.cuda.set_device(0)
    B, T, k = 16, 1024, cfg['quantization_channels']
    prior = pkg.prior.LatentPrior(cfg, 109, device='cuda', seed=0)
    prior.defer_guard = True
    g = torch.Generator().manual_seed(0)
    codes = torch.randint(0, k, (B, T), generator=g).int().cuda()
    spk = torch.randint(0, 109, (B,), generator=g).cuda()
    draws = [torch.randint(256, T + 1, (B,), generator=g).tolist() for _ in range(args.steps)]      # a fresh draw per step of a round

    def run(lengths_of, n):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for i in range(n):
            prior.train_step(codes, spk, lengths=lengths_of(i))
        prior.finish_steps()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3 / n
    modes = {'unmasked': lambda i: None, 'masked': lambda i: draws[i % len(draws)]}
    for fn in modes.values():
        run(fn, args.warmup)
    ms = {name: [] for name in modes}
    for _ in range(args.rounds):
        for name, fn in modes.items():
            ms[name].append(run(fn, args.steps))
    # the loss kernel alone, out of place into a scratch buffer (the logits stay what they are), rotating over 8 logits buffers
    bufs = [torch.randn(B, k, T, device='cuda') for _ in range(8)]
    scratch, loss = torch.empty(B, k, T, device='cuda'), torch.zeros(1, device='cuda')
    t_end = torch.tensor(draws[0], dtype=torch.int32, device='cuda')
    count = sum(draws[0])

    def median_us(call, iters=20):
        for i in range(3):
            call(i)
        out = []
        for i in range(iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call(i)
            b.record()
            b.synchronize()
            out.append(a.elapsed_time(b) * 1e3)
        return statistics.median(out)
    us = {'unmasked': median_us(lambda i: K.softmax_xent(bufs[i % 8], codes, loss_sum=loss, dlogits=scratch, grad_scale=1.0 / (B * T))),
          'masked': median_us(lambda i: K.softmax_xent_ranged(bufs[i % 8], codes, loss_sum=loss, dlogits=scratch, grad_scale=1.0 / count,
                                                              t_end=t_end))}
    print(json.dumps({'what': 'prior_masked_step', 'B': B, 'T': T, 'steps': args.steps, 'rounds': args.rounds,
                      'scored_share': round(sum(map(sum, draws)) / (len(draws) * B * T), 3),
                      'ms_per_step': {n: round(statistics.median(v), 3) for n, v in ms.items()},
                      'ms_per_step_rounds': {n: [round(x, 3) for x in v] for n, v in ms.items()},
                      'loss_kernel_us': {n: round(v, 2) for n, v in us.items()}, 'loss_kernel_scored_share': round(count / (B * T), 3),
                      'x3_steps': prior.x3_steps, 'x3_fallbacks': prior.x3_fallbacks}), flush=True)


def sample(args):
    import torch
    pkg = importlib.import_module('vq-vae-wavenet_amd')
    with open(os.path.join(ROOT, 'prior_parameters.json')) as f:
        cfg = json.load(f)
    torch.cuda.set_device(0)
    prior = pkg.prior.LatentPrior(cfg, 109, device='cuda', seed=0)
    for rows in (1, 8):
        spk = torch.arange(rows, dtype=torch.int64, device='cuda')
        gen = pkg.generator.PriorGenerator(prior, batch=rows)
        gen.sample(64, spk)
        torch.cuda.synchronize()
        t = time.perf_counter()
        gen.sample(args.codes, spk, mode='sample')
        torch.cuda.synchronize()
        us = (time.perf_counter() - t) * 1e6 / args.codes
        gen.close()
        print(json.dumps({'what': 'prior_sampling', 'rows': rows, 'codes': args.codes, 'us_per_code': round(us, 2)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--codes', type=int, default=512)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--part', choices=['all', 'train', 'sample', 'masked'], default='all')
    args = ap.parse_args()
    if args.part == 'train':
        return train(args)
    if args.part == 'sample':
        return sample(args)
    if args.part == 'masked':
        return masked(args)
    base = [sys.executable, os.path.abspath(__file__), '--steps', str(args.steps), '--warmup', str(args.warmup), '--codes', str(args.codes)]
    for env in ({}, {'VQW_ENGINE': 'fp32'}):
        subprocess.run(base + ['--part', 'train'], env=dict(os.environ, **env), check=True, timeout=900)
    subprocess.run(base + ['--part', 'sample'], check=True, timeout=900)
    subprocess.run(base + ['--part', 'masked', '--rounds', str(args.rounds)], check=True, timeout=900)


if __name__ == '__main__':
    main()
