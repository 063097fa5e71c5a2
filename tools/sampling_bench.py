#!/usr/bin/env python3
"""Cost of temperature / top-k / top-p sampling (csrc/ar_sampling.h) on the persistent generator, in one process: us per
generated step for the audio generator at the reference widths (R 256, S 512, 30 layers, Q 256; 1 and 8 utterances) and
for the latent prior's code sampling with prior_parameters.json (k 512; 1 and 8 speakers), under the settings default,
temperature only, top-k 50, top-p 0.9 and all three.  Each figure is the median of --repeats timed runs after a warm-up run;
`extra_us` is the difference to the default settings of the same generator.  One JSON line per (generator, rows, setting).

    python tools/sampling_bench.py [--steps 2000] [--codes 512] [--repeats 5]
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

SETTINGS = [('default', dict()), ('temperature 0.8', dict(temperature=0.8)), ('top_k 50', dict(top_k=50)),
            ('top_p 0.9', dict(top_p=0.9)), ('all three', dict(temperature=0.8, top_k=50, top_p=0.9))]


def timed(fn, n, repeats, sync):
    fn(64)                                   # warm-up (first launch, allocation of the condition projections)
    sync()
    runs = []
    for _ in range(repeats):
        t = time.perf_counter()
        fn(n)
        sync()
        runs.append((time.perf_counter() - t) * 1e6 / n)
    return statistics.median(runs), min(runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=2000, help='audio samples per timed run')
    ap.add_argument('--codes', type=int, default=512, help='codes per timed run')
    ap.add_argument('--repeats', type=int, default=5)
    args = ap.parse_args()
    import torch
    pkg = importlib.import_module('vq-vae-wavenet_amd')
    torch.cuda.set_device(0)
    sync = torch.cuda.synchronize
    m, w = pkg.model.load_configs(os.path.join(ROOT, 'model_parameters.json'))
    model = pkg.model.VQVAE(m, w, 109, device='cuda', seed=0)
    with open(os.path.join(ROOT, 'prior_parameters.json')) as f:
        prior = pkg.prior.LatentPrior(json.load(f), 109, device='cuda', seed=0)
    g = torch.Generator().manual_seed(0)
    for rows in (1, 8):
        enc = (torch.randn(rows, model.Cc, 64, generator=g) * 0.5).cuda()
        u = torch.rand(rows, args.steps, generator=g).cuda()
        gen = pkg.generator.FastGenerator(model, batch=rows)
        base = None
        for name, kw in SETTINGS:
            def run(n):
                gen.reset()
                gen.generate(enc, n, mode='sample', uniforms=u[:, :n].contiguous(), ratio=64, **kw)
            med, best = timed(run, args.steps, args.repeats, sync)
            base = med if base is None else base
            print(json.dumps({'what': 'audio_sampling', 'R': model.R, 'Q': model.Q, 'rows': rows, 'setting': name,
                              'us_per_step': round(med, 2), 'min_us_per_step': round(best, 2),
                              'extra_us': round(med - base, 2)}), flush=True)
        gen.close()
        spk = torch.arange(rows, dtype=torch.int64, device='cuda')
        uc = torch.rand(rows, args.codes, generator=g).cuda()
        pgen = pkg.generator.PriorGenerator(prior, batch=rows)
        base = None
        for name, kw in SETTINGS:
            def run(n):
                pgen.reset()
                pgen.sample(n, spk, mode='sample', uniforms=uc[:, :n].contiguous(), **kw)
            med, best = timed(run, args.codes, args.repeats, sync)
            base = med if base is None else base
            print(json.dumps({'what': 'prior_sampling', 'k': prior.Q, 'rows': rows, 'setting': name,
                              'us_per_code': round(med, 2), 'min_us_per_code': round(best, 2),
                              'extra_us': round(med - base, 2)}), flush=True)
        pgen.close()


if __name__ == '__main__':
    main()
