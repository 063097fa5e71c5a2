#!/usr/bin/env python3
"""Code steps of the wide generator's code-input mode against PriorGenerator, at the default prior (prior_parameters.json:
R 256, S 512, 512 codes, 20 layers, pre_k 1) with random weights, DESIGN 3.15.

  measure  ONE process: WidePriorGenerator at B = 8, 64, 256 and 1024 and PriorGenerator at B = 1 and 8, mode 'sample' with
           supplied uniforms.  `--rounds` rounds that alternate the six generators; host clock around one sample() call of
           `--wide_steps` / `--fast_steps` code steps plus a device synchronise.  Per generator: median (min .. max) of the
           rounds in us per step and total codes/s, and the smallest wide batch whose total rate passes PriorGenerator's 8-row
           total of the same run.
  profile  one `rocprofv3 --kernel-trace --stats` run of a wide code handle at `--profile_batch` rows: the time of every
           kernel of a step, arw_pre_code_kernel and the code-mode sampling kernel (arw_sample_kernel<true>) on their own.

Each part runs as a child process under its own `timeout`; the second is not started when the first fails.  One JSON line per
result, printed and written to profiles/wide_prior_bench_lines.json (`--out`); lines of that file that carry a "training_path"
key (the alternating bench.py pair recorded beside them) are kept.

    python tools/wide_prior_bench.py [--rounds 3] [--wide_steps 256] [--fast_steps 1536] [--profile_batch 256] [--out FILE]
"""
import argparse
import csv
import glob
import importlib
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WIDE_B = (8, 64, 256, 1024)
FAST_B = (1, 8)


def make_prior():
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('wide_prior_bench.py needs a GPU')
    pkg = importlib.import_module('vq-vae-wavenet_amd')
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    with open(os.path.join(ROOT, 'prior_parameters.json')) as f:
        cfg = json.load(f)
    cfg['verbose'] = False
    prior = pkg.prior.LatentPrior(cfg, 109, device=dev, seed=0)
    g = torch.Generator().manual_seed(1)
    named = {}
    for n, v in prior.named_parameters().items():          # every variable random, the zero-initialised ones included
        scale = float(v.abs().max()) if float(v.abs().max()) > 0 else 0.1
        named[n] = ((torch.rand(v.shape, generator=g) * 2 - 1) * scale).float()
    prior.load_named(named)
    return pkg, prior, dev


def inputs(B, n, dev):
    import torch
    g = torch.Generator().manual_seed(B)
    return torch.randint(0, 109, (B,), generator=g).to(dev), torch.rand(B, n, generator=g).to(dev)


def measure(args):
    import torch
    pkg, prior, dev = make_prior()
    emit = lambda **kw: print(json.dumps(kw), flush=True)  # noqa: E731
    gens = [('wide', B, pkg.generator.WidePriorGenerator(prior, batch=B), args.wide_steps) for B in WIDE_B] + \
           [('persistent', B, pkg.generator.PriorGenerator(prior, batch=B), args.fast_steps) for B in FAST_B]
    data = {(k, B): inputs(B, n, dev) for k, B, _, n in gens}

    def run(kind, B, gen, n):
        spk, u = data[(kind, B)]
        gen.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        gen.sample(n, spk, mode='sample', uniforms=u)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / n

    for g in gens:                                 # graph capture, first touch of the weights
        run(*g)
    us = {(k, B): [] for k, B, _, _ in gens}
    for _ in range(args.rounds):
        for g in gens:
            us[g[:2]].append(run(*g))
    rate = {}
    for kind, B, gen, n in gens:
        v = us[(kind, B)]
        med = statistics.median(v)
        rate[(kind, B)] = B * 1e6 / med
        emit(what='%s prior generator, B = %d' % (kind, B), generator=kind, B=B, us_per_step=med, min=min(v), max=max(v),
             us_per_row_step=med / B, codes_per_s=B * 1e6 / med, codes_per_s_min=B * 1e6 / max(v), codes_per_s_max=B * 1e6 / min(v),
             steps=n, rounds=args.rounds)
        gen.close()
    yard = rate[('persistent', 8)]
    over = [B for B in WIDE_B if rate[('wide', B)] > yard]
    emit(what='smallest wide batch whose total rate passes PriorGenerator at 8 rows in this run', overtakes_at=over[0] if over else None,
         persistent8_codes_per_s=yard, wide_codes_per_s={str(B): rate[('wide', B)] for B in WIDE_B})


def profile(args):
    import torch
    pkg, prior, dev = make_prior()
    B, n = args.profile_batch, 64
    gen = pkg.generator.WidePriorGenerator(prior, batch=B)
    spk, u = inputs(B, n, dev)
    gen.sample(n, spk, mode='sample', uniforms=u)
    torch.cuda.synchronize()
    gen.close()


def kernel_times(out_dir, B):
    """Lines of the per-kernel summary of the profile run: from rocprofv3's kernel_stats.csv, or its database."""
    found = glob.glob(os.path.join(out_dir, '**', '*kernel_stats.csv'), recursive=True)
    if not found:
        dbs = glob.glob(os.path.join(out_dir, '**', '*.db'), recursive=True)
        if not dbs:
            return [dict(what='profile: rocprofv3 left neither a kernel_stats.csv nor a database')]
        found = [os.path.join(out_dir, 'kernel_stats.csv')]
        subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'rocpd_stats.py'), dbs[0], found[0]], check=True, timeout=120)
    lines = []
    with open(found[0], newline='') as f:
        for row in csv.DictReader(f):
            name = row['Name'].replace('(anonymous namespace)::', '')
            if 'arw_' not in name:
                continue
            lines.append(dict(what='wide code step at B = %d: kernel time' % B, kernel=name[:120], calls=int(row['Calls']),
                              total_us=float(row['TotalDurationNs']) / 1e3, avg_us=float(row['AverageNs']) / 1e3))
    tot = sum(ln['total_us'] for ln in lines) or 1.0
    for ln in lines:
        ln['share_of_wide_kernels'] = ln['total_us'] / tot
    return lines


def kept_lines(path):
    """The training-path lines already in the output file (written beside this tool's, not by it)."""
    if not os.path.exists(path):
        return []
    keep = []
    with open(path) as f:
        for ln in f:
            try:
                rec = json.loads(ln)
            except ValueError:
                continue
            if isinstance(rec, dict) and 'training_path' in rec:
                keep.append(rec)
    return keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--part', choices=['all', 'measure', 'profile'], default='all')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--wide_steps', type=int, default=256)
    ap.add_argument('--fast_steps', type=int, default=1536)
    ap.add_argument('--profile_batch', type=int, default=256)
    ap.add_argument('--timeout', type=int, default=240, help='seconds each part may take')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'wide_prior_bench_lines.json'))
    args = ap.parse_args()
    if args.part == 'measure':
        return measure(args)
    if args.part == 'profile':
        return profile(args)
    me = [sys.executable, os.path.abspath(__file__), '--rounds', str(args.rounds), '--wide_steps', str(args.wide_steps),
          '--fast_steps', str(args.fast_steps), '--profile_batch', str(args.profile_batch)]
    lines = []
    out = subprocess.run(me + ['--part', 'measure'], capture_output=True, text=True, timeout=args.timeout)
    lines += [json.loads(ln) for ln in out.stdout.splitlines() if ln.startswith('{')]
    ok = out.returncode == 0
    if not ok:
        lines.append(dict(what='measure failed', returncode=out.returncode, stderr=out.stderr[-2000:]))
    elif shutil.which('rocprofv3') is None:
        lines.append(dict(what='profile skipped: rocprofv3 is not installed'))
    else:
        tmp = tempfile.mkdtemp(prefix='wide_prior_prof_')
        try:
            out = subprocess.run(['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', tmp, '-o', 'wide', '--']
                                 + me + ['--part', 'profile'], capture_output=True, text=True, timeout=args.timeout)
            if out.returncode == 0:
                lines += kernel_times(tmp, args.profile_batch)
            else:
                ok = False
                lines.append(dict(what='profile failed', returncode=out.returncode, stderr=out.stderr[-2000:]))
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    lines += kept_lines(args.out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        for ln in lines:
            print(json.dumps(ln))
            f.write(json.dumps(ln) + '\n')
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
