#!/usr/bin/env python3
"""Prefill of the wide generator at the reference widths (R 256, S 512, 30 layers), DESIGN 3.15.

  measure  ONE process: WideGenerator.prefill_prompt at B = 8, 64 and 256 rows for prompts of 8 000 and 48 000 samples (both
           longer than the window of 6 170, so both cost a window).  `--rounds` rounds that alternate the six cases; HIP events
           around the whole prefill call (reset, the chunked teacher-forced passes, the scatters, the finish).  Per case: the
           median (min .. max) in ms per call and per row, and the rows per pass (generator.prefill_chunk, cut evenly).  Beside
           it, DERIVED, not measured: what stepping a window's worth of steps would cost at the step times of
           profiles/wide_gen_bench_lines.json.  A wide handle cannot step teacher-forced, so that is a yardstick only.
  profile  one `rocprofv3 --kernel-trace --stats` run of `--profile_calls` prefills at `--profile_batch` rows: the time of
           the scatter kernels and their bytes/s against 2 (ks-1) sum(d) R rows 4 bytes per prefill (every ring float read
           once and written once).

Each part runs as a child process under its own `timeout`; the second is not started when the first fails.  One JSON line per
result, printed and written to profiles/wide_prefill_bench_lines.json (`--out`).  Nothing here asserts a time.

    python tools/wide_prefill_bench.py [--rounds 3] [--profile_batch 256] [--profile_calls 2] [--out FILE]
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROWS = (8, 64, 256)
PROMPTS = (8000, 48000)
RATIO = 64


def make_model():
    import torch
    import bench
    if not torch.cuda.is_available():
        raise SystemExit('wide_prefill_bench.py needs a GPU')
    pkg = importlib.import_module('vq-vae-wavenet_amd')
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    m, w = bench.default_configs()
    return pkg, pkg.model.VQVAE(m, w, 109, device=dev, seed=0), dev


def inputs(model, B, T, dev):
    import torch
    g = torch.Generator().manual_seed(B)
    enc = (0.5 * torch.randn(B, model.Cc, -(-T // RATIO) + 8, generator=g)).to(dev)
    return (torch.rand(B, T, generator=g) * 1.6 - 0.8).to(dev), enc


def step_times():
    """us per step of the wide generator by batch size, from the committed lines of tools/wide_gen_bench.py."""
    out = {}
    path = os.path.join(ROOT, 'profiles', 'wide_gen_bench_lines.json')
    if os.path.exists(path):
        with open(path) as f:
            for ln in f:
                d = json.loads(ln) if ln.startswith('{') else {}
                if d.get('generator') == 'wide':
                    out[d['B']] = d['us_per_step']
    return out


def measure(args):
    import torch
    pkg, model, dev = make_model()
    emit = lambda **kw: print(json.dumps(kw), flush=True)  # noqa: E731
    W = pkg.wavenet.prefill_window(0, model.ks, model.dil, model.pre_k, RATIO)[0]
    gens = {B: pkg.generator.WideGenerator(model, batch=B) for B in ROWS}
    cases = [(B, T) for B in ROWS for T in PROMPTS]
    data = {c: inputs(model, c[0], c[1], dev) for c in cases}

    def run(B, T):
        prompt, enc = data[(B, T)]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        gens[B].prefill_prompt(prompt, enc, ratio=RATIO)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for c in cases:                                # first touch of the weights, the pass's workspaces
        run(*c)
    ms = {c: [] for c in cases}
    for _ in range(args.rounds):
        for c in cases:
            ms[c].append(run(*c))
    steps = step_times()
    for B, T in cases:
        v = ms[(B, T)]
        med = statistics.median(v)
        _, s0, end = pkg.wavenet.prefill_window(T, model.ks, model.dil, model.pre_k, RATIO)
        chunk = pkg.generator.even_chunk(B, pkg.generator.prefill_chunk(B, model.R, model.Mall, end - s0, (end - s0) // RATIO))
        line = dict(what='wide prefill, B = %d, prompt of %d samples' % (B, T), B=B, T=T, window=min(T, W), rows_per_pass=chunk,
                    ms_per_call=med, min=min(v), max=max(v), ms_per_row=med / B, rounds=args.rounds)
        if B in steps:
            line['derived_not_measured_ms_of_stepping_a_window'] = steps[B] * min(T, W) / 1e3
            line['derived_from'] = 'profiles/wide_gen_bench_lines.json: %.1f us per step at B = %d, times %d steps' % (
                steps[B], B, min(T, W))
        emit(**line)
    for gen in gens.values():
        gen.close()


def profile(args):
    import torch
    pkg, model, dev = make_model()
    B, T = args.profile_batch, PROMPTS[-1]
    gen = pkg.generator.WideGenerator(model, batch=B)
    prompt, enc = inputs(model, B, T, dev)
    for _ in range(args.profile_calls):
        gen.prefill_prompt(prompt, enc, ratio=RATIO)
    torch.cuda.synchronize()
    gen.close()


def scatter_lines(out_dir, args):
    """The scatter and finish kernels of the profile run: from rocprofv3's kernel_stats.csv, or its database."""
    import bench
    found = glob.glob(os.path.join(out_dir, '**', '*kernel_stats.csv'), recursive=True)
    if not found:
        dbs = glob.glob(os.path.join(out_dir, '**', '*.db'), recursive=True)
        if not dbs:
            return [dict(what='profile: rocprofv3 left neither a kernel_stats.csv nor a database')]
        found = [os.path.join(out_dir, 'kernel_stats.csv')]
        subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'rocpd_stats.py'), dbs[0], found[0]], check=True, timeout=120)
    _, w = bench.default_configs()
    B, calls = args.profile_batch, args.profile_calls
    ring_floats = (w['kernel_size'] - 1) * sum(w['dilation_rates']) * w['residual_filters'] * B
    lines = []
    with open(found[0], newline='') as f:
        for row in csv.DictReader(f):
            name = row['Name'].replace('(anonymous namespace)::', '')
            if 'arw_prefill' not in name:
                continue
            ln = dict(what='wide prefill at B = %d, %d calls: kernel' % (B, calls), kernel=name[:120], calls=int(row['Calls']),
                      total_us=float(row['TotalDurationNs']) / 1e3, avg_us=float(row['AverageNs']) / 1e3)
            if 'scatter' in name:
                ln['us_per_prefill'] = ln['total_us'] / calls
                ln['bytes_per_prefill'] = 2 * ring_floats * 4
                ln['bytes_per_s'] = ln['bytes_per_prefill'] * calls / (ln['total_us'] * 1e-6)
            lines.append(ln)
    return lines or [dict(what='profile: no arw_prefill kernel in the trace')]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--part', choices=['all', 'measure', 'profile'], default='all')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--profile_batch', type=int, default=256)
    ap.add_argument('--profile_calls', type=int, default=2)
    ap.add_argument('--timeout', type=int, default=240, help='seconds each part may take')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'wide_prefill_bench_lines.json'))
    args = ap.parse_args()
    if args.part == 'measure':
        return measure(args)
    if args.part == 'profile':
        return profile(args)
    me = [sys.executable, os.path.abspath(__file__), '--rounds', str(args.rounds), '--profile_batch', str(args.profile_batch),
          '--profile_calls', str(args.profile_calls)]
    lines = []
    out = subprocess.run(me + ['--part', 'measure'], capture_output=True, text=True, timeout=args.timeout)
    lines += [json.loads(ln) for ln in out.stdout.splitlines() if ln.startswith('{')]
    ok = out.returncode == 0
    if not ok:
        lines.append(dict(what='measure failed', returncode=out.returncode, stderr=out.stderr[-2000:]))
    elif shutil.which('rocprofv3') is None:
        lines.append(dict(what='profile skipped: rocprofv3 is not installed'))
    else:
        tmp = tempfile.mkdtemp(prefix='wide_prefill_prof_')
        try:
            out = subprocess.run(['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', tmp, '-o', 'prefill', '--']
                                 + me + ['--part', 'profile'], capture_output=True, text=True, timeout=args.timeout)
            if out.returncode == 0:
                lines += scatter_lines(tmp, args)
            else:
                ok = False
                lines.append(dict(what='profile failed', returncode=out.returncode, stderr=out.stderr[-2000:]))
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        for ln in lines:
            print(json.dumps(ln))
            f.write(json.dumps(ln) + '\n')
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
