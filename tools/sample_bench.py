#!/usr/bin/env python3
"""Teacher-forced sampling timings on one GPU at bench.py's shape (B = 8, T = 6656, Q = 256): vqw_softmax_sample alone --
greedy, greedy with probs, default sampling, truncated sampling (temperature 0.8, top-k 50, top-p 0.9), default sampling
with probs -- next to vqw_softmax_score timed in the same run, and VQVAE.reconstruct (greedy / sample) next to
VQVAE.evaluate at the reference widths.  HIP events around windows of `--iters` launches, the median of 5 windows; the
kernels rotate over 8 logits buffers (437 MB) so that no window reads its logits from the 256 MB Infinity Cache.  One JSON
line each.

    python tools/sample_bench.py [--iters 50] [--steps 10]
"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from score_bench import median_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50, help='kernel launches per timed window')
    ap.add_argument('--steps', type=int, default=10, help='reconstruct / evaluate calls per timed window (0: the kernels only)')
    args = ap.parse_args()
    import torch
    from oracle import ref_model as M
    pkg = importlib.import_module('vq-vae-wavenet_amd')
    assert torch.cuda.is_available(), 'sample_bench.py needs a GPU'
    torch.cuda.set_device(0)
    B, T, Q = 8, 6656, 256
    g = torch.Generator(device='cuda').manual_seed(0)
    bufs = [torch.randn(B, Q, T, device='cuda', generator=g) * 3 for _ in range(8)]
    labels = torch.randint(0, Q, (B, T), device='cuda', generator=g).int()
    u = torch.rand(B, T, device='cuda', generator=g)
    idx, audio = torch.empty(B, T, dtype=torch.int32, device='cuda'), torch.empty(B, T, device='cuda')
    probs = torch.empty(B, T, Q, device='cuda')
    sums, counts = torch.empty(B, 2, dtype=torch.float64, device='cuda'), torch.empty(B, 2, dtype=torch.int32, device='cuda')
    read, wrote = B * T * 4 * Q, B * T * 8

    def report(what, ms, bytes_moved):
        med, lo, hi = ms
        print(json.dumps(dict(what=what, us=round(med * 1e3, 2), us_min=round(lo * 1e3, 2), us_max=round(hi * 1e3, 2),
                              MB=round(bytes_moved / 1e6, 1), TB_per_s=round(bytes_moved / (med * 1e-3) / 1e12, 2))), flush=True)

    # the C entry points directly, with the arguments made once: at 10 - 30 us per launch the Python wrappers' own checks and
    # allocations would be part of the figure
    L, lib = pkg._lib, pkg._lib.lib()
    st = L.stream()
    scratch = torch.empty(4 * B * ((T + 63) // 64), device='cuda')
    trunc = dict(temperature=0.8, top_k=50, top_p=0.9)
    rows = (L.ArSampling * B)(*[L.ArSampling(0.8, 50, 0.9) for _ in range(B)])

    def score(i):
        L.check(lib.vqw_softmax_score(L.ptr(bufs[i % 8]), L.ptr(labels), None, None, None, None, L.ptr(sums), L.ptr(counts), L.ptr(scratch),
                                      scratch.numel(), B, Q, T, st))

    def sample(mode, r=None, p=None):
        def fn(i):
            L.check(lib.vqw_softmax_sample(L.ptr(bufs[i % 8]), L.ptr(u) if mode else None, r, None, None, mode, L.ptr(idx), L.ptr(audio),
                                           L.ptr(p), B, Q, T, st))
        return fn
    report('softmax_score (row sums only)', median_ms(score, args.iters), read + 4 * B * T)
    report('softmax_sample greedy', median_ms(sample(0), args.iters), read + wrote)
    report('softmax_sample greedy + probs', median_ms(sample(0, p=probs), args.iters), 2 * read + wrote)
    report('softmax_sample sample, defaults', median_ms(sample(1), args.iters), read + wrote + 4 * B * T)
    report('softmax_sample sample, T 0.8 top_k 50 top_p 0.9', median_ms(sample(1, r=rows), args.iters), read + wrote + 4 * B * T)
    report('softmax_sample sample, defaults + probs', median_ms(sample(1, p=probs), args.iters), 2 * read + wrote + 4 * B * T)

    if args.steps < 1:
        return
    m, w = pkg.model.load_configs(os.path.join(ROOT, 'model_parameters.json'), os.path.join(ROOT, 'wavenet_parameters.json'))
    model = pkg.model.VQVAE(m, w, 109, device='cuda', seed=0)
    x, spk, _ = M.synthetic_batch(B, T, 109, 1234)
    x, spk = x[:, :, 0].contiguous().cuda(), spk.cuda()
    for _ in range(3):                       # the training steps give the guarded engine its plane scales
        model.train_step(x, spk)
    model.finish_steps()
    for what, fn in (('evaluate (ema, whole rows)', lambda i: model.evaluate(x, spk)),
                     ('reconstruct (ema, greedy)', lambda i: model.reconstruct(x, spk, mode='greedy')),
                     ('reconstruct (ema, sample, defaults)', lambda i: model.reconstruct(x, spk, seed=i)),
                     ('reconstruct (ema, sample, T 0.8 top_k 50 top_p 0.9)', lambda i: model.reconstruct(x, spk, seed=i, **trunc))):
        med = median_ms(fn, args.steps, warmup=1)
        print(json.dumps({'what': what, 'ms': round(med[0], 3), 'ms_min': round(med[1], 3), 'ms_max': round(med[2], 3),
                          'fp16x3_engine': bool(model._workspace(B, T, 'score').get('x3_used'))}), flush=True)


if __name__ == '__main__':
    main()
