#!/usr/bin/env python3
"""Held-out scoring timings on one GPU at bench.py's shape (B = 8, T = 6656, reference widths): the two kernels alone
(vqw_softmax_score with and without its per-position outputs, vqw_code_histogram; the training loss kernel vqw_softmax_xent
for comparison) and VQVAE.evaluate (whole rows and with lengths) beside one training step.  HIP events around windows of
`--iters` launches, the median of 5 windows; the kernels rotate over 8 logits buffers (437 MB) so that no window reads
its logits from the 256 MB Infinity Cache.  One JSON line each.

    python tools/score_bench.py [--iters 50] [--steps 10]
"""
import argparse
import importlib
import json
import os
import statistics
import sys

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
    ap.add_argument('--iters', type=int, default=50, help='kernel launches per timed window')
    ap.add_argument('--steps', type=int, default=10, help='evaluate / train_step calls per timed window')
    args = ap.parse_args()
    import torch
    from oracle import ref_model as M
    pkg = importlib.import_module('vq-vae-wavenet_amd')
    K = pkg.kernels
    assert torch.cuda.is_available(), 'score_bench.py needs a GPU'
    torch.cuda.set_device(0)
    B, T, Q, Kc = 8, 6656, 256, 512
    g = torch.Generator(device='cuda').manual_seed(0)
    bufs = [torch.randn(B, Q, T, device='cuda', generator=g) * 3 for _ in range(8)]
    labels = torch.randint(0, Q, (B, T), device='cuda', generator=g).int()
    nll, ent = torch.empty(B, T, device='cuda'), torch.empty(B, T, device='cuda')
    sums, counts = torch.empty(B, 2, dtype=torch.float64, device='cuda'), torch.empty(B, 2, dtype=torch.int32, device='cuda')
    loss = torch.zeros(1, device='cuda')
    scratch = torch.empty(B, Q, T, device='cuda')
    read = B * T * (4 * Q + 4)

    def report(what, ms, bytes_moved, **kw):
        med, lo, hi = ms
        print(json.dumps(dict(what=what, us=round(med * 1e3, 2), us_min=round(lo * 1e3, 2), us_max=round(hi * 1e3, 2),
                              MB=round(bytes_moved / 1e6, 1), TB_per_s=round(bytes_moved / (med * 1e-3) / 1e12, 2), **kw)), flush=True)

    report('softmax_score (row sums only)', median_ms(lambda i: K.softmax_score(bufs[i % 8], labels, row_sums=sums, row_counts=counts), args.iters), read)
    report('softmax_score (+ nll, entropy per position)',
           median_ms(lambda i: K.softmax_score(bufs[i % 8], labels, nll=nll, entropy=ent, row_sums=sums, row_counts=counts), args.iters),
           read + 8 * B * T)
    report('softmax_xent_fwd (loss sum only)', median_ms(lambda i: K.softmax_xent_fwd(bufs[i % 8], labels, loss_sum=loss), args.iters), read)
    report('softmax_xent (loss + d logits, as train_step)',
           median_ms(lambda i: K.softmax_xent(bufs[i % 8], labels, loss_sum=loss, dlogits=scratch, grad_scale=1.0), args.iters),
           read + 2 * 4 * B * Q * T)
    idx = torch.randint(0, Kc, (B, T // 64), device='cuda', generator=g)
    hist, flag = torch.zeros(Kc, dtype=torch.int32, device='cuda'), torch.zeros(1, dtype=torch.int32, device='cuda')
    report('code_histogram', median_ms(lambda i: K.code_histogram(idx, hist, flag), args.iters), 8 * B * (T // 64))

    m, w = pkg.model.load_configs(os.path.join(ROOT, 'model_parameters.json'), os.path.join(ROOT, 'wavenet_parameters.json'))
    model = pkg.model.VQVAE(m, w, 109, device='cuda', seed=0)
    x, spk, _ = M.synthetic_batch(B, T, 109, 1234)
    x, spk = x[:, :, 0].contiguous().cuda(), spk.cuda()
    lengths = [T - 64 * 13 * b for b in range(B)]
    xl = x.clone()
    for b, n in enumerate(lengths):
        xl[b, n:] = 0
    base = torch.cuda.memory_allocated()
    for _ in range(3):                       # the training steps also give the guarded engine its plane scales
        model.train_step(x, spk)
    model.finish_steps()
    train_bytes = torch.cuda.memory_allocated() - base
    med = median_ms(lambda i: model.train_step(x, spk), args.steps, warmup=1)
    model.finish_steps()
    print(json.dumps({'what': 'train_step', 'ms': round(med[0], 3), 'ms_min': round(med[1], 3), 'ms_max': round(med[2], 3),
                      'workspace_MB': round(train_bytes / 1e6), 'fallbacks': model.x3_fallbacks}), flush=True)
    base = torch.cuda.memory_allocated()
    sc = model.evaluate(x, spk)
    score_bytes = torch.cuda.memory_allocated() - base
    used = bool(model._workspace(B, T, 'score').get('x3_used'))
    for what, fn in (('evaluate (ema, whole rows)', lambda i: model.evaluate(x, spk)),
                     ('evaluate (live, whole rows)', lambda i: model.evaluate(x, spk, weights='live')),
                     ('evaluate (ema, lengths)', lambda i: model.evaluate(xl, spk, lengths=lengths))):
        med = median_ms(fn, args.steps, warmup=1)
        print(json.dumps({'what': what, 'ms': round(med[0], 3), 'ms_min': round(med[1], 3), 'ms_max': round(med[2], 3),
                          'fp16x3_engine': used, 'workspace_MB': round(score_bytes / 1e6),
                          'workspace_bytes_per_sample': round(score_bytes / (B * T)), 'bits_per_sample': round(sum(sc.row_bits()) / B, 4)}),
              flush=True)


if __name__ == '__main__':
    main()
