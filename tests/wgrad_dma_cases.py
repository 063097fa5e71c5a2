"""Seeded cases for the weight gradients with BOTH operands as planes (wgrad_f16x3_dma_kernel<BF>: the LDS-DMA loop), at the
shapes where a ring of 16-step stages can go wrong: K ranges shorter than the ring, one pair per block, a long wrap, taps that
shift by more than a batch row (zeros landing over ring slots that held finite data), batches whose problems differ, output
column blocks, rows that are no multiple of the 32-step pairs, the stride-2 form with parity blocks, one bf16 plane.
Cp = 256, nsplit always explicit: nothing depends on the CU count.

Every case is a dict of keyword arguments for run(); run() returns the dW tensors the planes-both launch wrote (and q_total where
asked).  tests/golden/make_wgrad_dma_digests.py hashes them into tests/golden/wgrad_dma_digests.json at the commit whose bits
are to be kept; tests/test_wgrad_dma_gpu.py compares against that file, the fp32-operand launch and float64."""
import functools
import hashlib

import numpy as np
import torch

DEV = 'cuda:0'
CP = 256
SP, SQ = 2.0 ** 9, 2.0 ** 27            # guard scales of p and q (q: gradients of order 1e-5)
X3_BF16 = 1


@functools.lru_cache(maxsize=None)
def operands(B, T, Q0, seed):
    """(p [B][CP][T], q [B][Q0][T]) fp32 on the host, seeded."""
    rng = np.random.RandomState(4000 + seed)
    return rng.standard_normal((B, CP, T)).astype(np.float32), (rng.standard_normal((B, Q0, T)) * 1e-5).astype(np.float32)


@functools.lru_cache(maxsize=None)
def scales():
    return torch.tensor([SP, SQ, SP / 2, SQ * 2, SP * 4, SQ / 4], device=DEV)


@functools.lru_cache(maxsize=None)
def slab():
    return torch.empty(96 * 65536, device=DEV)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _planes(K, x, B, C, T, scale, mode, s2d=False):
    pl = torch.empty(2 * B * C * T, dtype=torch.float16, device=DEV)
    K.f16x3_split_activations(x, pl, B, C, T, scale_dev=scale, mode=mode | (K.X3_S2D if s2d else 0))
    return pl


def problem_scales(i):
    """(p scale, q scale) of problem i of a batch: slices of the device tensor and their values."""
    s = scales()
    return s[2 * i:2 * i + 1], s[2 * i + 1:2 * i + 2], float(s[2 * i]), float(s[2 * i + 1])


def run(K, *, B, T, Q0, taps, nsplit, mode=0, form='planes', dw_form='plain', seed=0, strided=False):
    """One launch.  taps: a list of tap lists, one per problem of the batch (problem i: operands of seed + i, its own scales).
    form: 'planes' (both operands as planes: the loop under test) or 'fp32' (fp32 operands: the register path).
    dw_form: 'plain' -- dw [ntaps][CP][Q0] per problem; 'block' -- the residual-half form: dw a column block from column 512 of a
    [CP][512 + Q0] matrix (lddw wider than the tile), q_total over columns (64, Q0 - 32).
    strided: p [B][CP][2 T] is the input of a stride-2 conv, the taps are the conv's e = j - pad_left of either sign; planes:
    space-to-depth planes, tap e = parity block e & 1 at row offset e >> 1; fp32: p_stride = 2."""
    outs = {}
    probs = []
    for i, tp in enumerate(taps):
        p, q = operands(B, 2 * T if strided else T, Q0, seed + i)
        if strided:
            q = operands(B, T, Q0, seed + i)[1]
        spd, sqd, _, _ = problem_scales(i)
        if dw_form == 'block':
            full = torch.zeros(CP, 512 + Q0, device=DEV)
            dw, outs['dw%d' % i] = full.view(-1)[512:], full
            tot = outs['tot%d' % i] = torch.zeros(Q0, device=DEV)
            pr = dict(dw=dw, q_total=tot)
        else:
            dw = outs['dw%d' % i] = torch.zeros(len(tp), CP, Q0, device=DEV)
            pr = dict(dw=dw)
        pd, qd = _dev(p), _dev(q)
        if form == 'fp32':
            pr.update(p=pd, q0=qd, taps=list(tp))
        elif strided:
            pr.update(p_planes=_planes(K, pd, B, CP, 2 * T, spd, mode, s2d=True), p_planes_KC=2 * CP // 8, p_tap_chunk=[(e & 1) * (CP // 8) for e in tp],
                      q_planes=_planes(K, qd, B, Q0, T, sqd, mode), taps=[e >> 1 for e in tp])
        else:
            pr.update(p_planes=_planes(K, pd, B, CP, T, spd, mode), q_planes=_planes(K, qd, B, Q0, T, sqd, mode), taps=list(tp))
        pr.update(p_scale=spd, q0_scale=sqd)
        probs.append(pr)
    common = dict(slab=slab(), B=B, T=T, Cp=CP, Q0=Q0, nsplit=nsplit, mode=mode)
    if dw_form == 'block':
        common.update(lddw=512 + Q0, total_cols=(64, Q0 - 32))
    if strided and form == 'fp32':
        common.update(p_stride=2, T_p=2 * T)
    K.f16x3_wgrad_batch(probs, **common)
    return outs


def _c(name, **kw):
    kw.setdefault('Q0', 512)
    kw.setdefault('B', 2)
    return name, kw


def cases():
    """[(name, kwargs of run())] in a fixed order."""
    c = []
    near = [-2, -1, 0]
    # K ranges of 1, 2, 3 pairs per block (2, 4, 6 stages against a ring of 4), and 3 pairs that cross the batch rows
    for T in (32, 64, 96):
        c.append(_c('short/T=%d' % T, T=T, taps=[near], nsplit=2))
    c.append(_c('short/T=32/B=3/one-block', B=3, T=32, Q0=256, taps=[near], nsplit=1))
    # every block one pair; nsplit above pairs_total is clamped to it
    c.append(_c('split/every-pair', B=3, T=96, Q0=256, taps=[near], nsplit=9))
    c.append(_c('split/clamped', T=64, Q0=256, taps=[near], nsplit=7))
    # one block walks 128 pairs: the ring wraps 64 times
    c.append(_c('long/T=2048', T=2048, Q0=256, taps=[[-1024, -512, 0]], nsplit=1))
    # taps: none, near, and dilations up to twice the row (2T: whole taps out of range -- zeros over slots that held data)
    for T in (64, 96):
        c.append(_c('taps/T=%d/1x1' % T, T=T, Q0=256, taps=[[0]], nsplit=2))
        for d in (4, T // 2, T, 2 * T):
            c.append(_c('taps/T=%d/d=%d' % (T, d), T=T, Q0=256 if T == 64 else 512, taps=[[-2 * d, -d, 0]], nsplit=1 if d == T else 3))
    # three problems with different dilations and scales in one launch
    c.append(_c('batch/3', B=3, T=96, taps=[[-8, -4, 0], [-192, -96, 0], [-2, -1, 0]], nsplit=4))
    c.append(_c('batch/3/Q0=256', T=64, Q0=256, taps=[[-64, -32, 0], [-2, -1, 0], [-256, -128, 0]], nsplit=2))
    # the residual-half form: a column block of a wider matrix, bias sums over a column range
    c.append(_c('block/3', B=3, T=96, Q0=256, taps=[[0], [0], [0]], nsplit=3, dw_form='block'))
    c.append(_c('block/Q0=512', T=64, taps=[[0]], nsplit=4, dw_form='block'))
    # rows that are no multiple of the 32-step pairs (legal only with both operands as planes): no fp32-operand twin
    for T in (40, 72):
        c.append(_c('ragged/T=%d' % T, T=T, taps=[[-8, -3, 0]], nsplit=2))
        c.append(_c('ragged/T=%d/B=3' % T, B=3, T=T, Q0=256, taps=[[-2 * T, -T // 2, 0]], nsplit=1))
    # stride-2 form: five taps e = j - 1 of either sign, parity blocks; T = 48 is no multiple of 32 either, 96 is
    for T in (48, 96):
        c.append(_c('strided/T=%d' % T, T=T, Q0=256, taps=[[-1, 0, 1, 2, 3]], nsplit=2, strided=True))
    # one bf16 plane per operand
    c.append(_c('bf16/T=96', T=96, taps=[[-8, -4, 0]], nsplit=2, mode=X3_BF16))
    c.append(_c('bf16/T=40', B=3, T=40, Q0=256, taps=[near], nsplit=2, mode=X3_BF16))
    c.append(_c('bf16/long', T=1024, Q0=256, taps=[[-512, -3, 0]], nsplit=1, mode=X3_BF16))
    return c


def has_fp32_twin(kw):
    """The fp32-operand launch needs T % 32 == 0 (T % 4 with p_stride 2) and, unstrided, shifts <= 0."""
    return kw['T'] % 32 == 0 or (kw.get('strided', False) and kw['T'] % 4 == 0)


def digest(outs):
    return {k: hashlib.sha256(v.detach().contiguous().cpu().numpy().tobytes()).hexdigest() for k, v in sorted(outs.items()) if k.startswith('dw')}


def all_digests(K):
    """{case: {output: sha256}}: dW of every case's planes-both launch."""
    out = {name: digest(run(K, **kw)) for name, kw in cases()}
    torch.cuda.synchronize()
    return out
