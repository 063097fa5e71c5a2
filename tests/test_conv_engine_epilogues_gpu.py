"""The fp32 conv engine (vqw_conv_gemm, vqw_wgrad_gemm) against the float64 reference of its ABI contract (tests/conv_ref.py):
every epilogue and option on ragged shapes, on every tile and tail-tile form, out of place and in place, with a 16-byte
aligned output start (vector rows where T_store % 4 == 0) and one shifted by a float (scalar rows).

Outputs and in-place operands are views into sentinel-filled buffers; conv_ref.check holds the written region to the
project's bars (2e-4 conv outputs, 1e-3 weight gradients, 2e-5 GATE, each of max(1, max |ref|)) and everything else -- guard
bands, the stride phase a launch does not address, the other columns of a wider matrix -- to bit-equality.

Every test records err / bar of its case (record_property 'err_over_bar', with 'family'); DESIGN 6 lists the maxima."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_ref as CR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
OFFSETS = (0, 1)          # floats between the 16-byte aligned guard band and the first element of every output


@functools.lru_cache(maxsize=4)          # the tiles of one case follow one another: one reference serves them all
def _conv_expected(name, off):
    c = [c for c in CR.conv_base_cases() if c['name'] == name][0]
    return CR.conv_expected(c, off)


@functools.lru_cache(maxsize=4)
def _wgrad_expected(name, off):
    c = [c for c in CR.wgrad_cases() if c['name'] == name][0]
    return CR.wgrad_expected(c, off)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run_conv(K, c, tile, off):
    """One case on one tile and one output alignment -> err / bar."""
    ins, bufs, exp = _conv_expected(c['name'], off)
    what = '%s (output start +%d floats)' % (CR.case_id(c, tile), off)
    dins = {n: _dev(a) for n, a in ins.items()}
    full = {id(b): _dev(b.full) for b in bufs.values()}
    views = {n: full[id(b)][b.lo:b.lo + b.n] for n, b in bufs.items()}
    for L in CR.launches_of(c):
        K.conv_gemm(**CR.conv_kwargs(c, L, tile), **CR.conv_operands(c, L, dins, views))
    got = {n: full[id(b)].cpu().numpy() for n, b in bufs.items()}
    ratio = CR.check(got, {n: e[0] for n, e in exp.items()}, {n: e[1] for n, e in exp.items()}, CR.bar_of(c), what)
    if c['epilogue'] == CR.EPI_GATE and c['save0'] and c['save1']:
        w = ~exp['out0'][1]
        d = np.abs(got['save0'][w].astype(np.float64) * got['save1'][w] - got['out0'][w])
        assert float(d.max()) <= 1e-6, '%s: saved tanh * sigmoid differs from out0 by %.3e' % (what, float(d.max()))
    return ratio


@pytest.mark.parametrize('c,tile', CR.conv_cases(), ids=[CR.case_id(c, t) for c, t in CR.conv_cases()])
def test_conv_epilogues_match_float64_reference(K, record_property, c, tile):
    ratio = max(_run_conv(K, c, tile, off) for off in OFFSETS)
    record_property('family', c['fam'])
    record_property('err_over_bar', ratio)


@pytest.mark.parametrize('c', CR.wgrad_cases(), ids=[c['name'] for c in CR.wgrad_cases()])
def test_wgrad_options_match_float64_reference(K, record_property, c):
    worst = 0.0
    for off in OFFSETS:
        ins, dw, (ref, keep) = _wgrad_expected(c['name'], off)
        dins = {n: _dev(a) for n, a in ins.items()}
        full = _dev(dw.full)
        K.wgrad_gemm(p=dins['p'], q0=dins['q0'], q1=dins.get('q1'), dw=full[dw.lo + c['dw_off']:dw.lo + dw.n], **CR.wgrad_kwargs(c))
        worst = max(worst, CR.check({'dw': full.cpu().numpy()}, {'dw': ref}, {'dw': keep}, CR.BAR_WGRAD,
                                    '%s (dw start +%d floats)' % (c['name'], off)))
    record_property('family', 'wgrad')
    record_property('err_over_bar', worst)


def _sentinels(n):
    return torch.full((n,), float(CR.SENTINEL), device=DEV)


@pytest.mark.parametrize('tile', [11, 12, 14, 10014])
def test_gate_on_an_mt1_tile_is_an_error_and_does_not_launch(K, tile):
    B, T, C, H = 2, 100, 16, 36
    out = _sentinels(B * H * T)
    with pytest.raises(RuntimeError, match='GATE needs an MT=2 tile'):
        K.conv_gemm(x0=_dev(CR.randn(1, B, C, T)), w=_dev(CR.randn(2, C * 2 * H)), out0=out, B=B, T_in=T, T_out=T, M=2 * H, C0=C,
                    taps=[0], epilogue=K.EPI_GATE, tile=tile)
    torch.cuda.synchronize()
    assert torch.equal(out, _sentinels(B * H * T)), 'the refused launch wrote to out0'


@pytest.mark.parametrize('opt', ['out_relu', 'scale', 'cond', 'save0', 'aux1', 'out1', 'ACCUM_SPLIT', 'MASK'])
def test_split_k_with_a_non_linear_epilogue_is_an_error_and_does_not_launch(K, opt):
    B, T, C, M = 2, 100, 64, 36
    out, other = _sentinels(B * M * T), _dev(CR.randn(3, B * M * T))
    kw = dict(out_relu=dict(out_relu=True), scale=dict(scale=_dev(CR.randn(4, M)), shift=_dev(CR.randn(5, M))),
              cond=dict(cond=_dev(CR.randn(6, B * M * 5)), cond_T=5), save0=dict(save0=other), aux1=dict(aux1=other),
              out1=dict(out1=other, M0=20), ACCUM_SPLIT=dict(epilogue=K.EPI_ACCUM_SPLIT, M0=M),
              MASK=dict(epilogue=K.EPI_MASK, aux0=other))[opt]
    before = other.clone()
    with pytest.raises(RuntimeError, match='split_k needs a plain STORE'):
        K.conv_gemm(x0=_dev(CR.randn(1, B, C, T)), w=_dev(CR.randn(2, C * M)), out0=out, B=B, T_in=T, T_out=T, M=M, C0=C,
                    taps=[0], split_k=3, **kw)
    torch.cuda.synchronize()
    assert torch.equal(out, _sentinels(B * M * T)) and torch.equal(other, before), 'the refused launch wrote to its outputs'
