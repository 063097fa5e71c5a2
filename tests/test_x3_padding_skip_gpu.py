"""The fp16x3 conv loop leaves out taps that multiply nothing but causal padding, and the gate conv's 128-row blocks read
bias + condition from a table in LDS (csrc/f16x3.h, f16x3_mainloop; csrc/f16x3_conv.hip, gate_f16x3_kernel).  Both must leave every
output bit where it was.

1. A launch that skips taps against a launch of the SAME build that cannot skip them: the same weights on an input whose padding
   is real -- P zero columns in front of every batch row (behind it for the input gradient, which reads ahead), P the smallest
   multiple of 256 that is at least (ks - 1) d.  Every tile that produces the original columns then lies a whole reach inside
   its row: all of its taps are live, the zeros are requested, read and multiplied.  The original columns must be torch.equal.
   B = 2, T = 512, ks = 3: d = 256 skips two taps in tile 0 and one in tile 1, d = 512 leaves tile 0 and 1 with one live tap,
   d = 300 puts a tap that is partly padding in tile 1 beside one that is skipped, d = 128 skips one tap of tile 0, d = 100 none
   (its tile 0 is partly padded in both shifted taps), d = 1 skips nothing.
2. A block whose K range shrinks to Cin / 16 = 4 steps -- as many as the ring has slots (256-row blocks) or one more (128-row
   blocks), all requested before the first wait -- against the plane-exact float64 reference of tests/x3_conv_ref.py, integer
   operands bit for bit and normal ones at that reference's bar: a slot left over from a skipped tap would show.
3. The gate conv's constants: bias and condition present or absent, 1 / 4 / 8 frames per column tile (ratio 256 / 64 / 32 at
   T = 512), both block heights, the training step's outputs and out0 + save0 + save1, against the float64 reference at its bar,
   and bit for bit against a second launch that gets fl32(bias + cond) as its condition and no bias.  Why those are the same
   bits: the kernel forms the fp32 sum bias + cond (an absent operand is +0) before anything else is added, numpy's float32
   sum is the same IEEE operation, and +0 + s = s for every s but -0 (no sum of these operands is a zero)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import x3_conv_ref as Rf  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F32 = np.float32
B, T, KS = 2, 512, 3
R_GATE = 128                   # the smallest the gate conv takes
R_OUT, CIN_OUT = 256, 64       # the smallest the out conv takes: 4 K steps per tap
DILATIONS = (1, 100, 128, 256, 300, 512)
MODES = Rf.MODES
SX, SW = 1.0, 256.0
STEP = ('save1', 'out_planes')
ALL = ('out0', 'save0', 'save1', 'out_planes')


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _pad_of(d):
    return -(-((KS - 1) * d) // 256) * 256


def test_the_padding_of_the_cases():
    assert [_pad_of(d) for d in DILATIONS] == [256, 256, 256, 512, 768, 1024]


def _rng(*key):
    return np.random.default_rng(Rf.seed_of('/'.join(str(k) for k in key), 'padding_skip'))


# ---------------------------------------------------------------------------------------------------- launches
def _gate_run(K, x, w, mode, dilation, subset, bias=None, cond=None, cond_T=0, ks=KS):
    """x [B][R][T'], w [ks][R][2R], cond [B][2R][cond_T] or None -> dict of the outputs asked for (planes as int16 [2][R/8][B][T'][8])."""
    Bb, R, Tt = x.shape
    xp = torch.empty(2 * Bb * R * Tt, dtype=torch.float16, device=DEV)
    wp = torch.empty(2 * ks * R * 2 * R, dtype=torch.float16, device=DEV)
    K.f16x3_split_activations(_dev(x), xp, Bb, R, Tt, scale=SX, mode=mode)
    K.f16x3_pack_gate_weights(_dev(w), wp, ks, R, 2 * R, SW, mode=mode)
    out = {n: torch.full((Bb, R, Tt), float('nan'), device=DEV) for n in subset if n != 'out_planes'}
    pl = torch.zeros(2 * R * Bb * Tt, dtype=torch.float16, device=DEV) if 'out_planes' in subset else None
    K.f16x3_gate_conv(xp=xp, wp=wp, out0=out.get('out0'), B=Bb, T=Tt, R=R, ks=ks, dilation=dilation, w_scale_inv=1.0 / (SX * SW),
                      bias=None if bias is None else _dev(bias), cond=None if cond is None else _dev(cond), cond_T=cond_T,
                      cond_bstride=2 * R * cond_T, save0=out.get('save0'), save1=out.get('save1'), out_planes=pl, mode=mode)
    torch.cuda.synchronize()
    if pl is not None:
        out['out_planes'] = pl.view(torch.int16).view(2, R // 8, Bb, Tt, 8)
    return out


def _out_run(K, x, w, mode, dilation, direction, ks, bias=None, net_in=None, planes=False):
    """x [B][Cin][T'], w [ks][Cin][R] -> dict(net_out [B][R][T'], planes int16 [2][R/8][B][T'][8])."""
    Bb, Cin, Tt = x.shape
    R = w.shape[2]
    xp = torch.empty(2 * Bb * Cin * Tt, dtype=torch.float16, device=DEV)
    wp = torch.empty(2 * ks * Cin * R, dtype=torch.float16, device=DEV)
    K.f16x3_split_activations(_dev(x), xp, Bb, Cin, Tt, scale=SX, mode=mode)
    K.f16x3_pack_weights(_dev(w), wp, ks * Cin, R, R, SW, mode=mode)
    net_out = torch.full((Bb, R, Tt), float('nan'), device=DEV)
    kw = {}
    pl = None
    if planes:
        pl = torch.zeros(2 * R * Bb * Tt, dtype=torch.float16, device=DEV)
        kw = dict(net_out_planes=pl, out_scale=torch.ones(1, device=DEV), out_amax=torch.zeros(1, dtype=torch.int32, device=DEV),
                  flag=torch.zeros(1, dtype=torch.int32, device=DEV))
    K.f16x3_out_conv(xp=xp, wp=wp, B=Bb, T=Tt, R=R, S=0, Cin=Cin, w_scale_inv=1.0 / (SX * SW), net_in=None if net_in is None else _dev(net_in),
                     net_out=net_out, bias=None if bias is None else _dev(bias), ks=ks, dilation=dilation, direction=direction, mode=mode, **kw)
    torch.cuda.synchronize()
    out = dict(net_out=net_out)
    if pl is not None:
        assert int(kw['flag'].item()) == 0
        out['planes'] = pl.view(torch.int16).view(2, R // 8, Bb, Tt, 8)
    return out


# ---------------------------------------------------------------------------------------------------- 1. skipped against multiplied
@functools.lru_cache(maxsize=None)
def _gate_operands():
    g = _rng('gate')
    ct = T // 64
    return dict(x=g.standard_normal((B, R_GATE, T)).astype(F32), w=(g.standard_normal((KS, R_GATE, 2 * R_GATE)) * (KS * R_GATE) ** -0.5).astype(F32),
                bias=(g.standard_normal(2 * R_GATE) * 0.3).astype(F32), cond=(g.standard_normal((B, 2 * R_GATE, ct)) * 0.3).astype(F32))


@pytest.mark.parametrize('subset', (ALL, STEP), ids=('all', 'step'))
@pytest.mark.parametrize('mode', [m for _, m in MODES], ids=[n for n, _ in MODES])
@pytest.mark.parametrize('d', DILATIONS)
def test_gate_conv_skipped_padding_equals_multiplied_zeros(K, d, mode, subset):
    o = _gate_operands()
    P, ct = _pad_of(d), T // 64
    a = _gate_run(K, o['x'], o['w'], mode, d, subset, o['bias'], o['cond'], ct)
    # the padded rows: P zero columns in front, and P / 64 frames of a condition of their own in front of the row's frames
    xz = np.concatenate([np.zeros((B, R_GATE, P), F32), o['x']], axis=2)
    cz = np.concatenate([_rng('gate cond pad', d).standard_normal((B, 2 * R_GATE, P // 64)).astype(F32), o['cond']], axis=2)
    z = _gate_run(K, xz, o['w'], mode, d, subset, o['bias'], cz, (T + P) // 64)
    for n in subset:
        got = z[n][:, :, :, P:] if n == 'out_planes' else z[n][:, :, P:]
        assert not (n != 'out_planes' and bool(torch.isnan(a[n]).any())), n + ': not written'
        assert torch.equal(got, a[n]), '%s: d = %d: the launch that skips padded taps differs from the one that multiplies the zeros' % (n, d)


@functools.lru_cache(maxsize=None)
def _dgrad_operands():
    g = _rng('dgrad')
    return dict(x=g.standard_normal((B, CIN_OUT, T)).astype(F32), w=(g.standard_normal((KS, CIN_OUT, R_OUT)) * (KS * CIN_OUT) ** -0.5).astype(F32),
                bias=(g.standard_normal(R_OUT) * 0.3).astype(F32), net_in=g.standard_normal((B, R_OUT, T)).astype(F32))


@pytest.mark.parametrize('planes', (False, True), ids=('fp32', 'fp32+planes'))
@pytest.mark.parametrize('mode', [m for _, m in MODES], ids=[n for n, _ in MODES])
@pytest.mark.parametrize('d', DILATIONS)
def test_input_gradient_skipped_padding_equals_multiplied_zeros(K, d, mode, planes):
    o = _dgrad_operands()
    P = _pad_of(d)
    a = _out_run(K, o['x'], o['w'], mode, d, -1, KS, o['bias'], o['net_in'], planes)
    xz = np.concatenate([o['x'], np.zeros((B, CIN_OUT, P), F32)], axis=2)
    nz = np.concatenate([o['net_in'], _rng('dgrad net_in pad', d).standard_normal((B, R_OUT, P)).astype(F32)], axis=2)
    z = _out_run(K, xz, o['w'], mode, d, -1, KS, o['bias'], nz, planes)
    assert not bool(torch.isnan(a['net_out']).any())
    assert torch.equal(z['net_out'][:, :, :T], a['net_out']), 'net_out: d = %d' % d
    if planes:
        assert torch.equal(z['planes'][:, :, :, :T], a['planes']), 'planes: d = %d' % d


# ---------------------------------------------------------------------------------------------------- 2. a K range of one tap
def _short_case(direction):
    return dict(kernel='out', epi=0, B=B, T=T, R=R_OUT, S=0, Cin=CIN_OUT, ks=KS, dilation=256, dir=direction, net_in='none', bias=True, xp_kc0=0)


@functools.lru_cache(maxsize=None)
def _short(direction, kind):
    g = _rng('short', direction, kind)
    if kind == 'ints':
        ins = dict(x=g.integers(-4, 5, (B, CIN_OUT, T)).astype(F32), w=g.integers(-2, 3, (KS, CIN_OUT, R_OUT)).astype(F32),
                   bias=(g.integers(-8, 9, R_OUT) / 8.0).astype(F32), sx=SX, sw=SW)
    else:
        ins = dict(x=g.standard_normal((B, CIN_OUT, T)).astype(F32), w=(g.standard_normal((KS, CIN_OUT, R_OUT)) * (KS * CIN_OUT) ** -0.5).astype(F32),
                   bias=(g.standard_normal(R_OUT) * 0.3).astype(F32), sx=SX, sw=SW)
    return ins, Rf.out_ref(_short_case(direction), ins)


@pytest.mark.parametrize('kind', Rf.KINDS)
@pytest.mark.parametrize('mode', [m for _, m in MODES], ids=[n for n, _ in MODES])
@pytest.mark.parametrize('direction', (1, -1), ids=('causal', 'dgrad'))
def test_one_live_tap_of_four_steps_against_float64(K, record_property, direction, mode, kind):
    """ks = 3, d = 256, Cin = 64: the first tile of a row (the last for the input gradient) keeps one tap = 4 K steps, its neighbour
    two = 8, against 12 everywhere else."""
    ins, ref = _short(direction, kind)
    got = _out_run(K, ins['x'], ins['w'], mode, 256, direction, KS, ins['bias'])['net_out'].cpu().numpy()
    worst = Rf.compare(got, ref['net_out'], ref['bar_net'], kind, 'one live tap, dir %d' % direction)
    record_property('worst_fraction', worst)


# ---------------------------------------------------------------------------------------------------- 3. the table of constants
EPI_KS, EPI_D = 2, 1


def _epi_case(bias, ratio, subset):
    ct = T // ratio if ratio else 0
    return dict(kernel='gate', B=B, T=T, R=R_GATE, ks=EPI_KS, dilation=EPI_D, cond_T=ct, cond_bstride=2 * R_GATE * ct, bias=bias, subset=subset,
                out_planes_kc0=0, out_planes_KC=0)


@functools.lru_cache(maxsize=None)
def _epi_operands():
    g = _rng('epilogue table')
    d = dict(x=g.standard_normal((B, R_GATE, T)).astype(F32), w=(g.standard_normal((EPI_KS, R_GATE, 2 * R_GATE)) * (EPI_KS * R_GATE) ** -0.5).astype(F32),
             bias=(g.standard_normal(2 * R_GATE) * 0.3).astype(F32), sx=SX, sw=SW, winv=1.0 / (SX * SW))
    for ratio in (32, 64, 256):
        d['cond%d' % ratio] = (g.standard_normal((B, 2 * R_GATE, T // ratio)) * 0.3).astype(F32)
    return d


@functools.lru_cache(maxsize=None)
def _epi_reference(bias, ratio):
    o = _epi_operands()
    ins = dict(o, cond=o['cond%d' % ratio] if ratio else None)
    return Rf.gate_ref(_epi_case(bias, ratio, ALL), ins)


@pytest.mark.parametrize('subset', (STEP, ('out0', 'save0', 'save1')), ids=('step', 'out0+save0+save1'))
@pytest.mark.parametrize('mode', [m for _, m in MODES], ids=[n for n, _ in MODES])
@pytest.mark.parametrize('ratio', (0, 32, 64, 256), ids=('no cond', 'ratio 32', 'ratio 64', 'ratio 256'))
@pytest.mark.parametrize('bias', (True, False), ids=('bias', 'no bias'))
def test_gate_conv_constants(K, record_property, bias, ratio, mode, subset):
    o, ref = _epi_operands(), _epi_reference(bias, ratio)
    ct = T // ratio if ratio else 0
    bv, cv = (o['bias'] if bias else None), (o['cond%d' % ratio] if ratio else None)
    got = _gate_run(K, o['x'], o['w'], mode, EPI_D, subset, bv, cv, ct, ks=EPI_KS)
    worst = 0.0
    for n in subset:
        if n != 'out_planes':
            worst = max(worst, Rf.compare(got[n].cpu().numpy(), ref[n], ref['bar_' + n], 'normal', n))
    if 'out_planes' in subset:      # no fp32 out0 beside them: the decoded planes within the bar of out0 and the planes' own resolution
        img = got['out_planes'].cpu().numpy().view(np.uint16).reshape(2, R_GATE // 8, B * T, 8)
        dec = Rf.decode_planes(img, 0, R_GATE, B, T)
        worst = max(worst, Rf.compare(dec, ref['out0'], ref['bar_out0'] + Rf.SPLIT_REL * np.abs(ref['out0']) + Rf.F16_HALF_STEP, 'normal', 'decoded planes'))
    record_property('worst_fraction', worst)
    if not bias:
        return
    # bias folded into the condition on the host (module docstring): with no condition, one frame per row that holds the bias
    if ratio:
        folded = (cv + bv[None, :, None]).astype(F32)
    else:
        folded, ct = np.ascontiguousarray(np.broadcast_to(bv[None, :, None], (B, 2 * R_GATE, 1))).astype(F32), 1
    assert not (folded == 0).any()
    twin = _gate_run(K, o['x'], o['w'], mode, EPI_D, subset, None, folded, ct, ks=EPI_KS)
    for n in subset:
        assert torch.equal(twin[n], got[n]), n + ': bias + cond summed by the kernel and on the host give different bits'
