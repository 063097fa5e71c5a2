"""The bf16 engine's contractions (VQW_X3_BF16: the BF = true instantiations of csrc/f16x3_*.hip) against a bf16-rounded
float64 reference.

A bf16 x bf16 product is exact in fp32, so with operands rounded to bf16 (round to nearest even, x3_ref.bf16_round) a kernel differs
from an exact evaluation only by its fp32 accumulation and its fp32 epilogue -- the error sources the fp16x3 kernels meet at 1e-6 to
2e-5.  Every bar below is the bar the fp16x3 test of the same kernel and shape has in test_kernels_gpu.py (none was derived from a
measurement of the bf16 kernels); test_x3_ref_cpu.py shows that a kernel which truncates, forgets to round or reads across the start
of a batch row lies at least 10 bars away.

The operand planes come from vqw_f16x3_split_activations / vqw_f16x3_pack_* with the same mode (their images are pinned by
test_x3_range_gpu.py); the reference rounds the fp32 inputs itself and never reads planes back.  Plane buffers are allocated at
the bf16 size -- ONE plane -- filled with 0x7fc0 (a NaN as bf16 and as fp16) and followed by a guard of the same pattern as long as
the plane: a kernel that reads a second plane gets NaNs, one that writes a second plane breaks the guard."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import x3_ref as X  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BF, HALF = X.X3_BF16, X.X3_HALF_BLOCKS
NAN16 = 0x7fc0
SIGMOID_MIN_NORMAL = 1.17549435e-38

both_heights = pytest.mark.parametrize('half', [0, 1], ids=['blocks256', 'blocks128'])


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def image_of(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


class Planes:
    """n halves of one bf16 plane image (`.t`, what the kernels are given) inside a buffer that goes on for a guard of n more
    halves, all 0x7fc0."""

    def __init__(self, n):
        self.n = n
        self.full = torch.full((2 * n,), NAN16, dtype=torch.int16, device=DEV).view(torch.float16)
        self.t = self.full[:n]

    def image(self):
        return image_of(self.t)

    def check_guard(self, what):
        assert (image_of(self.full[self.n:]) == NAN16).all(), '%s: something was written behind the one bf16 plane' % what


def poisoned(*shape):
    return torch.full(shape, float('nan'), device=DEV)


def rd(x, scale=1.0):
    """float64 device tensor of bf16(scale * x) / scale, rounded by x3_ref on the host (scale: a power of two)."""
    a = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x, np.float32)
    return dev(X.bf16_round(X.scaled(a, scale))) / float(np.float32(scale))


def shift_t(x, sh, leak=False):
    """x [B][C][T] read at t + sh (either sign), zero outside [0, T) of the batch row.  leak: the flat (batch, time) row is read
    instead wherever it exists (a kernel that forgets the check)."""
    B, C, T = x.shape
    if leak:
        flat = x.permute(1, 0, 2).reshape(C, B * T)
        out = torch.zeros_like(flat)
        if sh >= 0:
            out[:, :B * T - sh] = flat[:, sh:]
        else:
            out[:, -sh:] = flat[:, :B * T + sh]
        return out.reshape(C, B, T).permute(1, 0, 2)
    out = torch.zeros_like(x)
    if sh >= 0 and sh < T:
        out[:, :, :T - sh] = x[:, :, sh:]
    elif sh < 0 and -sh < T:
        out[:, :, -sh:] = x[:, :, :T + sh]
    return out


def conv64(xr, wr, shifts, leak=False):
    """out[b][m][t] = sum_j sum_c xr[b][c][t + shifts[j]] wr[j][c][m] in float64."""
    out = torch.zeros(xr.shape[0], wr.shape[2], xr.shape[2], dtype=torch.float64, device=DEV)
    for j, sh in enumerate(shifts):
        out += torch.einsum('bct,cm->bmt', shift_t(xr, sh, leak), wr[j])
    return out


def wgrad64(pr, qr, shifts):
    """dw[j][c][o] = sum_{b,t} pr[b][c][t + shifts[j]] qr[b][o][t] in float64."""
    return torch.stack([torch.einsum('bct,bot->co', shift_t(pr, sh), qr) for sh in shifts])


def plane_image(x, scale=1.0, kc0=0, KC=0, into=None):
    """The bf16 plane image (flat uint16) of the fp32 device tensor x [B][C][T]."""
    return X.act_planes(x.detach().cpu().numpy(), scale, kc0=kc0, KC=KC, mode=BF, into=into).reshape(-1)


def rel_err(got, want):
    return float((got.double() - want).abs().max()) / float(want.abs().max())


# ----------------------------------------------------------------------------- gate conv
@both_heights
@pytest.mark.parametrize('B,T,R,ks,d', [(2, 512, 128, 3, 1), (2, 512, 128, 2, 7), (1, 1024, 256, 3, 64), (2, 768, 128, 3, 300)])
def test_gate_conv_bf16_matches_rounded_fp64(K, half, B, T, R, ks, d):
    """vqw_f16x3_gate_conv with one bf16 plane per operand: tanh * sigmoid, tanh and sigmoid over the WHOLE tensor against
    tanh / sigmoid of the float64 pre-activation of bf16(x) and bf16(256 w) (+ bias + the upsampled condition), 2e-5 absolute (the bar
    of test_gate_conv_f16x3_matches_fp32_engine); taps before t = 0, a dilation beyond the tile and one beyond half the signal, both
    kernel sizes.  The gated planes are bf16(out0) bit for bit, alone and as the middle layer of a three-layer buffer whose other
    chunks keep their bits, with and without the fp32 out0."""
    md = BF | (HALF if half else 0)
    x, w, bias, cond = X.gate_case(B, T, R, ks, d)
    cond_T = cond.shape[2]
    xd, wd, bd, cd = dev(x), dev(w), dev(bias), dev(cond)
    taps = [-(ks - 1 - j) * d for j in range(ks)]
    pre = conv64(rd(x), rd(w, 256.0), taps)
    if (T, R) == (512, 128):      # the device evaluation of the reference is the host's (the one test_x3_ref_cpu.py probes)
        assert np.abs(pre.cpu().numpy() - X.conv_bf16(x, w, taps, 1.0, 256.0)).max() <= 1e-12
    pre = pre + bd.double()[None, :, None] + cd.double().repeat_interleave(T // cond_T, dim=2)
    w_th, w_sg = torch.tanh(pre[:, :R]), torch.sigmoid(pre[:, R:])
    xp, wp, op = Planes(B * R * T), Planes(ks * R * 2 * R), Planes(B * R * T)
    K.f16x3_split_activations(xd, xp.t, B, R, T, mode=md)
    K.f16x3_pack_gate_weights(wd, wp.t, ks, R, 2 * R, 256.0, mode=md)
    out, th, sg = poisoned(B, R, T), poisoned(B, R, T), poisoned(B, R, T)
    args = dict(xp=xp.t, wp=wp.t, bias=bd, cond=cd, cond_T=cond_T, B=B, T=T, R=R, ks=ks, dilation=d, w_scale_inv=1.0 / 256.0, mode=md)
    K.f16x3_gate_conv(out0=out, save0=th, save1=sg, out_planes=op.t, **args)
    for got, want, nm in ((out, w_th * w_sg, 'gated'), (th, w_th, 'tanh'), (sg, w_sg, 'sigmoid')):
        err = float((got.double() - want).abs().max())
        print('%s: max abs err %.3e' % (nm, err))
        assert err <= 2e-5, '%s differs from the rounded float64 evaluation by %.3e' % (nm, err)
    first = op.image()
    assert np.array_equal(first, plane_image(out)), 'gated planes are not bf16(out0)'
    for pl, nm in ((xp, 'x planes'), (wp, 'weight planes'), (op, 'gated planes')):
        pl.check_guard(nm)
    # planes + sigmoid only (no fp32 out0)
    op2, sg2 = Planes(B * R * T), poisoned(B, R, T)
    K.f16x3_gate_conv(out0=None, save1=sg2, out_planes=op2.t, **args)
    assert np.array_equal(op2.image(), first) and torch.equal(sg2, sg)
    op2.check_guard('gated planes without out0')
    # the middle layer of three side by side
    kc = R // 8
    for with_out in (True, False):
        wide, out3, sg3 = Planes(3 * B * R * T), poisoned(B, R, T), poisoned(B, R, T)
        K.f16x3_gate_conv(out0=out3 if with_out else None, save1=sg3, out_planes=wide.t, out_planes_kc0=kc, out_planes_KC=3 * kc, **args)
        img = wide.image().reshape(3, kc * B * T * 8)
        assert np.array_equal(img[1], first), 'planes at chunk kc0 differ (out0: %s)' % with_out
        assert (img[0] == NAN16).all() and (img[2] == NAN16).all(), 'the neighbouring layers were touched'
        wide.check_guard('wide gated planes')
        assert torch.equal(sg3, sg) and (not with_out or torch.equal(out3, out))


# ----------------------------------------------------------------------------- skip + residual conv
@both_heights
def test_out_conv_bf16_matches_rounded_fp64(K, half):
    """vqw_f16x3_out_conv epi 0 on the gate kernel's bf16 planes: skip accumulated onto a random start and net = net_in + ... against
    the float64 contraction of bf16(gated) with bf16(64 w), 2e-5 of the tensor max (test_out_conv_f16x3_matches_fp32_engine's bar);
    net_out_planes = bf16(net_out) bit for bit; the residual half alone (S = 0); the skip path as one contraction over three layers'
    gated planes side by side (R = 0, Cin = 3 * 256) and over the middle layer alone (xp_kc0 != 0)."""
    md = BF | (HALF if half else 0)
    B, T, R, S, ks, d = 2, 512, 256, 512, 3, 2
    rng = np.random.RandomState(77 + T)
    x = rng.standard_normal((B, R, T)).astype(np.float32)
    wg = (rng.standard_normal((ks, R, 2 * R)) * 0.05).astype(np.float32)
    wo = (rng.standard_normal((R, S + R)) * 0.08).astype(np.float32)
    bo = (rng.standard_normal(S + R) * 0.3).astype(np.float32)
    skip0 = rng.standard_normal((B, S, T)).astype(np.float32)
    xd, wgd, wod, bod = dev(x), dev(wg), dev(wo), dev(bo)
    xp, wgp, gp, wop = Planes(B * R * T), Planes(ks * R * 2 * R), Planes(B * R * T), Planes(R * (S + R))
    gated = poisoned(B, R, T)
    K.f16x3_split_activations(xd, xp.t, B, R, T, mode=md)
    K.f16x3_pack_gate_weights(wgd, wgp.t, ks, R, 2 * R, 256.0, mode=md)
    K.f16x3_gate_conv(xp=xp.t, wp=wgp.t, out0=gated, out_planes=gp.t, B=B, T=T, R=R, ks=ks, dilation=d, w_scale_inv=1.0 / 256.0, mode=md)
    assert np.array_equal(gp.image(), plane_image(gated))
    lin = torch.einsum('cm,bct->bmt', rd(wo, 64.0), rd(gated)) + bod.double()[None, :, None]
    want_skip, want_net = dev(skip0).double() + lin[:, :S], xd.double() + lin[:, S:]
    K.f16x3_pack_weights(wod, wop.t, R, S + R, S + R, 64.0, mode=md)
    skip, net, npl = dev(skip0), poisoned(B, R, T), Planes(B * R * T)
    K.f16x3_out_conv(xp=gp.t, wp=wop.t, bias=bod, skip=skip, net_in=xd, net_out=net, net_out_planes=npl.t, B=B, T=T, R=R, S=S,
                     w_scale_inv=1.0 / 64.0, mode=md)
    for got, want, nm in ((skip, want_skip, 'skip'), (net, want_net, 'net')):
        err = rel_err(got, want)
        print('%s: %.3e of max' % (nm, err))
        assert err <= 2e-5, '%s differs from the rounded float64 evaluation by %.3e of max' % (nm, err)
    assert np.array_equal(npl.image(), plane_image(net)), 'net planes are not bf16(net_out)'
    for pl, nm in ((gp, 'gated planes'), (wop, 'weight planes'), (npl, 'net planes')):
        pl.check_guard(nm)
    # S = 0: the residual half alone (the matrix's columns S.. through ldw)
    wrp, net2, npl2 = Planes(R * R), poisoned(B, R, T), Planes(B * R * T)
    K.f16x3_pack_weights(wod.view(-1)[S:], wrp.t, R, R, S + R, 64.0, mode=md)
    K.f16x3_out_conv(xp=gp.t, wp=wrp.t, bias=bod[S:].contiguous(), net_in=xd, net_out=net2, net_out_planes=npl2.t, B=B, T=T, R=R, S=0,
                     w_scale_inv=1.0 / 64.0, mode=md)
    err = rel_err(net2, want_net)
    assert err <= 2e-5, 'S = 0: net differs by %.3e of max' % err
    assert np.array_equal(npl2.image(), plane_image(net2))
    npl2.check_guard('net planes, S = 0')
    # R = 0: skip += sum_l W_l g_l over three layers' gated planes side by side, and the middle layer alone
    kc = R // 8
    gs = [(rng.standard_normal((B, R, T)) * 0.3).astype(np.float32) for _ in range(3)]
    ws = (rng.standard_normal((3 * R, S)) * 0.08).astype(np.float32)
    gall, wsp, wmid = Planes(3 * B * R * T), Planes(3 * R * S), Planes(R * S)
    for i in range(3):
        K.f16x3_split_activations(dev(gs[i]), gall.t, B, R, T, kc0=i * kc, KC=3 * kc, mode=md)
    K.f16x3_pack_weights(dev(ws), wsp.t, 3 * R, S, S, 64.0, mode=md)
    K.f16x3_pack_weights(dev(ws[R:2 * R]), wmid.t, R, S, S, 64.0, mode=md)
    wsr = rd(ws, 64.0)
    parts = [torch.einsum('cm,bct->bmt', wsr[i * R:(i + 1) * R], rd(gs[i])) for i in range(3)]
    skip3 = dev(skip0)
    K.f16x3_out_conv(xp=gall.t, wp=wsp.t, skip=skip3, B=B, T=T, R=0, S=S, Cin=3 * R, xp_KC=3 * kc, w_scale_inv=1.0 / 64.0, mode=md)
    err = rel_err(skip3, dev(skip0).double() + parts[0] + parts[1] + parts[2])
    assert err <= 2e-5, 'R = 0 over three layers: skip differs by %.3e of max' % err
    skip1 = dev(skip0)
    K.f16x3_out_conv(xp=gall.t, wp=wmid.t, skip=skip1, B=B, T=T, R=0, S=S, Cin=R, xp_kc0=kc, xp_KC=3 * kc, w_scale_inv=1.0 / 64.0, mode=md)
    err = rel_err(skip1, dev(skip0).double() + parts[1])
    assert err <= 2e-5, 'R = 0, middle layer (xp_kc0 = %d): skip differs by %.3e of max' % (kc, err)
    gall.check_guard('three layers of gated planes')


# ----------------------------------------------------------------------------- input gradient
@both_heights
@pytest.mark.parametrize('lift', [2.0 ** 20, 1.0], ids=['lift2^20', 'nolift'])
@pytest.mark.parametrize('B,T,d,top', [(2, 512, 3, False), (2, 768, 300, True)])
def test_dgrad_bf16_matches_rounded_fp64(K, half, B, T, d, top, lift):
    """The gate conv's input gradient (vqw_f16x3_out_conv, ks = 3, dir < 0: reads AHEAD, zero behind the end of a batch row) on
    gradients of 3e-6, with the 2^20 lift the model applies to its gradient planes and with none (bf16 has fp32's exponent: both must
    meet the bar): 2e-5 of the tensor max (test_dgrad_f16x3_matches_fp32_engine's bar), and the last 2 d + 1 steps of every batch row
    -- where taps run out one by one -- once more on their own (an evaluation that reads on into the next row is shown to differ
    there by more than 10 bars)."""
    md = BF | (HALF if half else 0)
    R, ks = 256, 3
    rng = np.random.RandomState(5 + T + d)
    dpre = (rng.standard_normal((B, 2 * R, T)) * 3e-6).astype(np.float32)
    wt = (rng.standard_normal((ks, 2 * R, R)) * 0.05).astype(np.float32)
    dnet = (rng.standard_normal((B, R, T)) * 1e-5).astype(np.float32)
    ahead = [(ks - 1 - j) * d for j in range(ks)]
    dr, wr = rd(dpre, lift), rd(wt, 256.0)
    base = 0.0 if top else dev(dnet).double()
    want = conv64(dr, wr, ahead) + base
    dp, wp = Planes(B * 2 * R * T), Planes(ks * 2 * R * R)
    K.f16x3_split_activations(dev(dpre), dp.t, B, 2 * R, T, scale=lift, mode=md)
    K.f16x3_pack_weights(dev(wt), wp.t, ks * 2 * R, R, R, 256.0, mode=md)
    out = poisoned(B, R, T)
    K.f16x3_out_conv(xp=dp.t, Cin=2 * R, ks=ks, dilation=d, direction=-1, wp=wp.t, net_in=None if top else dev(dnet), net_out=out,
                     B=B, T=T, R=R, S=0, w_scale_inv=1.0 / (256.0 * lift), mode=md)
    top_max = float(want.abs().max())
    err = float((out.double() - want).abs().max()) / top_max
    print('input gradient: %.3e of max' % err)
    assert err <= 2e-5, 'input gradient differs from the rounded float64 evaluation by %.3e of max' % err
    n = min(2 * d + 1, T)
    tail = float((out.double() - want)[:, :, T - n:].abs().max()) / top_max
    assert tail <= 2e-5, 'last %d steps of the batch rows: %.3e of max' % (n, tail)
    leaked = conv64(dr, wr, ahead, leak=True) + base
    assert float((leaked - want)[:-1, :, T - n:].abs().max()) / top_max >= 10 * 2e-5
    assert float((leaked - want)[-1].abs().max()) <= 1e-12 * top_max      # (nothing lies behind the last row)
    # the very last step has one tap left
    last = torch.einsum('bc,cm->bm', dr[:, :, T - 1], wr[ks - 1]) + (0.0 if top else dev(dnet).double()[:, :, T - 1])
    assert float((out[:, :, T - 1].double() - last).abs().max()) / top_max <= 2e-5
    dp.check_guard('gradient planes')
    wp.check_guard('weight planes')


# ----------------------------------------------------------------------------- gate backward
@both_heights
def test_gate_backward_bf16_three_aux0_forms(K, half):
    """vqw_f16x3_out_conv epi 1 on one bf16 plane per operand, the construction of test_gate_backward_f16x3_from_tanh_or_from_gated
    (sigmoids that are exactly zero, denormal, and the smallest normal numbers): dpre = {dg sg (1 - th^2), dg th sg (1 - sg)} with
    dg = bf16(64 W)^T bf16(2^28 [dskip; dnet]) in float64, aux0 as fp32 tanh (1e-6 of max), as fp32 tanh * sigmoid (2e-6) and as the
    gated PLANES the forward pass wrote (3e-6) -- the bars of the fp16x3 test.  In the planes form the reference forms tanh from
    bf16_round(gated) / sg: single-plane gated storage MEANS the rounded value, so that is the exact result of the operation and not an
    error of the kernel (sigmoids below the smallest normal number give a zero filter gradient, as the header says).  The planes
    written are bf16(plane_scale * out_scale * dpre) bit for bit, with or without the fp32 dpre."""
    md = BF | (HALF if half else 0)
    B, T, R, S = 2, 512, 256, 256
    gen = torch.Generator().manual_seed(51)
    dcat = (torch.randn(B, S + R, T, generator=gen) * 1e-5).to(DEV)
    w = (torch.randn(S + R, R, generator=gen) * 0.05).to(DEV)
    xf, xg = torch.randn(B, R, T, generator=gen).to(DEV) * 2, torch.randn(B, R, T, generator=gen).to(DEV) * 3
    xg[:, ::7, ::5] = -200.0                                              # sigmoid == 0 exactly
    xg[:, 3::7, 1::5] = -88.0                                             # a denormal sigmoid
    xg[:, 5::7, 2::5] = -87.0                                             # the smallest normal numbers
    th, sg = torch.tanh(xf), torch.sigmoid(xg)
    assert 0 < float(sg[:, 3::7, 1::5].max()) < SIGMOID_MIN_NORMAL and float(sg[:, ::7, ::5].max()) == 0.0
    gated = th * sg
    sc = torch.tensor([2.0 ** 28, 64.0, 2.0 ** 26], device=DEV)
    gr, wp = Planes(B * (S + R) * T), Planes((S + R) * R)
    K.f16x3_split_activations(dcat, gr.t, B, S + R, T, scale_dev=sc[0:1], mode=md)
    K.f16x3_pack_weights(w, wp.t, S + R, R, R, 1.0, scale_dev=sc[1:2], mode=md)
    dg = torch.einsum('kc,bkt->bct', rd(w, 64.0), rd(dcat, 2.0 ** 28))
    th64, sg64 = th.double(), sg.double()
    want_fp32 = torch.cat([dg * sg64 * (1 - th64 ** 2), dg * th64 * sg64 * (1 - sg64)], 1)
    g_r = rd(gated)
    ff = torch.where(sg >= SIGMOID_MIN_NORMAL, sg64 - g_r * g_r / sg64.clamp_min(1e-300), torch.zeros_like(sg64))
    want_planes = torch.cat([dg * ff, dg * g_r * (1 - sg64)], 1)
    kc = R // 8
    gpl = Planes(3 * B * R * T)                # the gated planes as the middle layer of three side by side
    K.f16x3_split_activations(gated, gpl.t, B, R, T, kc0=kc, KC=3 * kc, mode=md)
    common = dict(epi=1, xp=gr.t, Cin=S + R, wp=wp.t, aux1=sg, B=B, T=T, R=R, S=0, w_scale_inv=1.0, x_scale=sc[0:1], w_scale=sc[1:2],
                  out_scale=sc[2:3], mode=md)
    from_planes = dict(aux0_planes=gpl.t, aux0_KC=3 * kc, aux0_kc0=kc, aux0_is_gated=True)
    for nm, kw, want, bar in (('tanh', dict(aux0=th), want_fp32, 1e-6), ('gated', dict(aux0=gated, aux0_is_gated=True), want_fp32, 2e-6),
                              ('gated planes', from_planes, want_planes, 3e-6)):
        dpre, planes = poisoned(B, 2 * R, T), Planes(B * 2 * R * T)
        K.f16x3_out_conv(net_out=dpre, net_out_planes=planes.t, **common, **kw)
        assert torch.isfinite(dpre).all()
        err = rel_err(dpre, want)
        print('aux0 = %s: %.3e of max' % (nm, err))
        assert err <= bar, 'aux0 = %s: %.3e of max' % (nm, err)
        assert np.array_equal(planes.image(), plane_image(dpre, 2.0 ** 26)), 'aux0 = %s: planes are not bf16(2^26 dpre)' % nm
        planes.check_guard('dpre planes')
    planes2 = Planes(B * 2 * R * T)            # planes only: no fp32 dpre at all
    K.f16x3_out_conv(net_out=None, net_out_planes=planes2.t, **common, **from_planes)
    assert np.array_equal(planes2.image(), planes.image())
    for pl, nm in ((planes2, 'dpre planes without dpre'), (gr, 'gradient planes'), (wp, 'weight planes'), (gpl, 'gated planes')):
        pl.check_guard(nm)


# ----------------------------------------------------------------------------- head convs
def _no_negative_zero(img):
    return np.where(img == 0x8000, 0, img)


@both_heights
def test_head_conv_bf16_epilogue_options(K, half):
    """vqw_f16x3_out_conv epi 2 on bf16 planes, the shape and options of test_head_conv_f16x3_epilogue_options: mask * (net_in + W x +
    bias + strided upsampled condition) in place over the mask source, against float64 of bf16(4 x) and bf16(64 w) at that test's 3e-6
    of max; the planes are bf16(16 relu(out)) bit for bit (the sign of a zero is not part of the contract), the max-abs report, a
    clean range flag; then the plain form."""
    md = BF | (HALF if half else 0)
    B, T, Cin, M, Tz = 2, 512, 512, 256, 8
    gen = torch.Generator().manual_seed(41)
    x = torch.randn(B, Cin, T, generator=gen).to(DEV)
    w = (torch.randn(Cin, M, generator=gen) * 0.05).to(DEV)
    bias = torch.randn(M, generator=gen).to(DEV)
    cond = torch.randn(B, M + 3, Tz, generator=gen).to(DEV)            # batch stride wider than the rows read
    ni = torch.randn(B, M, T, generator=gen).to(DEV)
    mask_src = torch.randn(B, M, T, generator=gen).to(DEV)
    sc = torch.tensor([4.0, 64.0, 16.0], device=DEV)
    xp, wp = Planes(B * Cin * T), Planes(Cin * M)
    K.f16x3_split_activations(x, xp.t, B, Cin, T, scale_dev=sc[0:1], mode=md)
    K.f16x3_pack_weights(w, wp.t, Cin, M, M, 1.0, scale_dev=sc[1:2], mode=md)
    lin = torch.einsum('cm,bct->bmt', rd(w, 64.0), rd(x, 4.0)) + bias.double()[None, :, None]
    up = cond[:, :M].double().repeat_interleave(T // Tz, dim=2)
    want = (mask_src > 0).double() * (ni.double() + lin + up)
    out = mask_src.clone()                                             # in place over the mask source
    planes = Planes(B * M * T)
    amax, flag = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    scales = dict(w_scale_inv=1.0, x_scale=sc[0:1], w_scale=sc[1:2], out_scale=sc[2:3])
    K.f16x3_out_conv(epi=2, xp=xp.t, Cin=Cin, wp=wp.t, bias=bias, net_in=ni, net_out=out, aux0=out, cond=cond, cond_T=Tz,
                     cond_bstride=(M + 3) * Tz, net_out_planes=planes.t, relu_planes=True, B=B, T=T, R=M, S=0, out_amax=amax, flag=flag,
                     mode=md, **scales)
    err = rel_err(out, want)
    print('masked head: %.3e of max' % err)
    assert err <= 3e-6, 'masked form: %.3e of max' % err
    assert np.array_equal(_no_negative_zero(planes.image()), _no_negative_zero(plane_image(torch.relu(out), 16.0)))
    assert abs(amax.view(torch.float32).item() - torch.relu(want).max().item()) <= 3e-6 * want.abs().max().item()
    assert flag.item() == 0
    planes.check_guard('relu planes')
    # plain form: no mask, no net_in, no condition, planes without relu
    out2, planes2 = poisoned(B, M, T), Planes(B * M * T)
    K.f16x3_out_conv(epi=2, xp=xp.t, Cin=Cin, wp=wp.t, bias=bias, net_out=out2, net_out_planes=planes2.t, B=B, T=T, R=M, S=0, mode=md, **scales)
    err = rel_err(out2, lin)
    assert err <= 3e-6, 'plain form: %.3e of max' % err
    assert np.array_equal(planes2.image(), plane_image(out2, 16.0))
    for pl, nm in ((planes2, 'planes'), (xp, 'x planes'), (wp, 'weight planes')):
        pl.check_guard(nm)


# ----------------------------------------------------------------------------- weight gradients
def wgrad_bar(want_update, dw0_max):
    """The bar of test_wgrad_f16x3_matches_fp64: 2e-6 of the largest update + 1e-6 of the largest value accumulated into."""
    return 2e-6 * max(float(want_update.abs().max()), 1e-30) + 1e-6 * dw0_max


def check_q_sums(tot, tot0, seg, want_q, cols, seg_len, what):
    """q_total / q_seg against float64 sums of want_q [B][Q][T] in the bound form of test_wgrad_f16x3_matches_fp64: per column
    1e-5 sum |q| (+ 2e-6 of the largest value accumulated into) for the totals, 1e-5 * 32 max |q| per 32 steps of a segment."""
    B, Q, T = want_q.shape
    want_tot = tot0.double().clone()
    want_tot[cols[0]:cols[1]] += want_q.sum((0, 2))[cols[0]:cols[1]]
    bound = 1e-5 * want_q.abs().sum((0, 2)) + 2e-6 * float(tot0.abs().max())
    bad = (tot.double() - want_tot).abs() > bound
    assert not bool(bad.any()), '%s: %d column totals outside 1e-5 sum |q|' % (what, int(bad.sum()))
    want_seg = want_q.reshape(B, Q, T // seg_len, seg_len).sum(-1)
    err = float((seg[:, :Q].double() - want_seg).abs().max())
    assert err <= 1e-5 * float(want_q.abs().max()) * 32 * (seg_len / 32.0), '%s: segment sums off by %.3e' % (what, err)
    assert float(seg[:, Q:].abs().max()) == 0.0 if seg.shape[1] > Q else True, '%s: the slack between the batch rows was written' % what


@pytest.mark.parametrize('B,T,d,Q1,scaled', [(2, 512, 1, 256, False), (2, 512, 2, 0, True), (3, 544, 3, 256, True), (1, 512, 512, 0, False)])
def test_wgrad_bf16_matches_rounded_fp64(K, B, T, d, Q1, scaled):
    """vqw_f16x3_wgrad with in-register bf16 conversions (split4<BF>) against the float64 einsum of the rounded shifted p and the
    rounded q, accumulated onto a random dw, at the bar of test_wgrad_f16x3_matches_fp64 (2e-6 of the update + 1e-6 of max |dw0|):
    taps before t = 0, shifts that are no multiples of 4, a dilation beyond the signal, guard scales, T no multiple of 64, two q
    sources; bitwise reproducible.  The q sums that ride along are formed from the fp32 q BEFORE it is rounded (include/vqwave.h), so
    their reference sums the unrounded q; batch stride wider than the rows, slack untouched."""
    Cp, Q0, ks = 256, 512, 3
    p, q0, q1, dw0, sc = X.wgrad_case(B, T, d, Q1, scaled)
    Q = Q0 + Q1
    pd, q0d, q1d, dw0d, scd = dev(p), dev(q0), (dev(q1) if Q1 else None), dev(dw0), dev(sc)
    taps = [-(ks - 1 - j) * d for j in range(ks)]
    slab = torch.empty(64 * 65536 * 4, device=DEV)
    args = dict(p=pd, q0=q0d, q1=q1d, Q1=Q1, slab=slab, B=B, T=T, Cp=Cp, Q0=Q0, taps=taps, p_scale=scd[0:1], q0_scale=scd[1:2],
                q1_scale=scd[2:3] if Q1 else None, mode=BF)

    def run():
        dw = dw0d.clone()
        K.f16x3_wgrad(dw=dw, **args)
        return dw
    got = run()
    qr = torch.cat([rd(q0, sc[1]), rd(q1, sc[2])], 1) if Q1 else rd(q0, sc[1])
    upd = wgrad64(rd(p, sc[0]), qr, taps)
    if (B, T, d) == (2, 512, 1):      # the device evaluation of the reference is the host's (scales are powers of two: they cancel)
        host = X.wgrad_bf16(p, np.concatenate([q0, q1], 1), taps)
        assert np.abs(upd.cpu().numpy() - host).max() <= 1e-9 * np.abs(host).max()
    err = float((got.double() - (dw0d.double() + upd)).abs().max())
    bar = wgrad_bar(upd, float(np.abs(dw0).max()))
    print('dw: max err %.3e (bar %.3e, update %.3e)' % (err, bar, float(upd.abs().max())))
    assert err <= bar, 'max err %.3e, bar %.3e' % (err, bar)
    assert torch.equal(run(), got), 'dw is not bitwise reproducible'
    seg_T = T // 32
    tot0 = (torch.randn(Q, generator=torch.Generator().manual_seed(d)) * float(np.abs(q0).max())).to(DEV)      # of q's size: no slack from it
    tot, seg = tot0.clone(), torch.zeros(B, Q + 5, seg_T, device=DEV)
    cols = (Q0, Q) if Q1 else (0, Q)
    K.f16x3_wgrad(dw=dw0d.clone(), q_total=tot, total_cols=cols, q_seg=seg, seg_T=seg_T, seg_bstride=(Q + 5) * seg_T, **args)
    q_raw = torch.cat([q0d, q1d], 1).double() if Q1 else q0d.double()
    check_q_sums(tot, tot0, seg, q_raw, cols, 32, 'q sums of fp32 q')


def test_wgrad_bf16_relu_operand(K):
    """p_relu in bf16 mode: max(p, 0) first, then scale and round (the shape of test_wgrad_f16x3_relu_operand)."""
    B, T, Cp, Q0 = 2, 512, 512, 256
    rng = np.random.RandomState(43)
    p = rng.standard_normal((B, Cp, T)).astype(np.float32)
    q = (rng.standard_normal((B, Q0, T)) * 1e-5).astype(np.float32)
    sc = torch.tensor([8.0, 2.0 ** 26], device=DEV)
    dw = torch.zeros(Cp, Q0, device=DEV)
    slab = torch.empty(256 * 65536, device=DEV)
    K.f16x3_wgrad(p=dev(p), q0=dev(q), dw=dw, slab=slab, B=B, T=T, Cp=Cp, Q0=Q0, taps=[0], p_scale=sc[0:1], q0_scale=sc[1:2], p_relu=True, mode=BF)
    want = wgrad64(rd(np.maximum(p, 0), 8.0), rd(q, 2.0 ** 26), [0])[0]
    err = float((dw.double() - want).abs().max())
    assert err <= wgrad_bar(want, 0.0), 'max err %.3e of update %.3e' % (err, float(want.abs().max()))


def test_wgrad_bf16_operands_from_planes(K):
    """q from planes, p from planes, and both (WgStage<QP, PP, BF>: one plane per LDS image, transposed reads), at shifts that are
    no multiples of 4 and at shifts of half / a quarter of the row, p also as the middle layer of a three-layer buffer whose other
    chunks are NaN: every combination bit-equal to the launch on the fp32 operands (the planes hold the bits split4<BF> makes), and
    that launch inside the float64 bar.  With q from planes the q sums are sums of the ROUNDED q."""
    B, T, R, Tz = 2, 2048, 256, 32
    rng = np.random.RandomState(19)
    net = rng.standard_normal((B, R, T)).astype(np.float32)
    dpre = (rng.standard_normal((B, 2 * R, T)) * 1e-5).astype(np.float32)
    sp, sq = 2.0 ** 9, 2.0 ** 27
    scd = torch.tensor([sp, sq], device=DEV)
    nd, dd = dev(net), dev(dpre)
    slab = torch.empty(256 * 65536, device=DEV)
    kc = R // 8
    ppl, qpl, pwide = Planes(B * R * T), Planes(B * 2 * R * T), Planes(3 * B * R * T)
    K.f16x3_split_activations(nd, ppl.t, B, R, T, scale_dev=scd[0:1], mode=BF)
    K.f16x3_split_activations(dd, qpl.t, B, 2 * R, T, scale_dev=scd[1:2], mode=BF)
    K.f16x3_split_activations(nd, pwide.t, B, R, T, kc0=kc, KC=3 * kc, scale_dev=scd[0:1], mode=BF)
    pr, qr = rd(net, sp), rd(dpre, sq)
    common = dict(slab=slab, B=B, T=T, Cp=R, Q0=2 * R, p_scale=scd[0:1], q0_scale=scd[1:2], mode=BF)
    for taps in ([-2, -1, 0], [-1024, -512, 0]):
        ref = torch.zeros(3, R, 2 * R, device=DEV)
        K.f16x3_wgrad(p=nd, q0=dd, dw=ref, taps=taps, **common)
        want = wgrad64(pr, qr, taps)
        err = float((ref.double() - want).abs().max())
        print('taps %s: max err %.3e (bar %.3e)' % (taps, err, wgrad_bar(want, 0.0)))
        assert err <= wgrad_bar(want, 0.0), 'taps %s: max err %.3e, bar %.3e' % (taps, err, wgrad_bar(want, 0.0))
        forms = (('q planes', dict(p=nd, q_planes=qpl.t)), ('p planes', dict(p_planes=ppl.t, q0=dd)),
                 ('both planes', dict(p_planes=ppl.t, q_planes=qpl.t)),
                 ('p in a wide buffer', dict(p_planes=pwide.t, p_planes_kc0=kc, p_planes_KC=3 * kc, q0=dd)),
                 ('p in a wide buffer, q planes', dict(p_planes=pwide.t, p_planes_kc0=kc, p_planes_KC=3 * kc, q_planes=qpl.t)))
        for nm, ops in forms:
            got = torch.zeros(3, R, 2 * R, device=DEV)
            tot0 = (torch.randn(2 * R, generator=torch.Generator().manual_seed(3)) * float(np.abs(dpre).max())).to(DEV)
            tot, seg = tot0.clone(), torch.zeros(B, 2 * R + 5, Tz, device=DEV)
            K.f16x3_wgrad(dw=got, taps=taps, q_total=tot, q_seg=seg, seg_T=Tz, seg_bstride=(2 * R + 5) * Tz, **common, **ops)
            assert torch.equal(got, ref), '%s, taps %s: dW differs from the fp32-operand launch' % (nm, taps)
            check_q_sums(tot, tot0, seg, qr if 'q_planes' in ops else dd.double(), (0, 2 * R), T // Tz, nm)
    for pl, nm in ((ppl, 'p planes'), (qpl, 'q planes'), (pwide, 'wide p planes')):
        pl.check_guard(nm)


def test_wgrad_bf16_batch_of_three_layers(K):
    """vqw_f16x3_wgrad_batch in bf16 mode: three layers (dilations, operands, scales, outputs differ) in one launch, each against
    the float64 einsum of its rounded operands at the single launch's bar; reproducible."""
    B, T, R = 2, 512, 256
    rng = np.random.RandomState(23)
    dils = [1, 6, 128]
    nets = [rng.standard_normal((B, R, T)).astype(np.float32) for _ in dils]
    dpres = [(rng.standard_normal((B, 2 * R, T)) * 1e-5).astype(np.float32) for _ in dils]
    s = np.float32([2.0 ** 9, 2.0 ** 10, 2.0 ** 8, 2.0 ** 27, 2.0 ** 26, 2.0 ** 28])
    sd = dev(s)
    slab = torch.empty(256 * 65536, device=DEV)
    dw0 = [rng.standard_normal((3, R, 2 * R)).astype(np.float32) * 1e-3 for _ in dils]

    def run():
        dws = [dev(d0) for d0 in dw0]
        K.f16x3_wgrad_batch([dict(p=dev(nets[i]), q0=dev(dpres[i]), dw=dws[i], taps=[-2 * d, -d, 0], p_scale=sd[i:i + 1],
                                  q0_scale=sd[3 + i:4 + i]) for i, d in enumerate(dils)], slab=slab, B=B, T=T, Cp=R, Q0=2 * R, mode=BF)
        return dws
    got, again = run(), run()
    for i, d in enumerate(dils):
        upd = wgrad64(rd(nets[i], s[i]), rd(dpres[i], s[3 + i]), [-2 * d, -d, 0])
        err = float((got[i].double() - (dev(dw0[i]).double() + upd)).abs().max())
        bar = wgrad_bar(upd, float(np.abs(dw0[i]).max()))
        assert err <= bar, 'layer %d: max err %.3e, bar %.3e' % (i, err, bar)
        assert torch.equal(got[i], again[i]), 'batched dW is not reproducible'


def test_wgrad_bf16_refuses_stride_2(K):
    """p_stride = 2 has no bf16 variant: the documented error, and nothing is launched (dw keeps its bits)."""
    B, Tq, Tin, Cp, Q0 = 2, 32, 64, 256, 256
    p, q = torch.randn(B, Cp, Tin, device=DEV), torch.randn(B, Q0, Tq, device=DEV)
    dw = torch.full((5, Cp, Q0), 3.0, device=DEV)
    slab = torch.empty(64 * 65536, device=DEV)
    with pytest.raises(RuntimeError, match='p_stride 2 needs Tp > 0 and the fp16x3 mode'):
        K.f16x3_wgrad(p=p, q0=q, dw=dw, slab=slab, B=B, T=Tq, T_p=Tin, Cp=Cp, Q0=Q0, taps=[-1, 0, 1, 2, 3], p_stride=2, mode=BF)
    torch.cuda.synchronize()
    assert bool((dw == 3.0).all())
