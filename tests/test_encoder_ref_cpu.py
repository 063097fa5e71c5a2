"""tests/encoder_ref.py against the oracle, against fp32, and against mistakes -- no GPU.

 * the composed chain is oracle/ref_model.py:encoder_64 on float64 copies: z_e and, through torch.autograd, every encoder gradient
   for a random dz, to 1e-12 of the tensor's max, with the BatchNorm statistics init_params gives (mean 0, variance 1) and with moved ones;
 * a device made of sequential fp32 evaluations (every product and addition rounded; the engine's layers: the three plane products
   of every (tap, channel) in turn) stays under sconv_ref.EMU_FRACTION of every bar check_step holds a real device to;
 * every deliberately wrong evaluation of encoder_ref.WRONG, on an engine layer and on an fp32 layer of the base case of
   tests/test_encoder_routes_gpu.py, leaves at least one bar by the factor MARGIN, and the tensors it does not touch stay inside.
   (A wrong scale slot has no such evaluation: it loses precision only; the GPU test's scale-rule assertion covers it.)"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from oracle import ref_model as M

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import encoder_ref as E  # noqa: E402
import gen_ref  # noqa: E402
import launch_trace as LT  # noqa: E402
import sconv_ref as S  # noqa: E402

SHAPES = ((1, 64, 48), (3, 192, 48), (1, 1024, 256))
MARGIN = 4.0        # a wrong evaluation must leave a bar by this factor: nothing inside a bar's own slack counts as detected
D = LT.MODEL['latent_dim']


def params(F, moved):
    """init_params(randomize_all=True) of the launch-trace configuration at F filters; moved: the moving statistics away from (0, 1)."""
    P = M.init_params(dict(LT.MODEL, use_vq=False, encoder_filters=F), dict(LT.WAVENET), LT.SPEAKERS, seed=3, randomize_all=True)
    if moved:
        rng = np.random.RandomState(7)
        for i in range(7):
            n = P[E.bn_scope(i) + '/gamma'].numel()
            P[E.bn_scope(i) + '/moving_mean'] = torch.from_numpy((0.2 * rng.standard_normal(n)).astype(np.float32))
            P[E.bn_scope(i) + '/moving_variance'] = torch.from_numpy(rng.uniform(0.5, 1.5, n).astype(np.float32))
    return {k: v for k, v in P.items() if k.startswith('encoder/')}


def batch(B, T):
    x = M.synthetic_batch(B, T, LT.SPEAKERS, 1234)[0][:, :, 0].numpy()
    dz = (np.random.RandomState(B * T).standard_normal((B, D, T // 64)) * 1e-3).astype(np.float32)
    return x, dz


@pytest.mark.parametrize('moved', [False, True], ids=['stats-init', 'stats-moved'])
@pytest.mark.parametrize('B,T,F', SHAPES)
def test_chain_is_the_oracles_encoder_64(B, T, F, moved):
    P = params(F, moved)
    x, dz = batch(B, T)
    P64 = gen_ref.to64(P)
    for n, p in P64.items():
        p.requires_grad_(M.is_trainable(n))
    z = M.encoder_64(torch.from_numpy(x).double()[:, :, None], P64)                       # [B][Tz][D]
    (z * torch.from_numpy(dz).double().permute(0, 2, 1)).sum().backward()
    fw = E.encoder_forward(x, P)
    rel = lambda a, b: float(np.abs(a - b).max()) / max(float(np.abs(b).max()), 1e-300)  # noqa: E731
    assert rel(fw['z_e'], z.detach().permute(0, 2, 1).numpy()) < 1e-12
    G = E.encoder_backward(x, P, fw, dz)
    assert set(G) == {n for n in P64 if M.is_trainable(n)}
    for n, g in G.items():
        want = P64[n].grad.numpy()
        assert g.shape == want.shape, n
        assert rel(g, want) < 1e-12, '%s: %.3e' % (n, rel(g, want))


ROUTES = {      # what tests/test_encoder_routes_gpu.py asserts of its cases at these shapes
    'fp32': dict(),
    'base': dict(enc_x3=(1,), on_w=(1,), w_planes=(1,)),
    'encx3-0': dict(on_w=(1,)),
}


@pytest.mark.parametrize('B,T,F,name', [(1, 64, 48, 'fp32'), (3, 192, 48, 'fp32'), (1, 1024, 256, 'fp32'), (1, 1024, 256, 'base'),
                                        (1, 1024, 256, 'encx3-0')])
def test_sequential_fp32_emulation_stays_under_the_bars(B, T, F, name, record_property):
    P = params(F, True)
    x, dz = batch(B, T)
    rt = E.route(B, T, F, D, **ROUTES[name])
    dev = E.fake_device(x, P, dz, rt, emulate=True)
    fr = E.check_step(dev, P, rt)
    worst = max(fr, key=fr.get)
    record_property('worst_fraction', fr[worst])
    print('emulation %s B%d T%d F%d: worst %s %.3f' % (name, B, T, F, worst, fr[worst]))
    over = {k: v for k, v in fr.items() if v > S.EMU_FRACTION}
    assert not over, over
    for slot, got, want in E.scale_checks(dev, P, rt):
        assert got == want, (slot, got, want)


@functools.lru_cache(maxsize=1)
def _base():
    P = params(256, True)
    x, dz = batch(1, 1024)
    rt = E.route(1, 1024, 256, D, **ROUTES['base'])
    return P, rt, E.fake_device(x, P, dz, rt)


# wrong evaluation -> the tensors of check_forward / check_backward(i) that must leave their bars (i the layer, k = i - 1)
DETECTED_BY = {
    'pad_prev_t_in': ('fwd_out_{i}', 'fwd_r_{i}'),
    'dbias_twice': ('dbias_{i}',),
    'dbias_dropped': ('dbias_{i}',),
    'bn_slice_prev': ('fwd_out_{i}',),
    'dgamma_no_mean': ('dgamma_{k}',),
    'parity_swap': ('dconv_{k}',),
    'drop_last_tap': ('fwd_out_{i}', 'fwd_r_{i}', 'dw_{i}', 'dconv_{k}'),
}
MAY_FOLLOW = {'parity_swap': ('dgamma_{k}',), 'drop_last_tap': ('dgamma_{k}', 'dbeta_{k}')}      # sums over the wrong input gradient


def test_the_right_evaluation_is_inside_every_bar():
    P, rt, dev = _base()
    fr = E.check_step(dev, P, rt)
    assert max(fr.values()) < 1.0, {k: v for k, v in fr.items() if v >= 1.0}


@pytest.mark.parametrize('layer', [1, 2], ids=['engine-layer', 'fp32-layer'])
@pytest.mark.parametrize('wrong', E.WRONG)
def test_wrong_evaluation_leaves_a_bar(wrong, layer):
    assert set(DETECTED_BY) == set(E.WRONG)
    P, rt, dev = _base()
    bad = E.with_wrong(dev, P, rt, layer, wrong)
    fr = dict(E.check_forward(layer, bad, P, rt), **E.check_backward(layer, bad, P, rt))
    fmt = lambda names: {n.format(i=layer, k=layer - 1) for n in names}  # noqa: E731
    must, may = fmt(DETECTED_BY[wrong]), fmt(MAY_FOLLOW.get(wrong, ()))
    for name in must:
        assert fr[name] >= MARGIN, '%s at layer %d not detected in %s: %.3f of its bar' % (wrong, layer, name, fr[name])
    print('%s at layer %d: detected, %s' % (wrong, layer, ', '.join('%s %.3g bars' % (n, fr[n]) for n in sorted(must))))
    others = {k: v for k, v in fr.items() if k not in must | may and v >= 1.0}
    assert not others, others
