"""Every route of Encoder64.forward / backward on the device, layer by layer against tests/encoder_ref.py (DESIGN 6.x "Encoder routes").

One train_step of the launch-trace configuration (tests/launch_trace.py MODEL / WAVENET, use_vq = False, so that the encoder's incoming
gradient ws['dz'] is a copy of ws['dcond'][:, :D] and can be read back) per case; the hook between the passes snapshots ws['X'], ws['r'],
ws['y6'], ws['z_e'] and ws['enc_scale'].  Every layer is then checked in isolation from the DEVICE'S OWN inputs (encoder_ref.check_step):
    forward   r[i], X[i] against conv_s2(device X[i-1]) through relu and the affine; engine layers plane-exactly at the scales found
              in the device's slots.  A relu input near zero needs no excuse: the bar is 1-Lipschitz through the relu.
    scales    every slot the case's routes use equals scale_rule(max |its tensor|), every other slot still holds its start-up 1, all
              are powers of two.
    backward  with d_i = ws['dX'][i] = d(conv_i output): kernel gradient against wgrad_s2(device X[i-1], d_i), bias gradient against
              dbias(d_i) (of the planes where q_total summed planes), ws['dX'][i-1] against dgrad_s2(d_i, w) scale mask with the
              mask ws['r'][i-1] > 0, BatchNorm gamma / beta gradients against the sums over the reference's own unmasked dgrad_s2;
              layer 6 (1x1) and layer 0 (conv_cin1_wgrad) likewise.
    whole     z_e against oracle.ref_model.encoder_64 in float64 at 2e-4 of the max; every encoder gradient against float64
              autograd over the oracle's ops with the device's masks imposed, at 5e-3 in relative L2 (tests/test_model_gpu.py's bars).
The moving statistics are moved away from (0, 1) (load_named loads them): with mean 0 and variance 1 a BatchNorm slice of the
wrong layer or a lost mean term would cost nothing.

Each case asserts the routes it is there for (ws['enc_x3'], plan.enc_wg3, model.wg_planes, _short_layer_split per layer at its
fixed cus = 256) and records worst_fraction = the worst err / bar over all its tensors."""
import os
import sys
import time

import numpy as np
import pytest
import torch

from oracle import ref_model as M
from oracle import ref_ops as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import encoder_ref as E  # noqa: E402
import gen_ref  # noqa: E402
import launch_trace as LT  # noqa: E402

pytestmark = pytest.mark.gpu

# encoder_filters 48 / 64 with the narrowest decoder the other tests run (32 / 64 / 32, two layers)
NARROW_W = dict(LT.WAVENET, dilation_filters=32, skip_filters=64, residual_filters=32, preprocess={'kernel_size': 32, 'filters': 32})
NARROW_M = dict(LT.MODEL, k=32, latent_dim=16, speaker_embedding=16)
ALL = (1, 2, 3, 4, 5)

# enc_x3: layers whose conv and input gradient run on the fp16x3 engine; wg3: plan.enc_wg3; on_w: layers whose weight gradient runs
# there (wg3, T_out % 4 == 0, B T_out >= 256); pp: model.wg_planes (both operands as kept planes where on_w and enc_x3 meet);
# splits: _short_layer_split of layers 1..5 (forward; the input gradient of layer i has that of layer i - 1's length, the same rule)
CASES = {
    'base': dict(B=1, T=1024, enc_x3=(1,), wg3=True, on_w=(1,), pp=True, splits=[8, 8, 8, 8, 8]),
    'pp0': dict(B=1, T=1024, env={'VQW_WGRAD_PP': '0'}, enc_x3=(1,), wg3=True, on_w=(1,), pp=False, splits=[8, 8, 8, 8, 8]),
    'encx3-0': dict(B=1, T=1024, env={'VQW_ENC_X3': '0'}, enc_x3=(), wg3=True, on_w=(1,), pp=True, splits=[8, 8, 8, 8, 8]),
    'encwg-0': dict(B=1, T=1024, env={'VQW_ENC_WGRAD_X3': '0'}, enc_x3=(1,), wg3=False, on_w=(), pp=True, splits=[8, 8, 8, 8, 8]),
    'split-0': dict(B=1, T=1024, env={'VQW_SCONV_SPLIT': '0'}, enc_x3=(1,), wg3=True, on_w=(1,), pp=True, splits=[8, 8, 8, 8, 8]),
    'overlap-0': dict(B=1, T=1024, env={'VQW_OVERLAP': '0'}, enc_x3=(1,), wg3=True, on_w=(1,), pp=True, splits=[8, 8, 8, 8, 8]),
    'fp32': dict(B=1, T=1024, env={'VQW_ENGINE': 'fp32'}, enc_x3=(), wg3=False, on_w=(), pp=True, splits=[8, 8, 8, 8, 8], table=False),
    # layer 5: 3 * 88 = 264 columns, a partial 256-column tile that crosses batch rows, odd batch
    'all-five': dict(B=3, T=5632, enc_x3=ALL, wg3=True, on_w=ALL, pp=True, splits=[7, 8, 8, 8, 8]),
    # T % 256 != 0: the decoder is refused, so no weight gradient on the engine; T_out = 130 in layer 4, layer 5 (130 columns) on fp32
    'ragged': dict(B=2, T=4160, enc_x3=(1, 2, 3, 4), wg3=False, on_w=(), pp=True, splits=[8, 8, 8, 8, 8]),
    # T_out = 1 in layer 5: fewer input samples than taps, taps outside on both sides; wgrad_gemm with T_p = 2, T_q = 1
    'shortest-B1': dict(B=1, T=64, model=dict(NARROW_M, encoder_filters=48), wavenet=NARROW_W, enc_x3=(), wg3=False, on_w=(), pp=True,
                        splits=[8, 8, 8, 8, 8], table=False),
    'shortest-B3': dict(B=3, T=64, model=dict(NARROW_M, encoder_filters=48), wavenet=NARROW_W, enc_x3=(), wg3=False, on_w=(), pp=True,
                        splits=[8, 8, 8, 8, 8], table=False),
    # layer 1: 65 * 8 = 520 blocks of 64 x 128 (> 512): one unsplit conv with the fused epilogue, plain parity input gradient; layer 2 in three
    'unsplit': dict(B=8, T=33280, env={'VQW_ENGINE': 'fp32'}, model=dict(NARROW_M, encoder_filters=64), wavenet=NARROW_W, enc_x3=(), wg3=False,
                    on_w=(), pp=True, splits=[1, 3, 7, 8, 8], table=False),
}


def _params(m, w):
    P = M.init_params(m, w, LT.SPEAKERS, seed=3, randomize_all=True)
    rng = np.random.RandomState(7)
    for i in range(7):
        n = P[E.bn_scope(i) + '/gamma'].numel()
        P[E.bn_scope(i) + '/moving_mean'] = torch.from_numpy((0.2 * rng.standard_normal(n)).astype(np.float32))
        P[E.bn_scope(i) + '/moving_variance'] = torch.from_numpy(rng.uniform(0.5, 1.5, n).astype(np.float32))
    return P


def _np(t):
    return t.detach().cpu().numpy().copy()


def run_step(pkg, monkeypatch, c):
    """One train_step of case c -> (dev: the tensors encoder_ref.check_step reads, as numpy; P; the route; ws; model)."""
    LT.set_switches(monkeypatch, c.get('env', {}))
    m, w = dict(c.get('model', LT.MODEL), use_vq=False), dict(c.get('wavenet', LT.WAVENET))
    B, T, F, D = c['B'], c['T'], m['encoder_filters'], m['latent_dim']
    P = _params(m, w)
    x, spk, _ = M.synthetic_batch(B, T, LT.SPEAKERS, 1234)
    model = pkg.model.VQVAE(m, w, LT.SPEAKERS, device='cuda', seed=0)
    model.load_named(P)
    assert torch.equal(model.bn_mean.cpu(), torch.cat([P[E.bn_scope(i) + '/moving_mean'] for i in range(7)]))
    snaps = []

    def hook(ws):
        snaps.append(dict(X=[_np(t) for t in ws['X']], r=[_np(t) for t in ws['r']], y6=_np(ws['y6']), z_e=_np(ws['z_e']),
                          scale=_np(ws['scale']), shift=_np(ws['shift']), es_fwd=_np(ws['enc_scale']) if 'enc_scale' in ws else np.ones(12, np.float32)))
    ws = model.train_step(x[:, :, 0].contiguous().cuda(), spk.cuda(), on_forward=hook)
    torch.cuda.synchronize()
    assert model.x3_fallbacks == 0 and len(snaps) == 1
    # the routes this case is there for
    enc = model.encoder
    assert tuple(ws['enc_x3']) == tuple(c['enc_x3']), ws['enc_x3']
    assert bool(ws['plan'].enc_wg3) == c['wg3'] and tuple(ws['plan'].enc_x3) == tuple(c['enc_x3'])
    assert bool(model.wg_planes) == c['pp']
    Tl = [T // 2 ** (i + 1) for i in range(6)]
    assert [type(enc)._short_layer_split(F, Tl[i], B) for i in ALL] == c['splits']
    assert ('enc_scale' in ws) == c.get('table', True)
    on_w = tuple(i for i in ALL if c['wg3'] and Tl[i] % 4 == 0 and B * Tl[i] >= 256)
    assert on_w == tuple(c['on_w'])
    rt = E.route(B, T, F, D, enc_x3=c['enc_x3'], on_w=c['on_w'], w_planes=[i for i in c['on_w'] if i in c['enc_x3'] and c['pp']])
    grads = {n: _np(g) for n, g in model.named_gradients().items() if n.startswith('encoder/')}
    dev = dict(snaps[0], x=x[:, :, 0].numpy(), dX=[_np(t) for t in ws['dX']], d6=_np(ws['dz']), dz=_np(ws['dcond'][:, :D]), grads=grads,
               es=_np(ws['enc_scale']) if 'enc_scale' in ws else np.ones(12, np.float32))
    return dev, {k: v for k, v in P.items() if k.startswith('encoder/')}, rt, ws, model


def autograd_with_masks(x, P, dz, masks):
    """float64 autograd over the oracle's own ops, the relu of layer i replaced by the product with masks[i] [B][F][T_i]:
    -> (z_e [B][D][Tz], {name: gradient})."""
    P64 = gen_ref.to64(P)
    for n, p in P64.items():
        p.requires_grad_(M.is_trainable(n))
    net = torch.from_numpy(x).double()[:, :, None]
    for i in range(6):
        net = R.keras_conv1d(net, P64[E.conv_scope(i) + '/kernel'], P64[E.conv_scope(i) + '/bias'], stride=2, padding='same')
        net = net * torch.from_numpy(masks[i]).double().permute(0, 2, 1)
        b = E.bn_scope(i)
        net = R.batch_norm_inference(net, P64[b + '/gamma'], P64[b + '/beta'], P64[b + '/moving_mean'], P64[b + '/moving_variance'])
    net = R.keras_conv1d(net, P64[E.conv_scope(6) + '/kernel'], P64[E.conv_scope(6) + '/bias'], stride=1, padding='valid')
    b = E.bn_scope(6)
    z = R.batch_norm_inference(net, P64[b + '/gamma'], P64[b + '/beta'], P64[b + '/moving_mean'], P64[b + '/moving_variance'])
    (z * torch.from_numpy(dz).double().permute(0, 2, 1)).sum().backward()
    return z.detach().permute(0, 2, 1).numpy(), {n: p.grad.numpy() for n, p in P64.items() if p.grad is not None}


def check_case(name, dev, P, rt, table, record_property):
    fr = E.check_step(dev, P, rt)
    for k in sorted(fr, key=fr.get, reverse=True)[:6]:
        print('%s: %-12s %.4f of its bar' % (name, k, fr[k]))
    worst = max(fr, key=fr.get)
    record_property('worst_fraction', fr[worst])
    record_property('worst_tensor', worst)
    over = {k: v for k, v in fr.items() if not v <= 1.0}
    assert not over, '%s: over their bars (err / bar): %s' % (name, over)
    if table:
        for tab in (dev['es_fwd'], dev['es']):
            assert np.array_equal(tab, np.exp2(np.round(np.log2(tab)))), 'scales must be powers of two: %s' % tab
        bad = [(slot, got, want) for slot, got, want in E.scale_checks(dev, P, rt) if got != want]
        assert not bad, '%s: scale slots (slot, found, the rule / 1.0 for a slot no route uses): %s' % (name, bad)
    # the whole encoder, at the project's bars
    with torch.no_grad():
        z64 = M.encoder_64(torch.from_numpy(dev['x']).double()[:, :, None], gen_ref.to64(P)).permute(0, 2, 1).numpy()
    e = float(np.abs(dev['z_e'] - z64).max()) / float(np.abs(z64).max())
    print('%s: z_e %.3e of max' % (name, e))
    assert e < 2e-4, e
    _, G = autograd_with_masks(dev['x'], P, dev['dz'], [r > 0 for r in dev['r']])
    assert set(G) == set(dev['grads'])
    worst_g = max((float(np.linalg.norm(dev['grads'][n].astype(np.float64) - g)) / max(float(np.linalg.norm(g)), 1e-30), n) for n, g in G.items())
    print('%s: worst gradient %.3e rel. L2 (%s)' % (name, *worst_g))
    assert worst_g[0] < 5e-3, worst_g
    return fr


@pytest.mark.parametrize('name', list(CASES))
def test_encoder_routes(pkg, monkeypatch, record_property, name):
    c = CASES[name]
    t0 = time.perf_counter()
    dev, P, rt, ws, model = run_step(pkg, monkeypatch, c)
    t1 = time.perf_counter()
    check_case(name, dev, P, rt, c.get('table', True), record_property)
    print('%s: step %.1f s, reference %.1f s' % (name, t1 - t0, time.perf_counter() - t1))


def test_one_stream_equals_two_streams(pkg, monkeypatch):
    """VQW_OVERLAP=0 against the base case on the same batch.  What no atomic addition has touched must agree bit for bit: that is the
    forward pass up to layer 1 (layer 0 and the engine's layer 1; layers 2..5 are split over K with fp32 atomics, and everything
    behind them -- z_e, the decoder, hence dz and every gradient -- inherits their summation order).  The gradients of both runs
    are held to the per-layer bars by test_encoder_routes[base] / [overlap-0]; here, the two runs' gradients are held to each
    other at the project's 5e-3 in relative L2 between two fp32 evaluations -- a weight gradient that read a buffer the main
    stream was still writing would differ by whole values."""
    a, P, rt, _, _ = run_step(pkg, monkeypatch, CASES['base'])
    b, _, _, _, _ = run_step(pkg, monkeypatch, CASES['overlap-0'])
    for k in ('X', 'r'):
        for i in (0, 1):
            assert np.array_equal(a[k][i].view(np.uint32), b[k][i].view(np.uint32)), '%s[%d] differs between one and two streams' % (k, i)
    assert np.array_equal(a['es_fwd'], b['es_fwd'])
    for n, g in a['grads'].items():
        e = float(np.linalg.norm(g.astype(np.float64) - b['grads'][n])) / max(float(np.linalg.norm(g)), 1e-30)
        assert e < 5e-3, '%s: one stream vs two streams %.3e rel. L2' % (n, e)
