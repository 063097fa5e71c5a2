"""GPU tests of clipping by global norm and gradient-norm logging: the segmented norm kernels
(csrc/gradnorm.hip) and the scaled Adam + EMA kernel against the float64 restatement of clip_ref.py, then
VQVAE.clip_norm / grad_norms at the optimiser level, end to end (VQ-VAE and latent prior) and under the deferred range guard.
Bars: every fp32 norm within 2^-22 relative of the float64 value (fp64 accumulation; sqrt and the cast to fp32 round once
each), the Adam step at the atol = rtol = 1e-6 of test_rowsum_transpose_softmax_adam."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

from oracle import ref_model as M

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_ref as CR  # noqa: E402

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REL = 2.0 ** -22
CHUNK = 16384


def tiny_cfg():
    spec = importlib.util.spec_from_file_location('make_golden', os.path.join(HERE, 'golden', 'make_golden.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.tiny_cfg()


def tiny_prior(k=32, pre_k=3):
    return {"quantization_channels": k, "num_cycles": 2, "num_cycle_layers": 4, "dilation_rates": [1, 2, 4, 8, 1, 2, 4, 8],
            "kernel_size": 3, "dilation_filters": 32, "skip_filters": 64, "residual_filters": 32,
            "preprocess": {"kernel_size": pre_k, "filters": 32}, "speaker_embedding": 16, "learning_rate_schedule": {"0": 1e-3}}


def close(got, want, rel=REL):
    return abs(got - want) <= rel * abs(want)


# ------------------------------------------------------------------ 1, 2: the norm kernels
LENGTHS = [1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 7]
#            alone: fp32 square = 0                 fp32 square = inf
MAGNITUDES = [1e-30, 1e-12, 1e-3, 1.0, 1e-20, 1e25, 1e15, 1e5]


@pytest.fixture(scope='module')
def norm_case(K):
    """~100 k floats in eight segments laid end to end (most offsets are no multiple of 4), a seeded normal times the
    segment's magnitude; the buffer on the device (never modified), its plan and the float64 norms per grad_scale."""
    assert K.GRAD_NORM_CHUNK == CHUNK
    bounds = np.concatenate(([0], np.cumsum(LENGTHS)))
    rng = np.random.default_rng(20240)
    host = np.concatenate([(rng.standard_normal(n) * mag).astype(np.float32) for n, mag in zip(LENGTHS, MAGNITUDES)])
    host[0] = np.float32(1e-30)                    # the one-element segment holds 1e-30 itself
    with np.errstate(all='ignore'):
        assert host[0] * host[0] == 0 and np.isinf(np.square(host[bounds[5]:bounds[6]])).any()
    ref = {gs: CR.segment_norms(host, bounds, gs) for gs in (1.0, 0.5)}
    return {'bounds': bounds, 'host': host, 'dev': torch.from_numpy(host).cuda(), 'plan': K.grad_norm_plan(bounds), 'ref': ref}


@pytest.mark.parametrize('grad_scale', [1.0, 0.5])
@pytest.mark.parametrize('clip_factor', [float('inf'), 2.0, 0.5], ids=['inf', 'above', 'below'])
def test_norm_kernel_matches_float64(K, norm_case, grad_scale, clip_factor):
    seg_ref, norm_ref = norm_case['ref'][grad_scale]
    clip = clip_factor * norm_ref
    out = K.grad_norm(norm_case['dev'], norm_case['plan'], grad_scale=grad_scale, clip=clip).cpu().double().numpy()
    assert out.shape == (2 + len(LENGTHS),)
    print('global %.9e (ref %.9e) scale %.9e' % (out[0], norm_ref, out[1]))
    assert close(out[0], norm_ref), (out[0], norm_ref)
    for k, want in enumerate(seg_ref):
        print('segment %d: %.9e (ref %.9e, rel %.2e)' % (k, out[2 + k], want, abs(out[2 + k] - want) / want))
        assert want > 0 and np.isfinite(want)
        assert close(out[2 + k], want), (k, out[2 + k], want)
    if clip_factor >= 1.0:
        assert out[1] == 1.0
    else:
        assert close(out[1], CR.clip_scale(norm_ref, clip)), (out[1], CR.clip_scale(norm_ref, clip))


def test_norm_kernel_is_reproducible_and_segments_are_independent(K, norm_case):
    plan, bounds = norm_case['plan'], norm_case['bounds']
    a = K.grad_norm(norm_case['dev'], plan, clip=3.0).cpu()
    b = K.grad_norm(norm_case['dev'], plan, clip=3.0).cpu()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    other = norm_case['dev'].clone()
    k = 5
    other[bounds[k]:bounds[k + 1]] = torch.linspace(-7.0, 9.0, LENGTHS[k], device='cuda')
    c = K.grad_norm(other, plan, clip=3.0).cpu()
    keep = [2 + j for j in range(len(LENGTHS)) if j != k]
    assert torch.equal(a[keep].view(torch.int32), c[keep].view(torch.int32))
    assert a[2 + k] != c[2 + k] and a[0] != c[0]


def test_norm_kernel_noncontiguous_segments(K):
    """The model's tables: a variable that is a column block of a grouped kernel is one run per row (rows of 6 and 4 columns
    of a [37][10] matrix, offsets of every alignment)."""
    rng = np.random.default_rng(7)
    w = rng.standard_normal((37, 10)).astype(np.float32)
    runs = [(r * 10, 6, 0) for r in range(37)] + [(r * 10 + 6, 4, 1) for r in range(37)]
    out = K.grad_norm(torch.from_numpy(w).cuda().view(-1), K.grad_norm_plan_runs(runs, 2), clip=float('inf')).cpu().double().numpy()
    w64 = w.astype(np.float64)
    for got, want in zip(out, [np.sqrt((w64 ** 2).sum()), 1.0, np.sqrt((w64[:, :6] ** 2).sum()), np.sqrt((w64[:, 6:] ** 2).sum())]):
        assert close(got, want), (got, want)


# ------------------------------------------------------------------ 3: scaled Adam
def test_scaled_adam(K, pkg):
    n, lr_ts = 1003, (1e-3, 7e-4)          # not a multiple of 4: the tail loop runs
    rng = np.random.default_rng(11)
    host = [rng.standard_normal(n).astype(np.float32) for _ in range(2)]        # p, ema
    grads = [rng.standard_normal(n).astype(np.float32) for _ in range(2)]
    L = pkg._lib

    def run(how):
        p, ema = torch.from_numpy(host[0]).cuda(), torch.from_numpy(host[1]).cuda()
        m, v = torch.zeros(n, device='cuda'), torch.zeros(n, device='cuda')
        for g, lr_t in zip(grads, lr_ts):
            how(p, torch.from_numpy(g).cuda(), m, v, ema, lr_t)
        torch.cuda.synchronize()
        return [t.cpu() for t in (p, m, v, ema)]

    def entry_before(p, g, m, v, ema, lr_t):      # the entry point the step used before the scaled form existed
        L.check(L.lib().vqw_adam_ema_step_guarded(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), L.ptr(ema), n, lr_t, 0.9, 0.999, 1e-8, 0.999,
                                                  0.5, None, L.stream()))

    one, quarter = torch.ones(1, device='cuda'), torch.full((1,), 0.25, device='cuda')
    base = run(lambda p, g, m, v, ema, lr_t: K.adam_ema_step(p, g, m, v, ema, lr_t=lr_t, grad_scale=0.5))
    for how in (entry_before, lambda p, g, m, v, ema, lr_t: K.adam_ema_step(p, g, m, v, ema, lr_t=lr_t, grad_scale=0.5, scale=one)):
        for a, b in zip(base, run(how)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    got = run(lambda p, g, m, v, ema, lr_t: K.adam_ema_step(p, g, m, v, ema, lr_t=lr_t, grad_scale=0.5, scale=quarter))
    ref = (host[0], np.zeros(n), np.zeros(n), host[1])
    for g, lr_t in zip(grads, lr_ts):
        p_, m_, v_, e_ = CR.adam_ema_step(ref[0], g, ref[1], ref[2], ref[3], lr_t=lr_t, grad_scale=0.5, scale=0.25)
        ref = (p_, m_, v_, e_)
    assert not np.allclose(got[1].numpy(), base[1].numpy(), atol=1e-6, rtol=1e-6)      # the scale is no no-op (m, v: Adam's step itself barely depends on it)
    for a, b in zip(got, ref):
        np.testing.assert_allclose(a.double().numpy(), b, atol=1e-6, rtol=1e-6)
    skip = torch.ones(1, dtype=torch.int32, device='cuda')
    start = [torch.from_numpy(host[0]), torch.zeros(n), torch.zeros(n), torch.from_numpy(host[1])]
    voided = run(lambda p, g, m, v, ema, lr_t: K.adam_ema_step(p, g, m, v, ema, lr_t=lr_t, grad_scale=0.5, skip=skip, scale=quarter))
    for a, b in zip(voided, start):
        assert torch.equal(a, b)


# ------------------------------------------------------------------ 4: model, optimiser level
STATE = ('flat', 'adam_m', 'adam_v', 'ema')


def test_model_optimiser_level(pkg):
    """The gradient is fixed (training steps are not bit-reproducible run to run: the fp32 engine's atomics)."""
    m, w = tiny_cfg()
    P = M.init_params(m, w, 10, seed=11, randomize_all=True)
    models = []
    for _ in range(3):
        model = pkg.model.VQVAE(m, w, 10, device='cuda', seed=0)
        model.load_named(P)
        models.append(model)
    g = torch.randn(models[0].n_flat, generator=torch.Generator().manual_seed(5))
    for model in models:
        model.grad.copy_(g)
    off, measured, clipped = models
    assert off.clip_norm is None
    with pytest.raises(ValueError):
        off.grad_norms()
    with pytest.raises(ValueError):
        off.clip_norm = 0.0
    with pytest.raises(ValueError):
        off.clip_norm = float('nan')
    with pytest.raises(ValueError):
        off.clip_norm = 1e-50                    # 0 as the fp32 the kernels take
    assert 'clip_norm' not in off.state_dict()
    start = {k: getattr(clipped, k).cpu().numpy() for k in STATE}
    measured.clip_norm = 1e30
    off.apply_gradients()
    measured.apply_gradients()
    for k in STATE:
        assert torch.equal(getattr(off, k), getattr(measured, k)), k
    norm = float(g.double().norm())
    gn = measured.grad_norms()
    assert close(gn['global'], norm) and gn['scale'] == 1.0
    clipped.clip_norm = 0.5 * norm
    clipped.apply_gradients()
    gn = clipped.grad_norms()
    assert close(gn['scale'], 0.5), gn['scale']
    lr_t = clipped.lr_at(0) * np.sqrt(1.0 - 0.999) / (1.0 - 0.9)
    p_, m_, v_, e_ = CR.adam_ema_step(start['flat'], g.numpy(), start['adam_m'], start['adam_v'], start['ema'], lr_t=lr_t,
                                      scale=CR.clip_scale(norm, 0.5 * norm))
    for k, want in zip(STATE, (p_, m_, v_, e_)):
        np.testing.assert_allclose(getattr(clipped, k).cpu().double().numpy(), want, atol=1e-6, rtol=1e-6, err_msg=k)
    assert not torch.equal(clipped.flat, off.flat)


# ------------------------------------------------------------------ 5: model, end to end
def _check_three_steps(model, batches):
    model.clip_norm = float('inf')
    names = [n for n in model.named_parameters() if M.is_trainable(n)]
    for x, spk in batches:
        model.train_step(x, spk)
        gn = model.grad_norms()
        want = float(model.grad.double().norm())
        assert want > 0 and close(gn['global'], want), (gn['global'], want)
        assert gn['scale'] == 1.0
        assert list(gn['segments']) == names
        total = sum(v * v for v in gn['segments'].values())
        assert abs(total - gn['global'] ** 2) <= 1e-6 * gn['global'] ** 2, (total, gn['global'] ** 2)
    model.clip_norm = None
    with pytest.raises(ValueError):
        model.grad_norms()
    model.clip_norm = 1.0                        # on again, no step since: the norms of a step before the switch are not reported
    with pytest.raises(ValueError):
        model.grad_norms()
    model.clip_norm = None


def test_model_end_to_end(pkg):
    m, w = tiny_cfg()
    model = pkg.model.VQVAE(m, w, 10, device='cuda', seed=0)
    model.load_named(M.init_params(m, w, 10, seed=11, randomize_all=True))
    batches = []
    for i in range(3):
        x, spk, _ = M.synthetic_batch(2, 512, 10, 1234 + i)
        batches.append((x[:, :, 0].contiguous().cuda(), spk.cuda()))
    _check_three_steps(model, batches)


def test_prior_end_to_end(pkg):
    prior = pkg.prior.LatentPrior(tiny_prior(), 10, device='cuda', seed=0, n_codes=32)
    g = torch.Generator().manual_seed(3)
    batches = [(torch.randint(0, 32, (2, 128), generator=g, dtype=torch.int32).cuda(), torch.randint(0, 10, (2,), generator=g).cuda())
               for _ in range(3)]
    _check_three_steps(prior, batches)


# ------------------------------------------------------------------ 6: deferred guard
def test_clipping_under_the_deferred_guard(pkg, monkeypatch):
    """As test_deferred_guard_matches_immediate: reference widths, B = 1, T = 1024, the second of four steps flagged by a
    layer-input scale pushed 2^24 up.  The voided steps measured norms too; after the replay the buffer holds the kept step's."""
    monkeypatch.setenv('VQW_ENGINE', 'f16x3')
    monkeypatch.delenv('VQW_GATE_F16X3', raising=False)
    m, w = dict(M.DEFAULT_MODEL), dict(M.DEFAULT_WAVENET)
    model = pkg.model.VQVAE(m, w, 109, device='cuda', seed=0)
    model.load_named(M.init_params(m, w, 109, seed=3, randomize_all=True))
    assert model.x3_guard and model.gbwd_f16x3
    model.defer_guard = True
    model.clip_norm = 0.5
    for i in range(4):
        x, spk, _ = M.synthetic_batch(1, 1024, 109, 4321 + i)
        if i == 1:
            model.x3_scale[model.SL['X'] + 2] *= 2.0 ** 24
        model.train_step(x[:, :, 0].contiguous().cuda(), spk.cuda())
    model.finish_steps()
    assert model.global_step == 4 and model.x3_fallbacks == 1
    for k in STATE:
        assert torch.isfinite(getattr(model, k)).all(), k
    gn = model.grad_norms()
    want = float(model.grad.double().norm())
    print('global %.9e (grad %.9e) scale %.6f' % (gn['global'], want, gn['scale']))
    assert want > 0 and close(gn['global'], want), (gn['global'], want)
    assert close(gn['scale'], CR.clip_scale(gn['global'], 0.5), 2.0 ** -23)
