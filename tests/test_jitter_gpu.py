"""GPU tests of the time-jitter regulariser: both kernels bit for bit against the numpy restatement
(jitter_ref.py), their argument checks, the model's training step against an autograd restatement built from the oracle's
pieces, "off is off", one draw per step under the range guard, and the command line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import ref_model as M

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jitter_ref as JR  # noqa: E402
from flips import describe, relu_flips  # noqa: E402
from test_model_gpu import _guarded_model, build, l2err, relerr, tiny_cfg  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (3, 64, 104): the benchmark's latent shape per row; Tz = 1, 2, 3: the reflections meet; (5, 12, 257): Tz crosses a wave and a
# 256-thread block and is odd, D is no multiple of the block's channel rows times anything
SHAPES = [(3, 64, 104), (2, 4, 1), (2, 4, 2), (1, 8, 3), (5, 12, 257)]
PROBS = [0.0, 0.12, 1.0]
SENTINEL = -12345.5
JITTER_KEYS = ('zq', 'dzq', 'jitter_u', 'jitter_src')
STATE = ('flat', 'ema', 'adam_m', 'adam_v')


def bits(t):
    return t.contiguous().view(torch.int32)


def uniforms(B, Tz, p, seed):
    """A random u and a hand-made one: a left move at t = 0, a right move at t = Tz - 1, values exactly at lo and hi and their
    fp32 neighbours below, cycled over the frames so that every row holds each of them."""
    rng = np.random.default_rng(seed)
    rand = rng.random((B, Tz), dtype=np.float32)
    lo, hi = JR.thresholds(p)
    top = np.nextafter(np.float32(1), np.float32(0))
    special = np.array([0.0, np.nextafter(lo, np.float32(-1)), lo, 0.5, np.nextafter(hi, np.float32(-1)), hi, top], np.float32)
    special = np.clip(special, np.float32(0), top)                        # u stays in [0, 1)
    hand = special[(np.arange(B)[:, None] * 3 + np.arange(Tz)[None, :]) % len(special)].astype(np.float32)
    hand[:, 0] = 0.0                     # u < lo (p > 0): frame 0 looks left and is reflected to frame 1
    hand[0, Tz - 1] = top                # u >= hi (p > 0): the last frame looks right and is reflected to Tz - 2
    return [rand, hand]


@pytest.mark.parametrize('p', PROBS)
@pytest.mark.parametrize('B,D,Tz', SHAPES)
def test_forward_kernel_bit_exact(K, B, D, Tz, p):
    rng = np.random.default_rng(B * 1000 + D * 10 + Tz)
    for n, u in enumerate(uniforms(B, Tz, p, seed=Tz + 17)):
        zbuf = rng.standard_normal((B, D + 3, Tz)).astype(np.float32)    # zq = the first D rows of a wider buffer
        want_src = JR.src_of(u, p)
        want = JR.fwd(zbuf[:, :D], want_src)
        if n == 1 and p > 0 and Tz >= 2:
            assert want_src[0, 0] == 1 and want_src[0, Tz - 1] == Tz - 2          # both reflections are in the case
        zd, ud = torch.from_numpy(zbuf).cuda(), torch.from_numpy(u).cuda()
        out = torch.full((B, D + 7, Tz), SENTINEL, device='cuda')
        src = torch.full((B, Tz), -7, dtype=torch.int32, device='cuda')
        K.time_jitter_fwd(zd, ud, out, src, p=p, D=D, zq_bstride=(D + 3) * Tz, out_bstride=(D + 7) * Tz)
        assert torch.equal(src.cpu(), torch.from_numpy(want_src)), 'src, u %d' % n
        assert torch.equal(bits(out[:, :D]).cpu(), bits(torch.from_numpy(want))), 'out, u %d' % n
        assert bool((out[:, D:] == SENTINEL).all()), 'rows >= D were written'
        assert torch.equal(zd.cpu(), torch.from_numpy(zbuf))


@pytest.mark.parametrize('p', PROBS)
@pytest.mark.parametrize('B,D,Tz', SHAPES)
def test_backward_kernel_bit_exact(K, B, D, Tz, p):
    rng = np.random.default_rng(B * 1000 + D * 10 + Tz + 1)
    for n, u in enumerate(uniforms(B, Tz, p, seed=Tz + 18)):
        src = JR.src_of(u, p)
        gbuf = rng.standard_normal((B, D + 7, Tz)).astype(np.float32)    # dout = the first D rows of a wider buffer
        gbuf[:, :, ::5] *= -0.0                                            # signed zeros: 0.0f + (-0.0f) = +0.0f
        want = JR.bwd(gbuf[:, :D], src)
        dzq = torch.full((B, D, Tz), float('nan'), device='cuda')
        K.time_jitter_bwd(torch.from_numpy(gbuf).cuda(), torch.from_numpy(src).cuda(), dzq, D=D, dout_bstride=(D + 7) * Tz)
        assert torch.equal(bits(dzq).cpu(), bits(torch.from_numpy(want))), 'dzq, u %d' % n


def test_argument_checks_return_errors(pkg, K):
    L = pkg._lib
    lib = L.lib()
    B, D, Tz = 2, 4, 9
    z = torch.randn(B, D, Tz, device='cuda')
    z0 = z.clone()
    o = torch.full((B, D, Tz), SENTINEL, device='cuda')
    u = torch.rand(B, Tz, device='cuda')
    src = torch.zeros(B, Tz, dtype=torch.int32, device='cuda')
    n, st = D * Tz, L.stream()
    fwd, bwd, ptr = lib.vqw_time_jitter_fwd, lib.vqw_time_jitter_bwd, L.ptr
    assert fwd(ptr(z), n, ptr(u), 0.25, 0.75, ptr(z), n, ptr(src), B, D, Tz, st) != 0
    assert b'alias' in lib.vqw_last_error()
    for args in ((None, n, ptr(u), 0.25, 0.75, ptr(o), n, ptr(src)), (ptr(z), n, None, 0.25, 0.75, ptr(o), n, ptr(src)),
                 (ptr(z), n, ptr(u), 0.25, 0.75, None, n, ptr(src)), (ptr(z), n, ptr(u), 0.25, 0.75, ptr(o), n, None)):
        assert fwd(*args, B, D, Tz, st) != 0
        assert b'null pointer' in lib.vqw_last_error()
    for dims in ((0, D, Tz), (B, 0, Tz), (B, D, 0), (B, D, -3)):
        assert fwd(ptr(z), n, ptr(u), 0.25, 0.75, ptr(o), n, ptr(src), *dims, st) != 0
        assert b'positive' in lib.vqw_last_error()
    assert fwd(ptr(z), n - 1, ptr(u), 0.25, 0.75, ptr(o), n, ptr(src), B, D, Tz, st) != 0
    assert b'batch strides' in lib.vqw_last_error()
    assert fwd(ptr(z), n, ptr(u), 0.25, 0.75, ptr(o), n - 1, ptr(src), B, D, Tz, st) != 0
    assert bwd(ptr(o), n, ptr(src), ptr(o), n, B, D, Tz, st) != 0
    assert b'alias' in lib.vqw_last_error()
    assert bwd(None, n, ptr(src), ptr(z), n, B, D, Tz, st) != 0 and bwd(ptr(o), n, None, ptr(z), n, B, D, Tz, st) != 0
    assert bwd(ptr(o), n, ptr(src), None, n, B, D, Tz, st) != 0
    assert b'null pointer' in lib.vqw_last_error()
    assert bwd(ptr(o), n, ptr(src), ptr(z), n - 1, B, D, Tz, st) != 0 and bwd(ptr(o), n, ptr(src), ptr(z), n, B, D, 0, st) != 0
    with pytest.raises(RuntimeError, match='alias'):
        K.time_jitter_fwd(z, u, z, src, p=0.5, D=D)
    with pytest.raises(ValueError):
        K.time_jitter_fwd(z, u, o, src, p=1.5, D=D)
    with pytest.raises(ValueError):
        K.time_jitter_fwd(z, u, o[:, :D - 1].contiguous(), src, p=0.5, D=D)       # out too small for D rows
    torch.cuda.synchronize()
    assert torch.equal(z, z0) and bool((o == SENTINEL).all()) and int(src.abs().max()) == 0      # nothing was launched


# ------------------------------------------------------------------ 4: the model's step against autograd
def ref_step(x, spk, P, m, w, src=None, collect=None):
    """oracle.ref_model.train_step's forward + backward with an index gather on the time axis between discretise and concat
    (src int [B][Tz], None: no jitter).  The VQ and commitment losses are those of the un-jittered tensors."""
    for n_, p_ in P.items():
        p_.requires_grad_(M.is_trainable(n_))
        p_.grad = None
    z_e = M.encoder_64(x, P, collect)
    if m['use_vq']:
        q, e_k, z_q = M.discretise(z_e, P['embedding/embedding'])
    else:
        q, e_k, z_q = None, z_e, z_e
    seen = z_q if src is None else torch.gather(z_q, 1, src.long()[:, :, None].expand_as(z_q))
    h = P['speaker_embedding'][spk].unsqueeze(1)
    logits, labels = M.wavenet_build(x, M.R.concat(seen, h), P, w, collect)
    out = {'q': q, 'z_e': z_e, 'logits': logits, 'labels': labels,
           'reconstruction_loss': torch.nn.functional.cross_entropy(logits, labels.long(), reduction='mean')}
    out['loss'] = out['reconstruction_loss']
    if m['use_vq']:
        out['vq_loss'] = torch.mean((z_e.detach() - e_k) ** 2)
        out['loss'] = out['loss'] + out['vq_loss'] + m['beta'] * torch.mean((z_e - e_k.detach()) ** 2)
    out['loss'].backward()
    grads = {n_: p_.grad.detach().clone() for n_, p_ in P.items() if p_.grad is not None}
    for p_ in P.values():
        p_.requires_grad_(False)
    return out, grads


# both edges of row 0 move (t = 0 left, t = 7 right); interior moves: row 0 t = 2, 4; row 1 t = 1, 3, 5, 6  (p = 0.5: lo 0.25, hi 0.75)
FIXED_U = [[0.1, 0.5, 0.9, 0.5, 0.1, 0.5, 0.5, 0.9],
           [0.5, 0.1, 0.5, 0.9, 0.5, 0.9, 0.1, 0.5]]
FIXED_SRC = [[1, 1, 3, 3, 3, 5, 6, 6],
             [0, 0, 2, 4, 4, 6, 5, 7]]


def check_step(model, xd, sd, x, spk, P, m, w, src, grad_tol, flip_tol, what):
    """run_parity's checks and bars (tests/test_model_gpu.py) for one step of `model` against ref_step(src)."""
    col = {}
    out, grads = ref_step(x, spk, P, m, w, None if src is None else torch.from_numpy(src), collect=col)
    model._jitter_step = None if src is None else 0       # a forward pass as train_step runs it, but keeping the logits
    try:
        ws = model.forward(xd, sd, compute_grad_seed=False)
    finally:
        model._jitter_step = None
    assert bool(ws['jittered']) == (src is not None)
    if out['q'] is not None:
        assert torch.equal(ws['idx'].cpu(), out['q']), what
    assert torch.equal(ws['labels'].cpu().reshape(-1), out['labels']), what
    assert relerr(ws['z_e'].permute(0, 2, 1), out['z_e']) < 2e-4
    e = relerr(ws['logits'].permute(0, 2, 1).reshape(-1, model.Q), out['logits'])
    print('%s: logits %.3e' % (what, e))
    assert e < 5e-4, what
    snap = {}

    def relu_inputs(ws_):
        snap['skip_sum'] = ws_['skip'].permute(0, 2, 1).clone()
        snap['post1_pre'] = ws_['h1'].permute(0, 2, 1).clone()
    ws = model.train_step(xd, sd, on_forward=relu_inputs)
    if src is not None:
        assert torch.equal(ws['jitter_src'].cpu(), torch.from_numpy(src)), what
    pairs = {k: (snap[k], col[k]) for k in snap}
    pairs.update({'enc_relu_%d' % i: (ws['r'][i].permute(0, 2, 1), col['enc_relu_%d' % i]) for i in range(6)})
    flips = relu_flips(pairs)
    loss, recon, vq, commit = model.losses(ws)
    np.testing.assert_allclose(recon, out['reconstruction_loss'].item(), rtol=2e-5)
    np.testing.assert_allclose(vq, out['vq_loss'].item() if 'vq_loss' in out else 0.0, rtol=2e-5)
    np.testing.assert_allclose(loss, out['loss'].item(), rtol=2e-5)
    got = model.named_gradients()
    benign = bool(flips) and all(f['benign'] for f in flips)
    worst = ('', 0.0)
    for name, gref in grads.items():
        if benign and flip_tol is not None:
            e, tol = l2err(got[name], gref), flip_tol
        else:
            e, tol = relerr(got[name], gref), grad_tol
        worst = max(worst, (name, e), key=lambda v: v[1])
        assert e < tol, '%s: grad %s err %.3e (bar %.1e); %s' % (what, name, e, tol, describe(flips))
    print('%s: worst grad %s %.3e; %s' % (what, worst[0], worst[1], describe(flips)))
    return grads


@pytest.mark.parametrize('use_vq', [True, False], ids=['vq', 'no_vq'])
def test_model_step_matches_autograd(pkg, use_vq):
    """The tiny configuration, B = 2, T = 512 (Tz = 8), time_jitter = 0.5 with a fixed u.  Bars: those run_parity holds for the
    same configuration without jitter (test_tiny_model_two_steps: gradients 2e-3 of the tensor max; use_vq false,
    test_config_variants_use_vq_false_and_one_hot_speakers: 5e-3, or 2e-2 in relative L2 in a step with a demonstrated benign
    relu flip).  The un-jittered step is held to the same bars first, against the same restatement."""
    m, w = tiny_cfg()
    seed, grad_tol, flip_tol = (11, 2e-3, None) if use_vq else (31, 5e-3, 2e-2)
    m = dict(m, use_vq=use_vq)
    P = M.init_params(m, w, 10, seed=seed, randomize_all=True)
    x, spk, _ = M.synthetic_batch(2, 512, 10, 1234)
    xd, sd = x[:, :, 0].contiguous().cuda(), spk.cuda()
    u = np.array(FIXED_U, np.float32)
    src = JR.src_of(u, 0.5)
    assert src.tolist() == FIXED_SRC
    plain = build(pkg, m, w, 10, P)
    g0 = check_step(plain, xd, sd, x, spk, P, m, w, None, grad_tol, flip_tol, 'no jitter')
    assert not any(k in ws for ws in plain._ws.values() for k in JITTER_KEYS)
    model = build(pkg, dict(m, time_jitter=0.5), w, 10, P)
    calls = []

    def fixed_u(B, Tz, step):
        calls.append((B, Tz, step))
        return torch.from_numpy(u).cuda()
    model.jitter_uniforms = fixed_u
    g1 = check_step(model, xd, sd, x, spk, P, m, w, src, grad_tol, flip_tol, 'jitter')
    assert calls[-1] == (2, 8, 0)                             # the step's entry value of global_step
    assert abs(model.jitter_moved(model._ws[(2, 512, True)]) - 8 / 16) < 1e-6
    # the jitter does change the encoder's gradients (the test would otherwise pass with the gather left out of the backward)
    name = 'encoder/conv1d_6/kernel'
    assert l2err(g1[name], g0[name]) > 1e-2


# ------------------------------------------------------------------ 5: off is off
def _batches(n, B, T, S, seed):
    out = []
    for i in range(n):
        x, spk, _ = M.synthetic_batch(B, T, S, seed + i)
        out.append((x[:, :, 0].contiguous().cuda(), spk.cuda()))
    return out


def reproducible_cfg():
    """A configuration and shape whose training step is bit-reproducible from run to run, which the fp32 engine's steps are not
    in general (tests/test_clip_gpu.py: its weight gradients, bias sums and Encoder_64's split-K layers add with fp32
    atomics).  The tiny configuration with the Magenta encoder at B = 2, T = 128 (Tz = 2): no split-K launch in the forward
    pass, the weight gradients run as one time chunk, so every atomic address has at most the two batch rows as
    contributors (0 + a + b = 0 + b + a).  Measured without this feature: 15 of 15 pairs of models bit-equal after two steps
    (B = 1 and 2, T = 64 and 128), against 0 of 4 at T = 512 and 0 of 10 with Encoder_64 at any shape."""
    m, w = tiny_cfg()
    return dict(m, encoder='Magenta'), w, 2, 128


def test_off_is_off(pkg):
    """Key absent against "time_jitter": 0.0, two steps from the same parameters: the same bits in the parameters, EMA shadows
    and Adam slots, and no jitter buffer in any workspace."""
    m, w, B, T = reproducible_cfg()
    P = M.init_params(m, w, 10, seed=21, randomize_all=True)
    batches = _batches(2, B, T, 10, 1234)
    absent, zero = build(pkg, m, w, 10, P), build(pkg, dict(m, time_jitter=0.0), w, 10, P)
    assert 'time_jitter' not in m and absent.time_jitter == 0.0 and zero.time_jitter == 0.0
    for model in (absent, zero):
        for xd, sd in batches:
            model.train_step(xd, sd)
        model.finish_steps()
        assert model.global_step == 2
        assert not any(k in ws for ws in model._ws.values() for k in JITTER_KEYS)
        assert not any(k.startswith('jitter') or k == 'time_jitter' for k in model.state_dict())
    for k in STATE:
        assert torch.equal(bits(getattr(absent, k)), bits(getattr(zero, k))), k
    assert not torch.equal(absent.flat, absent.ema)           # (the steps did move the parameters)


def test_only_train_step_jitters(pkg):
    """Two models, one with time_jitter = 0.5: forward(), evaluate(), encode() and encode_codes() give the same bits.  The
    tiny configuration with the Magenta encoder: two forward passes of Encoder_64 are not bit-equal even without this feature
    (its short layers are split over K with fp32 atomics, tests/test_model_gpu.py), the Magenta stack has no such launch."""
    m, w = tiny_cfg()
    m = dict(m, encoder='Magenta')
    P = M.init_params(m, w, 10, seed=21, randomize_all=True)
    (xd, sd), = _batches(1, 2, 512, 10, 1234)
    plain, jit = build(pkg, m, w, 10, P), build(pkg, dict(m, time_jitter=0.5), w, 10, P)
    with pytest.raises(ValueError):
        build(pkg, dict(m, time_jitter=1.5), w, 10, P)
    with pytest.raises(ValueError):
        jit.time_jitter = -0.1
    a, b = plain.forward(xd, sd, compute_grad_seed=False), jit.forward(xd, sd, compute_grad_seed=False)
    assert not b['jittered'] and not any(k in b for k in JITTER_KEYS)
    for k in ('cond', 'logits', 'idx'):
        assert torch.equal(a[k], b[k]), k
    sa, sb = plain.evaluate(xd, sd), jit.evaluate(xd, sd)
    assert torch.equal(sa.nll_sum, sb.nll_sum) and torch.equal(sa.entropy_sum, sb.entropy_sum) and torch.equal(sa.codes, sb.codes)
    assert torch.equal(plain.encode(xd, sd), jit.encode(xd, sd))
    assert torch.equal(plain.encode_codes(xd, sd), jit.encode_codes(xd, sd))
    # ... also after a jittered training step has left its buffers in the workspace those calls share
    jit.train_step(xd, sd)
    ws = jit._ws[(2, 512, True)]
    assert ws['jittered'] and all(k in ws for k in JITTER_KEYS) and 0.0 < jit.jitter_moved(ws) < 1.0
    assert torch.equal(ws['jitter_src'].cpu(), torch.from_numpy(JR.src_of(ws['jitter_u'].cpu().numpy(), 0.5)))
    jit.load_named(P)
    assert torch.equal(plain.encode(xd, sd), jit.encode(xd, sd))
    b = jit.forward(xd, sd, compute_grad_seed=False)
    assert not b['jittered'] and torch.equal(a['cond'], b['cond'])


# ------------------------------------------------------------------ 6: one draw per step
def test_uniforms_are_a_pure_function_of_seed_and_step(pkg):
    m, w = tiny_cfg()
    model = pkg.model.VQVAE(dict(m, time_jitter=0.12), w, 10, device='cuda', seed=0)
    torch.cuda.manual_seed(1234)
    state = torch.cuda.get_rng_state()
    cpu_state = torch.get_rng_state()
    a, b, c = model.jitter_uniforms(3, 104, 5), model.jitter_uniforms(3, 104, 5), model.jitter_uniforms(3, 104, 6)
    model.jitter_seed = 1
    d = model.jitter_uniforms(3, 104, 5)
    assert torch.equal(torch.cuda.get_rng_state(), state) and torch.equal(torch.get_rng_state(), cpu_state)
    assert a.dtype == torch.float32 and a.is_cuda and tuple(a.shape) == (3, 104)
    assert torch.equal(a, b) and not torch.equal(a, c) and not torch.equal(a, d)
    assert float(a.min()) >= 0.0 and float(a.max()) < 1.0
    assert 'jitter_seed' not in model.state_dict()


def test_guard_repeat_draws_the_same_jitter(pkg, monkeypatch):
    """test_deferred_guard_matches_immediate's shape and way of flagging a step: reference widths, B = 1, T = 1024, a
    layer-input scale pushed 2^24 up behind the engine's back.  The fp32 repeat of the flagged step reads the attempt's frames."""
    m, w = dict(M.DEFAULT_MODEL, time_jitter=0.5), dict(M.DEFAULT_WAVENET)
    P = M.init_params(m, w, 109, seed=3, randomize_all=True)
    batches = _batches(2, 1, 1024, 109, 4321)
    model = _guarded_model(pkg, monkeypatch, P, m, w)
    seen = []
    for i, (xd, sd) in enumerate(batches):
        if i == 1:
            model.x3_scale[model.SL['X'] + 2] *= 2.0 ** 24
        seen.append([])
        model.train_step(xd, sd, on_forward=lambda ws, i=i: seen[i].append((ws['jitter_src'].clone(), ws['jitter_u'].clone(), bool(ws['x3_used']))))
    assert model.x3_fallbacks == 1 and model.global_step == 2
    assert len(seen[0]) == 1 and len(seen[1]) == 2
    (s_try, u_try, x3_try), (s_rep, u_rep, x3_rep) = seen[1]
    assert x3_try and not x3_rep
    assert torch.equal(s_try, s_rep) and torch.equal(u_try, u_rep)
    assert torch.equal(u_try, model.jitter_uniforms(1, 16, 1)) and not torch.equal(u_try, seen[0][0][1])
    assert torch.equal(s_try.cpu(), torch.from_numpy(JR.src_of(u_try.cpu().numpy(), 0.5)))


def test_deferred_and_immediate_agree_bit_for_bit(pkg, monkeypatch):
    """Three jittered steps on different batches with the range flag read on the spot and one step late (defer_guard): the
    same source frames in every step and the same bits in the parameters, EMA shadows and Adam slots.  At reproducible_cfg's
    shape: steps on the guarded engine's own shapes are not bit-equal between two runs of ONE mode
    (test_deferred_guard_matches_immediate holds them to 3e-3); the replay of a flagged step at such a shape is
    test_deferred_replay_draws_each_step_as_before."""
    monkeypatch.setenv('VQW_ENGINE', 'f16x3')
    monkeypatch.delenv('VQW_GATE_F16X3', raising=False)
    m, w, B, T = reproducible_cfg()
    m = dict(m, time_jitter=0.5)
    P = M.init_params(m, w, 10, seed=21, randomize_all=True)
    batches = _batches(3, B, T, 10, 1234)
    runs = []
    for defer in (False, True):
        model = build(pkg, m, w, 10, P)
        assert model.x3_guard
        model.defer_guard = defer
        srcs = []
        for xd, sd in batches:
            ws = model.train_step(xd, sd)
            srcs.append(ws['jitter_src'].clone())
        model.finish_steps()
        assert model.global_step == 3 and ws['jittered']
        runs.append((model, srcs))
    (a, sa), (b, sb) = runs
    assert len({tuple(s_.reshape(-1).tolist()) for s_ in sa}) > 1          # (the draw changes from step to step)
    for s0, s1 in zip(sa, sb):
        assert torch.equal(s0, s1)
    for k in STATE:
        assert torch.equal(bits(getattr(a, k)), bits(getattr(b, k))), k


def test_deferred_replay_draws_each_step_as_before(pkg, monkeypatch):
    """test_deferred_guard_matches_immediate's shape, deferred mode, the second of three steps flagged: _resolve_oldest rewinds
    global_step before it repeats the flagged step and runs the speculative one again, so the draws are asked for steps
    0, 1, 2 (speculative, voided), then 1 (the fp32 repeat) and 2 again."""
    m, w = dict(M.DEFAULT_MODEL, time_jitter=0.5), dict(M.DEFAULT_WAVENET)
    P = M.init_params(m, w, 109, seed=3, randomize_all=True)
    batches = _batches(3, 1, 1024, 109, 4321)
    model = _guarded_model(pkg, monkeypatch, P, m, w)
    model.defer_guard = True
    asked, draw = [], model.jitter_uniforms

    def logged(B, Tz, step):
        asked.append(step)
        return draw(B, Tz, step)
    model.jitter_uniforms = logged
    for i, (xd, sd) in enumerate(batches):
        if i == 1:
            model.x3_scale[model.SL['X'] + 2] *= 2.0 ** 24
        ws = model.train_step(xd, sd)
    model.finish_steps()
    assert model.global_step == 3 and model.x3_fallbacks == 1
    assert asked == [0, 1, 2, 1, 2], asked
    assert torch.equal(ws['jitter_u'], draw(1, 16, 2))
    assert torch.equal(ws['jitter_src'].cpu(), torch.from_numpy(JR.src_of(ws['jitter_u'].cpu().numpy(), 0.5)))


# ------------------------------------------------------------------ 7: command line
def test_train_cli_logs_the_moved_share(tmp_path):
    w = {"verbose": False, "quantization_channels": 256, "num_cycles": 1, "num_cycle_layers": 4,
         "dilation_rates": [1, 2, 4, 8], "kernel_size": 3, "dilation_filters": 32, "skip_filters": 64,
         "residual_filters": 32, "preprocess": {"kernel_size": 32, "filters": 32}}
    m = {"encoder": "64", "use_vq": True, "speaker_embedding": 16, "k": 32, "latent_dim": 16, "beta": 0.25,
         "encoder_filters": 48, "wavenet_parameters": str(tmp_path / 'w.json'), "verbose": False,
         "learning_rate_schedule": {"0": 1e-3}}
    (tmp_path / 'w.json').write_text(json.dumps(w))
    (tmp_path / 'm.json').write_text(json.dumps(m))
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'train.py'), '-dataset', 'synthetic', '-length', '512',
                          '-batch', '2', '-step', '2', '-interval', '1', '-save', 'saved_model/weights', '-params',
                          str(tmp_path / 'm.json'), '-time_jitter', '0.5'], cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT),
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert '[jitter 0.' in out.stdout
    lines = [json.loads(ln) for ln in (tmp_path / 'saved_model' / 'summaries.jsonl').read_text().splitlines()]
    assert [ln['global_step'] for ln in lines] == [1, 2]
    for ln in lines:
        assert 0.0 < ln['jitter_moved'] < 1.0
