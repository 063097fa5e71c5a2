"""GPU tests of the conditioning conv inside the model: the training step against an autograd restatement built
from the oracle's pieces, "off is off", the condition paths outside training, both generators, the optimiser and the command
line.  The tiny configuration and shapes of tests/test_jitter_gpu.py."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import ref_model as M

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_ref as G  # noqa: E402
import jitter_ref as JR  # noqa: E402
from flips import describe, relu_flips  # noqa: E402
from test_jitter_gpu import FIXED_SRC, FIXED_U, STATE, _batches, bits, reproducible_cfg  # noqa: E402
from test_model_gpu import build, l2err, relerr, tiny_cfg  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('decoder/condition_conv/kernel', 'decoder/condition_conv/bias')


def conv_params(m, w, S, seed):
    """oracle.ref_model.init_params for a configuration with the conv: the local_condition kernels over C + Cs rows, the
    conv's kernel (glorot-uniform) and a bias away from zero, so that every term shows."""
    P = M.init_params(m, w, S, seed=seed, randomize_all=True)
    C, k, D = m['condition_conv'], m.get('condition_conv_kernel', 3), m['latent_dim']
    rows = C + (m['speaker_embedding'] or S)
    g = torch.Generator().manual_seed(seed + 1)
    for n in [n for n in P if n.endswith('local_condition/kernel')]:
        P[n] = (torch.rand(1, rows, P[n].shape[2], generator=g) * 2 - 1) * math.sqrt(3.0 / rows)
    P[NAMES[0]] = (torch.rand(k, D, C, generator=g) * 2 - 1) * math.sqrt(6.0 / (k * D + k * C))
    P[NAMES[1]] = 0.1 * torch.randn(C, generator=g)
    return P


def ref_condition(z_q, P):
    """The float64 conv1d between discretise and concat: z_q [B][Tz][D] -> [B][Tz][C]."""
    wc, bc = P[NAMES[0]].double(), P[NAMES[1]].double()
    out = torch.nn.functional.conv1d(z_q.double().permute(0, 2, 1), wc.permute(2, 1, 0), bc, padding=(wc.shape[0] - 1) // 2)
    return out.permute(0, 2, 1).to(z_q.dtype)


def ref_step(x, spk, P, m, w, src=None, collect=None):
    """tests/test_jitter_gpu.py's ref_step with the conv behind the gather: encoder, discretise, [gather], conv, concat, decoder."""
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
    logits, labels = M.wavenet_build(x, M.R.concat(ref_condition(seen, P), h), P, w, collect)
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


def check_step(model, xd, sd, x, spk, P, m, w, src, grad_tol, flip_tol, what):
    """test_jitter_gpu.check_step against this file's ref_step: logits 5e-4, losses 2e-5, gradients grad_tol of the tensor max."""
    col = {}
    out, grads = ref_step(x, spk, P, m, w, None if src is None else torch.from_numpy(src), collect=col)
    assert set(NAMES) <= set(grads)
    model._jitter_step = None if src is None else 0       # a forward pass as train_step runs it, but keeping the logits
    try:
        ws = model.forward(xd, sd, compute_grad_seed=False)
    finally:
        model._jitter_step = None
    assert bool(ws['jittered']) == (src is not None)
    if out['q'] is not None:
        assert torch.equal(ws['idx'].cpu(), out['q']), what
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


# ------------------------------------------------------------------ 1: the step against autograd
@pytest.mark.parametrize('C', [32, 128], ids=['Cc48', 'Cc144'])
@pytest.mark.parametrize('engine', [None, 'fp32'], ids=['default', 'fp32'])
@pytest.mark.parametrize('use_vq', [True, False], ids=['vq', 'no_vq'])
def test_model_step_matches_autograd(pkg, monkeypatch, use_vq, engine, C):
    """The tiny configuration, B = 2, T = 512 (Tz = 8), without jitter and with time_jitter = 0.5 on a fixed u.  Bars: those the
    same configuration holds without the conv.  C = 32: Cc = 48, the projections on their own kernels; C = 128:
    Cc = 144 > 128, on the fp32 conv engine."""
    if engine is None:
        monkeypatch.delenv('VQW_ENGINE', raising=False)
    else:
        monkeypatch.setenv('VQW_ENGINE', engine)
    m, w = tiny_cfg()
    seed, grad_tol, flip_tol = (11, 2e-3, None) if use_vq else (31, 5e-3, 2e-2)
    m = dict(m, use_vq=use_vq, condition_conv=C)
    P = conv_params(m, w, 10, seed)
    x, spk, _ = M.synthetic_batch(2, 512, 10, 1234)
    xd, sd = x[:, :, 0].contiguous().cuda(), spk.cuda()
    plain = build(pkg, m, w, 10, P)
    assert plain.Cc == C + 16 and plain.cond_proj == (C + 16 <= 128)
    g0 = check_step(plain, xd, sd, x, spk, P, m, w, None, grad_tol, flip_tol, 'no jitter')
    u = np.array(FIXED_U, np.float32)
    src = JR.src_of(u, 0.5)
    assert src.tolist() == FIXED_SRC
    model = build(pkg, dict(m, time_jitter=0.5), w, 10, P)
    model.jitter_uniforms = lambda B, Tz, step: torch.from_numpy(u).cuda()
    g1 = check_step(model, xd, sd, x, spk, P, m, w, src, grad_tol, flip_tol, 'jitter')
    # the conv's gradients are no small part of the step, and the jitter does reach them
    assert float(g0[NAMES[0]].abs().max()) > 0 and float(g0[NAMES[1]].abs().max()) > 0 and l2err(g1[NAMES[0]], g0[NAMES[0]]) > 1e-2


# ------------------------------------------------------------------ 2: off is off
def test_off_is_off(pkg):
    """"condition_conv": 0 against the key absent, three steps from the same parameters at the shape whose step is
    bit-reproducible (test_jitter_gpu.reproducible_cfg): the same bits in parameters, EMA shadows and Adam slots, no new
    variable, buffer or state entry."""
    m, w, B, T = reproducible_cfg()
    P = M.init_params(m, w, 10, seed=21, randomize_all=True)
    batches = _batches(3, B, T, 10, 1234)
    absent, zero = build(pkg, m, w, 10, P), build(pkg, dict(m, condition_conv=0), w, 10, P)
    assert 'condition_conv' not in m and absent.n_flat == zero.n_flat
    for model in (absent, zero):
        assert model.cconv == 0 and model.Dc == model.D
        for xd, sd in batches:
            model.train_step(xd, sd)
        model.finish_steps()
        assert model.global_step == 3
        assert not any(k in ws for ws in model._ws.values() for k in ('zq', 'dzq', 'zj', 'dzj', 'cconv_scratch', 'cconv_in'))
        assert 'condition_conv' not in model.state_dict() and not any('condition_conv' in n for n in model.named_parameters())
    for k in STATE:
        assert torch.equal(bits(getattr(absent, k)), bits(getattr(zero, k))), k
    assert not torch.equal(absent.flat, absent.ema)


# ------------------------------------------------------------------ 3: the condition paths outside training
def test_condition_paths_agree(pkg, K):
    """encode, its one-utterance form and condition_from_codes apply the conv forward() applies, and none of them jitters.
    The Magenta encoder: two passes of Encoder_64 are not bit-equal (tests/test_jitter_gpu.py)."""
    m, w = tiny_cfg()
    C = 32
    m = dict(m, encoder='Magenta', condition_conv=C, condition_conv_kernel=5, time_jitter=0.5)
    model = pkg.model.VQVAE(m, w, 10, device='cuda', seed=3)
    model.P['condition_conv_b'].copy_(0.1 * torch.randn(C, generator=torch.Generator().manual_seed(1)))
    (xd, sd), = _batches(1, 3, 512, 10, 1234)
    ws = model.forward(xd, sd, compute_grad_seed=False)
    assert not ws['jittered'] and tuple(ws['cond'].shape) == (3, C + 16, 8)
    cond = ws['cond'].clone()
    direct = torch.full((3, C, 8), float('nan'), device='cuda')
    K.cond_conv_fwd(ws['zq'], model.P['condition_conv_w'], model.P['condition_conv_b'], direct)
    assert torch.equal(cond[:, :C], direct)
    assert torch.equal(cond[:, C:], model.P['speaker_embedding'][sd][:, :, None].expand(3, 16, 8))
    assert torch.equal(model.encode(xd, sd), cond)
    model.train_step(xd, sd)                          # a jittered step leaves its buffers in the workspace those calls share
    model.finish_steps()
    model.load_state_dict({k: v.clone() for k, v in model.state_dict().items()})
    spk3 = torch.tensor([4, 0, 7], dtype=torch.int64, device='cuda')
    one = model.encode(xd[:1].contiguous(), spk3)
    assert torch.equal(one, model.encode(xd[:1].repeat(3, 1), spk3)) and not torch.equal(one[0, C:], one[1, C:])
    enc = model.encode(xd, sd)
    codes = model.encode_codes(xd, sd)
    got = model.condition_from_codes(codes, sd)
    z = model.P['embedding'][codes.long()].permute(0, 2, 1).contiguous()
    K.cond_conv_fwd(z, model.P['condition_conv_w'], model.P['condition_conv_b'], direct)
    assert torch.equal(got[:, :C], direct) and torch.equal(got[:, C:], enc[:, C:])
    # (encode's own latent rows come from the straight-through z_q = z_e + (e_k - z_e): e_k up to that sum's rounding)
    assert relerr(got[:, :C], enc[:, :C]) < 1e-5 and float(direct.abs().max()) > 0.05


# ------------------------------------------------------------------ 4: the generators
N_GEN, T_GEN = 2 * 64 + 3, 256          # past the second frame boundary; teacher-forced on four whole frames


@pytest.fixture(scope='module')
def gen_case(pkg):
    m, w = tiny_cfg()
    m = dict(m, condition_conv=32)
    P = conv_params(m, w, 10, 11)
    model = build(pkg, m, w, 10, P)
    (xd, sd), = _batches(1, 3, T_GEN, 10, 77)
    enc = model.encode(xd, sd)
    assert tuple(enc.shape) == (3, 48, T_GEN // 64)
    u = torch.rand(3, N_GEN, generator=torch.Generator().manual_seed(5))
    return dict(pkg=pkg, model=model, P=P, w=w, x=xd, enc=enc, u=u)


def check_last_step(c, audio, idx, probs, first=0):
    """The distribution of step N_GEN - 1 against the training graph in float64, teacher-forced on `audio` [B][N_GEN] (zeros
    behind it up to whole frames: the graph is causal) under the condition the model encoded: test_wide_gen_gpu.check_a's bar."""
    full = torch.zeros(3, T_GEN)
    full[:, :N_GEN] = audio.cpu()
    p64 = G.decoder_probs64(c['P'], c['w'], full.numpy(), c['enc'].permute(0, 2, 1))
    G.check_sampled(p64[:, first:N_GEN], c['u'][:, first:], idx.cpu()[:, first:])
    np.testing.assert_allclose(probs.cpu().numpy(), p64[:, N_GEN - 1], rtol=2e-4, atol=1e-7, err_msg='distribution of the last step')


@pytest.mark.parametrize('cls', ['FastGenerator', 'WideGenerator'])
def test_generators_see_the_condition(gen_case, cls):
    c = gen_case
    gen = getattr(c['pkg'].generator, cls)(c['model'], batch=3)
    try:
        audio, idx, probs = gen.generate(c['enc'], N_GEN, mode='sample', uniforms=c['u'].cuda(), ratio=64, return_probs=True)
        check_last_step(c, audio, idx, probs)
        # from a prompt of 70 samples (past the first frame boundary): the same last step
        prompt = c['x'][:, :70].contiguous()
        (gen.prefill if cls == 'FastGenerator' else gen.prefill_prompt)(prompt, c['enc'], ratio=64)
        rest = c['u'][:, 70:].contiguous()
        audio, idx, probs = gen.generate(c['enc'], N_GEN - 70, mode='sample', uniforms=rest.cuda(), ratio=64, return_probs=True)
        # (the graph's input of step t is mu_law_encode(prompt[t - 1]): the prompt itself stands in front of the generated audio)
        check_last_step(c, torch.cat([prompt.cpu(), audio.cpu()], 1), torch.cat([torch.zeros(3, 70, dtype=idx.dtype), idx.cpu()], 1), probs, first=70)
    finally:
        gen.close()


# ------------------------------------------------------------------ 5: the optimiser
def test_optimiser_sees_the_variables(pkg, monkeypatch):
    monkeypatch.setenv('VQW_ENGINE', 'fp32')
    m, w = tiny_cfg()
    m = dict(m, condition_conv=32)
    P = conv_params(m, w, 10, 11)
    x, spk, _ = M.synthetic_batch(4, 512, 10, 1234)
    xd, sd = x[:, :, 0].contiguous().cuda(), spk.cuda()
    model = build(pkg, m, w, 10, P)
    model.clip_norm = float('inf')
    before = {n: (model.P[n].clone(), model.E[n].clone()) for n in ('condition_conv_w', 'condition_conv_b')}
    model.train_step(xd, sd)
    model.finish_steps()
    for n, (p0, e0) in before.items():
        assert not torch.equal(model.P[n], p0) and not torch.equal(model.E[n], e0) and not torch.equal(model.P[n], model.E[n]), n
    seg = model.grad_norms()['segments']
    assert all(n in seg and seg[n] > 0 for n in NAMES)
    # accumulate = 2 over two batches of 2 against one step on the 4 rows (tests/test_accum_gpu.py: relative L2 5e-3 per variable)
    window, big = build(pkg, m, w, 10, P), build(pkg, m, w, 10, P)
    window.accumulate = 2
    for k in range(2):
        window.train_step(xd[2 * k:2 * k + 2].contiguous(), sd[2 * k:2 * k + 2].contiguous())
    assert window.global_step == 1 and window.accum_index == 0
    big.train_step(xd, sd)
    got, own = window.named_gradients(), big.named_gradients()
    for name in own:
        e = l2err(got[name] / 2, own[name])
        assert e < 5e-3, (name, e)
    assert all(float(own[n].abs().max()) > 0 for n in NAMES)


# ------------------------------------------------------------------ 6: the command line
def test_train_then_generate_cli(tmp_path):
    from scipy.io import wavfile
    w = {"verbose": False, "quantization_channels": 256, "num_cycles": 1, "num_cycle_layers": 4,
         "dilation_rates": [1, 2, 4, 8], "kernel_size": 3, "dilation_filters": 32, "skip_filters": 64,
         "residual_filters": 32, "preprocess": {"kernel_size": 32, "filters": 32}}
    m = {"encoder": "64", "use_vq": True, "speaker_embedding": 16, "k": 32, "latent_dim": 16, "beta": 0.25,
         "encoder_filters": 48, "wavenet_parameters": str(tmp_path / 'w.json'), "verbose": False,
         "learning_rate_schedule": {"0": 1e-3}, "condition_conv": 32}
    (tmp_path / 'w.json').write_text(json.dumps(w))
    (tmp_path / 'm.json').write_text(json.dumps(m))
    (tmp_path / 'off.json').write_text(json.dumps({k: v for k, v in m.items() if k != 'condition_conv'}))
    env, cwd = dict(os.environ, PYTHONPATH=ROOT), str(tmp_path)
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'train.py'), '-dataset', 'synthetic', '-length', '512',
                          '-batch', '2', '-step', '2', '-interval', '1', '-save', 'saved_model/weights', '-params',
                          str(tmp_path / 'm.json')], cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    ckpt = tmp_path / 'saved_model' / 'weights-2.pt'
    sd = torch.load(str(ckpt), map_location='cpu', weights_only=True)
    assert sd['condition_conv'].tolist() == [32, 3]
    (tmp_path / 'data').mkdir()
    (tmp_path / 'data' / 'vctk_speakers.txt').write_text('p225, 3\np226, 5\n')
    t = np.arange(1100) / 16000.0
    wavfile.write(str(tmp_path / 'a.wav'), 16000, (np.sin(2 * np.pi * 220 * t) * 8000).astype(np.int16))
    gen = [sys.executable, os.path.join(ROOT, 'generate.py'), '-audio', str(tmp_path / 'a.wav'), '-speakers', 'p226', 'None', '-mode', 'greedy']
    out = subprocess.run(gen + ['-restore', str(ckpt), '-params', str(tmp_path / 'm.json')], cwd=cwd, env=env, capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    for name in ('2_no_speaker.wav', '2_p226.wav'):
        sr, audio = wavfile.read(str(tmp_path / 'saved_model' / name))
        assert sr == 16000 and audio.shape == (1024,) and np.isfinite(audio).all()
    for restore in (ckpt, tmp_path / 'saved_model' / 'weights-2.safetensors'):
        bad = subprocess.run(gen + ['-restore', str(restore), '-params', str(tmp_path / 'off.json')], cwd=cwd, env=env,
                             capture_output=True, text=True, timeout=600)
        assert bad.returncode != 0 and "'condition_conv'" in bad.stderr and 'local_condition' in bad.stderr, bad.stderr[-2000:]
