"""GPU tests of the latent prior over VQ codes (prior.py, csrc/prior.hip, the code-input mode of csrc/ar_persist.hip)
against a CPU restatement built from oracle.ref_ops: conv1d_v2 over one_hot(shift_right(codes)), the decoder's residual
stack and head with the speaker as the only condition, cross-entropy against the codes; FastConvState queues for sampling.
Bars as in test_model_gpu.py: logits 5e-4 of max, loss rtol 2e-5, gradients 2e-3 of the per-tensor max (tiny), 5e-3
relative L2 at the reference widths, parameters / EMA after Adam 1e-4."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from oracle import ref_model as M
from oracle import ref_ops as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tiny_prior(k=32, pre_k=3):
    return {"quantization_channels": k, "num_cycles": 2, "num_cycle_layers": 4, "dilation_rates": [1, 2, 4, 8, 1, 2, 4, 8],
            "kernel_size": 3, "dilation_filters": 32, "skip_filters": 64, "residual_filters": 32,
            "preprocess": {"kernel_size": pre_k, "filters": 32}, "speaker_embedding": 16, "learning_rate_schedule": {"0": 1e-3}}


def default_prior():
    with open(os.path.join(ROOT, 'prior_parameters.json')) as f:
        return json.load(f)


def relerr(a, b):
    a, b = a.detach().cpu().float(), b.detach().cpu().float()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-12)


def l2err(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm()) / max(float(b.norm()), 1e-30)


def random_params(prior, seed):
    """Every variable random (biases and the zero-initialised ones included), so that every path carries signal."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for n, v in prior.named_parameters().items():
        scale = float(v.abs().max()) if float(v.abs().max()) > 0 else 0.1
        out[n] = ((torch.rand(v.shape, generator=g) * 2 - 1) * scale).float()
    return out


# ------------------------------------------------------------------ CPU restatement
def ref_logits(codes, spk, P, cfg):
    """codes int64 [B,T], spk int64 [B] -> logits [B,T,k], in the parameters' dtype (float64 copies: tests/gen_ref.py)."""
    k = cfg['quantization_channels']
    B, T = codes.shape
    x = R.shift_right(Fn.one_hot(codes, k).to(P['prior/preprocess/kernel'].dtype))
    net = R.conv1d_v2(x, P['prior/preprocess/kernel'], P['prior/preprocess/bias'])
    skip = R.conv1d_v2(net, P['prior/skip/kernel'], P['prior/skip/bias'])
    cond = P['prior/speaker_embedding'][spk].unsqueeze(1).repeat(1, T // 64, 1)          # [B, Tz, Cs]
    for i, d in enumerate(cfg['dilation_rates']):
        s = M.layer_scope(i, cfg['num_cycle_layers']).replace('decoder/', 'prior/')
        p = {n[len(s) + 1:]: v for n, v in P.items() if n.startswith(s + '/')}
        s_out, r_out = R.residual_stack(net, p, cfg['dilation_filters'], d, cond)
        skip, net = skip + s_out, net + r_out
    h = R.conv1d_v2(torch.relu(skip), P['prior/postprocess1/kernel'], P['prior/postprocess1/bias'])
    h = R.add_condition(h, cond, P['prior/postprocess1/local_condition/kernel'])
    out = R.conv1d_v2(torch.relu(h), P['prior/postprocess2/kernel'], P['prior/postprocess2/bias'])
    assert out.shape == (B, T, k)
    return out


def ref_step(codes, spk, P, cfg, state):
    for p in P.values():
        p.requires_grad_(True)
        p.grad = None
    logits = ref_logits(codes, spk, P, cfg)
    loss = Fn.cross_entropy(logits.reshape(-1, cfg['quantization_channels']), codes.reshape(-1))
    loss.backward()
    grads = {n: p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p) for n, p in P.items()}   # (the top
    # layer's residual 1x1 feeds nothing: zero gradient)
    for p in P.values():
        p.requires_grad_(False)
    M.adam_ema_step(P, grads, state, M.lr_at(cfg['learning_rate_schedule'], state['t']))
    return logits.detach(), float(loss.detach()), grads


class RefPriorGen:
    """Fast generation of the restatement: FIFO queues (FastConvState), a one-hot input, zero before the first code."""

    def __init__(self, P, cfg, B):
        self.P, self.c, self.B = P, cfg, B
        self.pre = R.FastConvState(cfg['preprocess']['kernel_size'], 1, B, cfg['quantization_channels'])
        self.layers = [R.FastConvState(cfg['kernel_size'], d, B, cfg['residual_filters']) for d in cfg['dilation_rates']]

    def step(self, prev, cond_t):
        """prev int [B] (-1: no code yet) -> probabilities [B,k]."""
        P, c = self.P, self.c
        x = torch.zeros(self.B, c['quantization_channels'])
        for b, q in enumerate(prev):
            if q >= 0:
                x[b, q] = 1.0
        cur = self.pre.step(x, P['prior/preprocess/kernel'], P['prior/preprocess/bias'])
        skip = R.linear(cur, P['prior/skip/kernel'], P['prior/skip/bias'])
        Df = c['dilation_filters']
        for i in range(len(c['dilation_rates'])):
            s = M.layer_scope(i, c['num_cycle_layers']).replace('decoder/', 'prior/')
            net = self.layers[i].step(cur, P[s + '/gated/kernel'], P[s + '/gated/bias'])
            net = net + R.linear(cond_t, P[s + '/gated/local_condition/kernel'])
            g = torch.tanh(net[:, :Df]) * torch.sigmoid(net[:, Df:])
            skip = skip + R.linear(g, P[s + '/skip/kernel'], P[s + '/skip/bias'])
            cur = cur + R.linear(g, P[s + '/residual/kernel'], P[s + '/residual/bias'])
        h = R.linear(torch.relu(skip), P['prior/postprocess1/kernel'], P['prior/postprocess1/bias'])
        h = h + R.linear(cond_t, P['prior/postprocess1/local_condition/kernel'])
        out = R.linear(torch.relu(h), P['prior/postprocess2/kernel'], P['prior/postprocess2/bias'])
        return torch.softmax(out, dim=-1)


def rand_codes(B, T, k, seed):
    c = torch.randint(0, k, (B, T), generator=torch.Generator().manual_seed(seed))
    c[0, :3] = torch.tensor([0, k - 1, 0])
    c[-1, -2:] = torch.tensor([k - 1, 0])
    return c


# ------------------------------------------------------------------ 1. input kernels
@pytest.mark.parametrize('pre_k', [1, 3])
def test_input_kernels(pkg, pre_k):
    K = pkg.kernels
    B, T, k, R_ = 3, 200, 40, 96          # T not a multiple of the 64-step block, R not of the 64-channel block
    codes = rand_codes(B, T, k, 1)
    g = torch.Generator().manual_seed(2)
    w = torch.randn(pre_k, k, R_, generator=g)
    b = torch.randn(R_, generator=g)
    net0 = torch.full((B, R_, T), float('nan'), device='cuda')
    labels = torch.full((B, T), -7, dtype=torch.int32, device='cuda')
    K.prior_input_fwd(codes.int().cuda(), w.cuda(), b.cuda(), net0, labels)
    wn, cn = w.double().numpy(), codes.numpy()
    want = np.broadcast_to(b.double().numpy()[None, :, None], (B, R_, T)).copy()
    for bb in range(B):
        for t in range(T):
            for j in range(pre_k):
                s = t - pre_k + j
                if s >= 0:
                    want[bb, :, t] += wn[j, cn[bb, s]]
    np.testing.assert_allclose(net0.cpu().double().numpy(), want, rtol=1e-6, atol=1e-6)
    assert torch.equal(labels.cpu(), codes.int())
    # the same as conv1d_v2 over the one-hot input
    ref = R.conv1d_v2(R.shift_right(Fn.one_hot(codes, k).double()), w.double(), b.double()).permute(0, 2, 1)
    np.testing.assert_allclose(net0.cpu().double().numpy(), ref.numpy(), rtol=1e-6, atol=1e-6)
    # weight gradient: fp64 scatter, and bitwise equal from run to run
    dnet = torch.randn(B, R_, T, generator=g)
    dw_ref = torch.zeros(pre_k, k, R_, dtype=torch.float64)
    for bb in range(B):
        for s in range(T):
            for j in range(pre_k):
                t = s + pre_k - j
                if t < T:
                    dw_ref[j, cn[bb, s]] += dnet[bb, :, t].double()
    dnet_t = dnet.permute(0, 2, 1).contiguous().cuda()
    order, starts = K.prior_code_buckets(codes.int().cuda(), k)
    dw1 = torch.full((pre_k, k, R_), float('nan'), device='cuda')
    dw2 = torch.full((pre_k, k, R_), float('nan'), device='cuda')
    K.prior_input_wgrad(order, starts, dnet_t, dw1, B=B, T=T)
    order2, starts2 = K.prior_code_buckets(codes.int().cuda(), k)
    K.prior_input_wgrad(order2, starts2, dnet_t, dw2, B=B, T=T)
    assert relerr(dw1, dw_ref) < 1e-5
    assert torch.equal(dw1, dw2)


# ------------------------------------------------------------------ 2. tiny-config step vs the restatement
def test_tiny_step_matches_restatement(pkg):
    cfg = tiny_prior(k=32, pre_k=3)
    B, T, nspk = 2, 512, 10
    prior = pkg.prior.LatentPrior(cfg, nspk, device='cuda', seed=0)
    P = random_params(prior, 7)
    prior.load_named(P)
    state = {'t': 0, 'm': {}, 'v': {}, 'ema': {}}
    spk = torch.tensor([3, 8])
    sd = spk.cuda()
    for step in range(2):
        if step:        # start every step from the restatement's parameters (two fp32 trajectories part), as test_model_gpu.py
            prior.load_named(P, also_ema=False)
        codes = rand_codes(B, T, 32, 10 + step)
        cd = codes.int().cuda()
        ws = prior.forward(cd, sd, compute_grad_seed=False)
        got_logits = ws['logits'].permute(0, 2, 1).cpu()
        ref_lg, ref_loss, ref_grads = ref_step(codes, spk, P, cfg, state)
        assert relerr(got_logits, ref_lg) < 5e-4, 'step %d logits' % step
        ws = prior.train_step(cd, sd)
        loss = prior.losses(ws)[0]
        np.testing.assert_allclose(loss, ref_loss, rtol=2e-5)
        got = prior.named_gradients()
        assert set(got) == set(ref_grads)
        for n, g in ref_grads.items():
            assert relerr(got[n], g) < 2e-3, 'step %d grad %s: %.3g' % (step, n, relerr(got[n], g))
        newp, ema = prior.named_parameters(), prior.named_parameters(ema=True)
        for n in P:
            assert relerr(newp[n], P[n]) < 1e-4, 'step %d param %s' % (step, n)
            assert relerr(ema[n], state['ema'][n]) < 1e-4, 'step %d ema %s' % (step, n)


# ------------------------------------------------------------------ 3. reference widths on the fp16x3 engine
def _ref_width_step(pkg, monkeypatch, engine, defer, codes, spk):
    monkeypatch.setenv('VQW_ENGINE', engine)
    prior = pkg.prior.LatentPrior(default_prior(), 109, device='cuda', seed=0)
    prior.defer_guard = defer
    logits = prior.forward_checked(codes, spk)['logits'].clone()
    prior.train_step(codes, spk)
    prior.finish_steps()
    return prior, logits, prior.named_gradients()


def test_reference_width_step_on_fp16x3(pkg, monkeypatch, capfd):
    B, T = 4, 1024
    codes = rand_codes(B, T, 512, 3).int().cuda()
    spk = torch.tensor([0, 5, 17, 108], device='cuda')
    capfd.readouterr()
    x3, lg3, g3 = _ref_width_step(pkg, monkeypatch, 'f16x3', False, codes, spk)
    err = capfd.readouterr().err
    assert x3.x3_steps == 1 and x3.x3_fallbacks == 0
    assert 'fp32-MFMA engine' not in err, err
    f32, lg32, g32 = _ref_width_step(pkg, monkeypatch, 'fp32', False, codes, spk)
    assert l2err(lg3, lg32) < 5e-4
    for n, g in g32.items():
        assert l2err(g3[n], g) < 5e-3, '%s: %.3g' % (n, l2err(g3[n], g))
    dx3, _, gd = _ref_width_step(pkg, monkeypatch, 'f16x3', True, codes, spk)
    assert dx3.x3_steps == 1
    for n, g in g32.items():
        assert l2err(gd[n], g) < 5e-3, 'deferred %s' % n
    # the deferred flag changes when the flag is read, not the step (bars of test_deferred_guard_matches_immediate: two
    # immediate runs already differ by summation-order noise, which Adam turns into +-lr on near-zero gradients)
    for name in ('flat', 'ema'):
        assert l2err(getattr(dx3, name), getattr(x3, name)) < 3e-3, name


# ------------------------------------------------------------------ 4. sampling vs the restatement
def test_prior_sampling_matches_restatement(pkg, monkeypatch):
    cfg = tiny_prior(k=32, pre_k=3)
    prior = pkg.prior.LatentPrior(cfg, 10, device='cuda', seed=0)
    P = random_params(prior, 11)
    prior.load_named(P)
    spk = torch.tensor([2, 9])
    sd = spk.cuda()
    n = 160                                       # crosses two condition frames
    cond = P['prior/speaker_embedding'][spk]      # [B, Cs], the same in every frame
    gen = pkg.generator.PriorGenerator(prior, batch=2)
    codes, probs = gen.sample(n, sd, return_probs=True)
    got = codes.cpu().numpy()
    assert got.dtype == np.int32 and got.shape == (2, n) and got.min() >= 0 and got.max() < 32
    g = RefPriorGen(P, cfg, 2)
    prev = [-1, -1]
    with torch.no_grad():
        for i in range(n):
            pr = g.step(prev, cond).numpy()
            for b in range(2):
                assert pr[b].max() - pr[b, got[b, i]] <= 2e-6, 'step %d row %d: %d vs argmax %d' % (i, b, got[b, i], pr[b].argmax())
            prev = list(got[:, i])
    np.testing.assert_allclose(probs.cpu().numpy(), pr, rtol=2e-4, atol=1e-7)
    # continued runs == one long run; reset() == a fresh handle (empty history, not code 0)
    gen.reset()
    c1 = gen.sample(100, sd)
    c2 = gen.sample(60, sd)
    assert torch.equal(torch.cat([c1, c2], 1), codes)
    fresh = pkg.generator.PriorGenerator(prior, batch=2)
    assert torch.equal(fresh.sample(n, sd), codes)
    fresh.close()
    # sampled with supplied uniforms
    u = torch.rand(2, n, generator=torch.Generator().manual_seed(0))
    gen.reset()
    si = gen.sample(n, sd, mode='sample', uniforms=u.cuda()).cpu().numpy()
    g = RefPriorGen(P, cfg, 2)
    prev = [-1, -1]
    with torch.no_grad():
        for i in range(n):
            cdf = np.cumsum(g.step(prev, cond).numpy(), axis=1)
            for b in range(2):
                want = min(int(cdf[b].searchsorted(u[b, i].item())), 31)
                if want != si[b, i]:
                    assert np.abs(cdf[b] - u[b, i].item()).min() < 2e-6, 'step %d row %d: %d vs %d' % (i, b, si[b, i], want)
            prev = list(si[:, i])
    # u above the float cdf's last value gives index k, which is no code: clamped to the last code
    for uval in (1.0, 2.0):
        gen.reset()
        top = gen.sample(8, sd, mode='sample', uniforms=torch.full((2, 8), uval, device='cuda'))
        assert int(top.min()) >= 0 and int(top.max()) <= 31
        if uval > 1.0:
            assert (top == 31).all()
    gen.close()
    monkeypatch.setenv('VQW_AR_PERSISTENT', '0')
    with pytest.raises(NotImplementedError, match='persistent'):
        pkg.generator.PriorGenerator(prior, batch=2)


# ------------------------------------------------------------------ 5. condition_from_codes(encode_codes(x)) vs encode(x)
def test_condition_from_codes_equals_encode(pkg):
    import importlib.util
    spec = importlib.util.spec_from_file_location('make_golden', os.path.join(ROOT, 'tests', 'golden', 'make_golden.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    m, w = mod.tiny_cfg()
    P = M.init_params(m, w, 10, seed=11, randomize_all=True)
    model = pkg.model.VQVAE(m, w, 10, device='cuda', seed=0)
    model.load_named(P)
    x, spk, _ = M.synthetic_batch(2, 1024, 10, 1234)
    xd, sd = x[:, :, 0].contiguous().cuda(), spk.cuda()
    enc = model.encode(xd, sd)
    codes = model.encode_codes(xd, sd)
    assert codes.dtype == torch.int32 and tuple(codes.shape) == (2, 16)
    cond = model.condition_from_codes(codes, sd)
    D = model.D
    # the speaker rows are encode()'s bit for bit; the code rows are the chosen embedding rows e_k bit for bit.  encode()'s
    # own rows are the straight-through z_q = z_e + (e_k - z_e) of model.py:73, which equals e_k up to the rounding of
    # that sum in fp32: no function of the codes alone can reproduce those last bits
    assert torch.equal(cond[:, D:], enc[:, D:])
    assert torch.equal(cond[:, :D], model._workspace(2, 1024, train=False)['e_k'])
    assert relerr(cond[:, :D], enc[:, :D]) < 1e-6


# ------------------------------------------------------------------ 6. CLI round trip
def test_cli_train_prior_then_generate(tmp_path):
    w = {"verbose": False, "quantization_channels": 256, "num_cycles": 1, "num_cycle_layers": 4,
         "dilation_rates": [1, 2, 4, 8], "kernel_size": 3, "dilation_filters": 32, "skip_filters": 64,
         "residual_filters": 32, "preprocess": {"kernel_size": 32, "filters": 32}}
    m = {"encoder": "64", "use_vq": True, "speaker_embedding": 16, "k": 32, "latent_dim": 16, "beta": 0.25,
         "encoder_filters": 48, "wavenet_parameters": str(tmp_path / 'w.json'), "verbose": False,
         "learning_rate_schedule": {"0": 1e-3}}
    (tmp_path / 'w.json').write_text(json.dumps(w))
    (tmp_path / 'm.json').write_text(json.dumps(m))
    (tmp_path / 'p.json').write_text(json.dumps(tiny_prior(k=32, pre_k=2)))
    env = dict(os.environ, PYTHONPATH=ROOT)
    cwd = str(tmp_path)
    run = lambda args: subprocess.run([sys.executable] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)  # noqa: E731
    out = run([os.path.join(ROOT, 'train.py'), '-dataset', 'synthetic', '-length', '512', '-batch', '2', '-step', '2',
               '-interval', '2', '-save', 'saved_model/weights', '-params', str(tmp_path / 'm.json')])
    assert out.returncode == 0, out.stderr[-2000:]
    out = run([os.path.join(ROOT, 'train_prior.py'), '-restore', 'saved_model/weights-2.pt', '-dataset', 'synthetic',
               '-length', '128', '-batch', '2', '-step', '4', '-interval', '2', '-save', 'saved_prior/prior',
               '-params', str(tmp_path / 'p.json'), '-vqvae_params', str(tmp_path / 'm.json')])
    assert out.returncode == 0, out.stderr[-2000:]
    assert '[step 4]' in out.stdout and '[prior ' in out.stdout
    assert (tmp_path / 'saved_prior' / 'prior-4.pt').exists()
    (tmp_path / 'data').mkdir()
    (tmp_path / 'data' / 'vctk_speakers.txt').write_text('p225, 3\np226, 5\n')
    out = run([os.path.join(ROOT, 'generate.py'), '-restore', 'saved_model/weights-2.pt', '-prior', 'saved_prior/prior-4.pt',
               '-frames', '32', '-speakers', 'p225', 'None', '-mode', 'sample', '-seed', '3', '-params', str(tmp_path / 'm.json'),
               '-prior_params', str(tmp_path / 'p.json')])
    assert out.returncode == 0, out.stderr[-2000:]
    from scipy.io import wavfile
    for s in ('p225', 'no_speaker'):
        sr, a = wavfile.read(str(tmp_path / 'saved_model' / ('2_%s_prior.wav' % s)))
        assert sr == 16000 and a.shape == (32 * 64,) and np.isfinite(a).all() and np.abs(a).max() <= 1.0
        c = np.load(str(tmp_path / 'saved_model' / ('prior_codes_2_%s.npy' % s)))
        assert c.shape == (32,) and c.min() >= 0 and c.max() < 32
