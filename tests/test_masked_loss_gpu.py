"""GPU tests of length-masked prior training: vqw_softmax_xent_ranged against the float64 reference of
tests/masked_ref.py and, bit for bit, against vqw_softmax_xent; LatentPrior.train_step(lengths=) against the float64
restatement of the masked step at the tiny config and, on the fp16x3 engine, at the reference widths, in both guard modes;
the deferred guard's repeat with each step's own lengths; train_prior.py -whole_utterances end to end.

Bars: the kernel's are pointwise_ref.softmax_bars, what the unmasked kernel is held to; the model's are those of
tests/test_prior_gpu.py (loss rtol 2e-5, gradients 2e-3 of the per-tensor max at the tiny config, 5e-3 relative L2 at the
reference widths, parameters / EMA after Adam 1e-4) and of test_model_gpu.py::test_deferred_guard_matches_immediate."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import masked_ref as MR  # noqa: E402
import pointwise_ref as PR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class DBuf:
    """The device twin of a pointwise_ref.Buf (as in test_pointwise_kernels_gpu.py): `view` is what the kernel gets."""

    def __init__(self, n, init=None):
        self.buf = PR.Buf(n, 0, init)
        self.full = _dev(self.buf.full)
        self.view = self.full[self.buf.lo:self.buf.lo + n]

    def host(self):
        return self.full.cpu().numpy()

    def check(self, vals, bar, what):
        return PR.compare(self.host(), self.buf, vals, bar, None, what)

    def untouched(self, what):
        return PR.compare(self.host(), self.buf, self.buf.view, None, np.zeros(self.buf.n, dtype=bool), what)


def l2err(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm()) / max(float(b.norm()), 1e-30)


def relerr(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-12)


# ---------------------------------------------------------------------------------------------------- the kernel
def range_sets(T):
    """(name, t_begin, t_end) for B = 4 rows each; None: the NULL pointer.  Values past T are clamped by the kernel."""
    return [('full-empty-crossed-one', [0, 0, 5, 0], [T, 0, 3, 1]),
            ('ends', [0, 0, 0, 0], [63, 64, 65, T - 1]),
            ('begins', [1, 64, 1, 64], [T, T, 65, T - 1]),
            ('crossed-equal', [T, 64, 1, 0], [T, 64, 1, T]),
            ('null-begin', None, [T, 0, 1, T - 1]),
            ('null-end', [0, 1, 64, T], None),
            ('null-both', None, None)]


@pytest.mark.parametrize('T', PR.SOFTMAX_T)
@pytest.mark.parametrize('Q', [4, 68, 256, 512])
def test_softmax_xent_ranged_matches_reference_and_the_unmasked_kernel(K, Q, T):
    B = 4
    sd = PR.seed_of('xent-ranged', Q, T)
    x = PR.randn(sd, B, Q, T) * np.float32(3.0)
    lab = np.random.RandomState(sd + 1).randint(0, Q, (B, T)).astype(np.int32)
    gs = float(np.float32(1.0 / 37.0))
    dx, dlab = _dev(x), _dev(lab)
    # what the unmasked kernel writes for the same logits and grad_scale: the scored positions' bits
    ud, up = torch.empty(B, Q, T, device=DEV), torch.empty(B, Q, T, device=DEV)
    K.softmax_xent(dx, dlab, loss_sum=torch.zeros(1, device=DEV), dlogits=ud, probs=up, grad_scale=gs)
    ubits = {'d': ud.cpu().numpy().view(np.uint32), 'p': up.cpu().numpy().view(np.uint32)}
    for name, tb, te in range_sets(T):
        ref = MR.xent_ranged_ref(x, lab, gs, tb, te)
        bars = MR.xent_ranged_bars(ref, lab, gs)
        m3 = np.broadcast_to(ref['mask'][:, None, :], x.shape)
        want_ls = PR.SOFTMAX_LOSS0 + ref['loss'].sum()
        dtb = None if tb is None else _dev(np.asarray(tb, np.int32))
        dte = None if te is None else _dev(np.asarray(te, np.int32))
        nan_x = _dev(np.where(m3, x, np.float32('nan')))
        runs = [('fused', d, p, poison) for d in (False, True) for p in (False, True) for poison in (False,)]
        runs += [('in_place', True, False, False), ('fused', True, True, True), ('in_place', True, False, True)]
        for entry, with_d, with_p, poison in runs:
            what = 'Q=%d T=%d %s %s dlogits=%d probs=%d nan_outside=%d' % (Q, T, name, entry, with_d, with_p, poison)
            src = nan_x if poison else dx
            ls = DBuf(1, init=[PR.SOFTMAX_LOSS0])
            pb = DBuf(x.size) if with_p else None
            db = (DBuf(x.size, init=src.cpu().numpy()) if entry == 'in_place' else DBuf(x.size)) if with_d else None
            pv = pb.view.view(B, Q, T) if with_p else None
            dv = db.view.view(B, Q, T) if with_d else None
            K.softmax_xent_ranged(dv if entry == 'in_place' else src, dlab, loss_sum=ls.view, dlogits=dv, probs=pv, grad_scale=gs,
                                  t_begin=dtb, t_end=dte)
            ls.check([want_ls], bars['loss_sum'], what + ' loss_sum')
            for key, buf, bar, want in (('p', pb, bars['p'], ref['p']), ('d', db, bars['dlogits'], ref['d'])):
                if buf is None:
                    continue
                buf.check(want, bar, what + ' ' + key)            # (guard bands bit-equal; scored positions within the bars)
                got = buf.view.cpu().numpy().reshape(x.shape)
                assert np.isfinite(got).all(), what + ': a non-finite ' + key
                bits = got.view(np.uint32)
                assert (bits[~m3] == 0).all(), what + ': an unscored %s is not +0.0f' % key
                assert np.array_equal(bits[m3], ubits[key][m3]), what + ': scored %s differs from vqw_softmax_xent in its bits' % key


def test_softmax_xent_ranged_refuses_q_6_and_writes_nothing(K):
    B, Q, T = 2, 6, 10
    x, lab = _dev(PR.randn(1, B, Q, T)), _dev(np.zeros((B, T), np.int32))
    ls, d, p = DBuf(1), DBuf(B * Q * T), DBuf(B * Q * T)
    with pytest.raises(RuntimeError, match='must be a multiple of 4'):
        K.softmax_xent_ranged(x, lab, loss_sum=ls.view, dlogits=d.view.view(B, Q, T), probs=p.view.view(B, Q, T),
                              t_end=_dev(np.array([3, 10], np.int32)))
    with pytest.raises(ValueError, match='t_end must be int32'):
        K.softmax_xent_ranged(x, lab, loss_sum=ls.view, t_end=torch.zeros(1, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    for b in (ls, d, p):
        b.untouched('softmax_xent_ranged with Q = 6')


# ---------------------------------------------------------------------------------------------------- the model
def tiny_prior(k=32, pre_k=3):
    return {"quantization_channels": k, "num_cycles": 2, "num_cycle_layers": 4, "dilation_rates": [1, 2, 4, 8, 1, 2, 4, 8],
            "kernel_size": 3, "dilation_filters": 32, "skip_filters": 64, "residual_filters": 32,
            "preprocess": {"kernel_size": pre_k, "filters": 32}, "speaker_embedding": 16, "learning_rate_schedule": {"0": 1e-3}}


def wide_prior():
    """prior_parameters.json's widths, two layers."""
    with open(os.path.join(ROOT, 'prior_parameters.json')) as f:
        cfg = json.load(f)
    cfg.update(dilation_rates=[1, 2], num_cycles=1, num_cycle_layers=2)
    return cfg


def rand_codes(B, T, k, seed):
    return torch.randint(0, k, (B, T), generator=torch.Generator().manual_seed(seed))        # (random in the padding too)


def _seed_is_zero_behind(ws, lengths):
    """ws['logits'] after a step is the gradient seed: exactly +0.0 from lengths[b] on, and not all zero before."""
    seed = ws['logits']
    for b, n in enumerate(lengths):
        assert (seed[b, :, n:].contiguous().view(torch.int32) == 0).all(), 'row %d: the gradient seed is not +0.0 behind its length' % b
        assert bool((seed[b, :, :n] != 0).any()), 'row %d: no gradient seed inside its length' % b


def test_tiny_masked_step_matches_restatement(pkg):
    cfg = tiny_prior()
    B, T, lengths, nspk = 3, 512, (512, 193, 64), 10
    prior = pkg.prior.LatentPrior(cfg, nspk, device=DEV, seed=0)
    P = MR.random_params(prior.named_parameters(), 7)
    prior.load_named(P)
    state = {'t': 0, 'm': {}, 'v': {}, 'ema': {}}
    spk = torch.tensor([3, 8, 0])
    sd = spk.cuda()
    for step in range(2):
        if step:        # start every step from the restatement's parameters (two trajectories part), as test_prior_gpu.py
            prior.load_named(P, also_ema=False)
        codes = rand_codes(B, T, 32, 10 + step)
        ref_loss, ref_grads = MR.masked_step(codes, spk, lengths, P, cfg, state)
        ws = prior.train_step(codes.int().cuda(), sd, lengths=lengths)
        assert ws['count'] == sum(lengths)
        loss = prior.losses(ws)[0]
        print('step %d: loss %.9g, restatement %.9g' % (step, loss, ref_loss))
        np.testing.assert_allclose(loss, ref_loss, rtol=2e-5)
        _seed_is_zero_behind(ws, lengths)
        got = prior.named_gradients()
        assert set(got) == set(ref_grads)
        for n, g in ref_grads.items():
            assert relerr(got[n], g) < 2e-3, 'step %d grad %s: %.3g' % (step, n, relerr(got[n], g))
        newp, ema = prior.named_parameters(), prior.named_parameters(ema=True)
        for n in P:
            assert relerr(newp[n], P[n]) < 1e-4, 'step %d param %s' % (step, n)
            assert relerr(ema[n], state['ema'][n]) < 1e-4, 'step %d ema %s' % (step, n)
    assert prior.global_step == 2


_WIDE = {}


def _wide_reference(pkg):
    """The float64 restatement's loss and gradients of the reference-width problem, computed once."""
    if not _WIDE:
        cfg = wide_prior()
        named = pkg.prior.LatentPrior(cfg, 109, device='cpu', seed=0).named_parameters()
        P = {n: v.double() for n, v in named.items()}
        codes, spk, lengths = rand_codes(2, 512, 512, 3), torch.tensor([5, 108]), (512, 256)
        loss, grads = MR.loss_and_grads(MR.padded_loss, codes, spk, lengths, P, cfg)
        _WIDE.update(cfg=cfg, codes=codes, spk=spk, lengths=lengths, loss=loss, grads=grads)
    return _WIDE


@pytest.mark.parametrize('defer', [False, True], ids=['immediate', 'deferred'])
def test_reference_width_masked_step_on_fp16x3(pkg, monkeypatch, capfd, defer):
    W = _wide_reference(pkg)
    monkeypatch.setenv('VQW_ENGINE', 'f16x3')
    capfd.readouterr()
    prior = pkg.prior.LatentPrior(W['cfg'], 109, device=DEV, seed=0)
    prior.defer_guard = defer
    ws = prior.train_step(W['codes'].int().cuda(), W['spk'].cuda(), lengths=W['lengths'])
    prior.finish_steps()
    err = capfd.readouterr().err
    assert prior.x3_steps == 1 and prior.x3_fallbacks == 0 and prior.global_step == 1
    assert 'fp32-MFMA engine' not in err, err
    np.testing.assert_allclose(prior.losses(ws)[0], W['loss'], rtol=2e-5)
    _seed_is_zero_behind(ws, W['lengths'])
    got = prior.named_gradients()
    assert set(got) == set(W['grads'])
    for n, g in W['grads'].items():
        assert l2err(got[n], g) < 5e-3, '%s: %.3g' % (n, l2err(got[n], g))


def test_deferred_guard_repeats_each_step_with_its_own_lengths(pkg, monkeypatch):
    """dp_worker.guard_problem's recipe for raising the range flag in the first step: a scaled preprocess kernel (and gate
    kernels scaled down by as much, which keeps the gates unsaturated).  Its factor 3e5 is sized for the VQ-VAE's 32-tap
    preprocess kernel over audio (|w| <= 0.31: |net| ~ 1e5); the prior's is ONE row of a [1][512][256] kernel per step,
    |w| <= sqrt(3 / 512) = 0.077, so 3e5 would leave |net| <= 2.3e4, inside fp16's 65504 at a fresh model's plane scale of 1.0,
    and raise nothing.  3e6 puts |net| at up to 2.3e5: the layer-input planes of layer 1 leave fp16's range, as the recipe means.
    Deferred: the step behind the flagged one is enqueued before the flag is read; then the first is repeated on the fp32
    engine and the second run again, each with ITS lengths -- the state is that of the same two steps in the immediate mode."""
    monkeypatch.setenv('VQW_ENGINE', 'f16x3')
    cfg = wide_prior()
    steps = [(rand_codes(2, 512, 512, 21).int().cuda(), (512, 64)), (rand_codes(2, 512, 512, 22).int().cuda(), (64, 512))]
    spk = torch.tensor([5, 108], device=DEV)
    models = []
    for defer in (False, True):
        prior = pkg.prior.LatentPrior(cfg, 109, device=DEV, seed=0)
        P = prior.named_parameters()
        P['prior/preprocess/kernel'] *= 3e6
        for name in P:
            if name.endswith('/gated/kernel'):
                P[name] *= 1e-6
        prior.load_named(P)
        prior.defer_guard = defer
        for i, (codes, lengths) in enumerate(steps):
            ws = prior.train_step(codes, spk, lengths=lengths)
            if defer and i == 0:     # the flagged step's verdict is still on the device when the second step is enqueued behind it
                assert len(prior._pending) == 1 and prior.x3_fallbacks == 0
        prior.finish_steps()
        assert prior.x3_fallbacks == 1 and prior.global_step == 2, (prior.x3_fallbacks, prior.global_step, prior.x3_steps)
        assert ws['count'] == 576
        _seed_is_zero_behind(ws, steps[1][1])
        models.append(prior)
    a, b = models
    for name, bar in (('flat', 3e-3), ('ema', 3e-3), ('adam_v', 2e-1), ('adam_m', 3e-1)):      # test_deferred_guard_matches_immediate's
        ta, tb = getattr(a, name), getattr(b, name)
        assert torch.isfinite(tb).all(), name
        print('%s: deferred vs immediate rel. L2 %.3e' % (name, l2err(tb, ta)))
        assert l2err(tb, ta) < bar, '%s: deferred vs immediate rel. L2 %.3e' % (name, l2err(tb, ta))


# ---------------------------------------------------------------------------------------------------- command line
def test_cli_train_prior_whole_utterances_then_generate(tmp_path):
    from test_score_cpu import write_dataset
    w = {"verbose": False, "quantization_channels": 256, "num_cycles": 1, "num_cycle_layers": 4,
         "dilation_rates": [1, 2, 4, 8], "kernel_size": 3, "dilation_filters": 32, "skip_filters": 64,
         "residual_filters": 32, "preprocess": {"kernel_size": 32, "filters": 32}}
    m = {"encoder": "64", "use_vq": True, "speaker_embedding": 16, "k": 32, "latent_dim": 16, "beta": 0.25,
         "encoder_filters": 48, "wavenet_parameters": str(tmp_path / 'w.json'), "verbose": False,
         "learning_rate_schedule": {"0": 1e-3}}
    (tmp_path / 'w.json').write_text(json.dumps(w))
    (tmp_path / 'm.json').write_text(json.dumps(m))
    (tmp_path / 'p.json').write_text(json.dumps(tiny_prior(k=32, pre_k=2)))
    root = str(tmp_path / 'data')          # a held-out list of three short utterances (synthetic training has 109 speakers)
    rels = write_dataset(root, [1000, 5000, 700], speakers=['p%d' % (225 + i) for i in range(109)])
    (tmp_path / 'held.txt').write_text('\n'.join(rels) + '\n')
    env = dict(os.environ, PYTHONPATH=ROOT)
    run = lambda args: subprocess.run([sys.executable] + args, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)  # noqa: E731
    out = run([os.path.join(ROOT, 'train.py'), '-dataset', 'synthetic', '-length', '512', '-batch', '2', '-step', '2',
               '-interval', '2', '-save', 'saved_model/weights', '-params', str(tmp_path / 'm.json')])
    assert out.returncode == 0, out.stderr[-2000:]
    out = run([os.path.join(ROOT, 'train_prior.py'), '-restore', 'saved_model/weights-2.pt', '-dataset', 'synthetic',
               '-whole_utterances', '-min_frames', '16', '-length', '256', '-batch', '2', '-step', '3', '-interval', '1',
               '-save', 'saved_prior/prior', '-params', str(tmp_path / 'p.json'), '-vqvae_params', str(tmp_path / 'm.json'),
               '-eval_list', str(tmp_path / 'held.txt'), '-eval_interval', '2', '-eval_batches', '1', '-data_root', root])
    assert out.returncode == 0, out.stderr[-2000:]
    assert '[step 3]' in out.stdout and '[prior ' in out.stdout and '[scored ' in out.stdout, out.stdout[-500:]
    lines = out.stdout.splitlines()             # (text mode: the console line's carriage returns read as line ends)
    assert ['[eval bits/code ' in ln for ln in lines if ln.startswith('[step ')] == [False, True, False], out.stdout[-500:]
    bits = float([ln for ln in lines if '[eval bits/code ' in ln][0].split('[eval bits/code ')[1].split(']')[0])
    assert 0 < bits < 16                   # (32 codes: 5 bits for a prior that knows nothing)
    assert (tmp_path / 'saved_prior' / 'prior-3.pt').exists()
    out = run([os.path.join(ROOT, 'generate.py'), '-restore', 'saved_model/weights-2.pt', '-prior', 'saved_prior/prior-3.pt',
               '-frames', '32', '-speakers', 'p225', '-mode', 'sample', '-seed', '3', '-params', str(tmp_path / 'm.json'),
               '-prior_params', str(tmp_path / 'p.json')])
    assert out.returncode == 0, out.stderr[-2000:]
    c = np.load(str(tmp_path / 'saved_model' / 'prior_codes_2_p225.npy'))
    assert c.shape == (32,) and c.min() >= 0 and c.max() < 32
