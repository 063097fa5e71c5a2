"""GPU tests of the codebook by moving averages with dead-code restart: both kernels bit for bit against the
numpy restatement (codebook_ref.py), their argument checks, the model's training step against an autograd restatement, "off is
off", one update per applied step under the range guard (immediate and deferred), resume, two data-parallel ranks and the
command line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import ref_model as M

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import codebook_ref as CR  # noqa: E402
from test_jitter_gpu import STATE, _batches, bits, reproducible_cfg  # noqa: E402
from test_model_gpu import _guarded_model, build, relerr, tiny_cfg  # noqa: E402
from test_multirank_gpu import run_ranks  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32

# (3, 64, 104, 512): the benchmark's latent shape per row; (1, 4, 1, 3): one frame, fewer codes than lanes; (2, 8, 65, 70): the
# frames cross a 64-lane chunk, K is no multiple of the four waves of a block; (5, 12, 257, 33)
SHAPES = [(3, 64, 104, 512), (1, 4, 1, 3), (2, 8, 65, 70), (5, 12, 257, 33)]
CB_KEYS = ('cb_pack', 'cb_cnt', 'cb_pick', 'cb_u', 'cb_stats', 'cb_sum', 'cb_cand')


def nbits(a):
    return torch.from_numpy(np.ascontiguousarray(a)).view(torch.int32)


def same_bits(t, a):
    return torch.equal(bits(t).cpu(), nbits(np.asarray(a, f32)))


# ------------------------------------------------------------------ 1: the statistics kernel
@pytest.mark.parametrize('pattern', ['random', 'one_code', 'ends'])
@pytest.mark.parametrize('B,D,Tz,Kc', SHAPES)
def test_stats_kernel_bit_exact(K, B, D, Tz, Kc, pattern):
    rng = np.random.default_rng(B * 1000 + D * 10 + Tz)
    Nf = B * Tz
    z = rng.standard_normal((B, D, Tz)).astype(f32)
    z[:, :, ::3] *= f32(0.0)                       # signed zeros: +0.0 + (-0.0) = +0.0
    one = Kc // 2
    idx = {'random': rng.integers(0, Kc, (B, Tz)), 'one_code': np.full((B, Tz), one),
           'ends': np.where(rng.random((B, Tz)) < 0.5, 0, Kc - 1)}[pattern].astype(np.int64)
    pick = rng.integers(0, Nf, Kc).astype(np.int32)
    pick[0], pick[-1] = 0, Nf - 1
    if Kc > 3:
        pick[1], pick[2] = Nf + 3, -5                # outside [0, Nf): clamped to Nf - 1 and 0
    cnt_w, sum_w, cand_w = CR.stats(z, idx, Kc, pick)
    if pattern == 'one_code':
        assert cnt_w[one] == Nf and (np.delete(cnt_w, one) == 0).all() and (np.delete(sum_w, one, 0).view(np.int32) == 0).all()
    zd, idd, pd = torch.from_numpy(z).cuda(), torch.from_numpy(idx).cuda(), torch.from_numpy(pick).cuda()
    for with_cand in (True, False):
        cnt = torch.full((Kc,), -7, dtype=torch.int32, device='cuda')
        tot, cand = torch.full((Kc, D), float('nan'), device='cuda'), torch.full((Kc, D), float('nan'), device='cuda')
        K.vq_cluster_stats(zd, idd, cnt=cnt, sum=tot, pick=pd if with_cand else None, cand=cand if with_cand else None, K=Kc)
        assert torch.equal(cnt.cpu(), torch.from_numpy(cnt_w))
        assert same_bits(tot, sum_w)
        if with_cand:
            assert same_bits(cand, cand_w)
            assert same_bits(cand[0], z[0, :, 0]) and same_bits(cand[-1], z[B - 1, :, Tz - 1])
        else:
            assert bool(torch.isnan(cand).all())
    assert torch.equal(zd.cpu(), torch.from_numpy(z)) and torch.equal(idd.cpu(), torch.from_numpy(idx))


# ------------------------------------------------------------------ 2: the update kernel
def update_case(seed, Kc=70, D=12, tau=0.3):
    """Random state with the three branches in one call (decay 0.5), codes 0 and 1 on the two sides of the threshold."""
    rng = np.random.default_rng(seed)
    E, m = rng.standard_normal((Kc, D)).astype(f32), rng.standard_normal((Kc, D)).astype(f32)
    n = (rng.random(Kc) * 2).astype(f32)
    cnt = np.where(rng.random(Kc) < 0.5, 0, rng.integers(1, 9, Kc)).astype(np.int32)
    t = f32(tau)
    n[0], n[1] = t / f32(0.5), np.nextafter(t, f32(0)) / f32(0.5)
    cnt[0] = cnt[1] = 0
    n[2], cnt[2] = f32(0.1), 0          # dead and unused
    n[3], cnt[3] = f32(0.1), 3          # alive through its count
    n[4], cnt[4] = f32(1.5), 0          # alive, unused: E untouched
    tot = np.where(cnt[:, None] > 0, rng.standard_normal((Kc, D)), 0).astype(f32)
    cand = rng.standard_normal((Kc, D)).astype(f32)
    return E, n, m, cnt, tot, cand


def test_update_kernel_bit_exact(K):
    tau = 0.3
    E, n, m, cnt, tot, cand = update_case(5, tau=tau)
    E_w, n_w, m_w, info_w = CR.update(E, n, m, cnt, tot, cand, 0.5, tau)
    g = f32(0.5)
    dead = (g * n + f32(1 - 0.5) * cnt.astype(f32)) < f32(tau)
    assert not dead[0] and dead[1] and dead[2] and not dead[3] and not dead[4]
    assert dead.sum() >= 2 and ((cnt > 0) & ~dead).sum() >= 2 and ((cnt == 0) & ~dead).sum() >= 2      # restarted, updated, untouched
    assert np.array_equal(E_w[4].view(np.int32), E[4].view(np.int32)) and n_w[0] == f32(tau) and n_w[1] == 1
    dev = lambda a: torch.from_numpy(a.copy()).cuda()  # noqa: E731
    for case in ('restart', 'tau0', 'skip0', 'skip1'):
        Ed, nd, md = dev(E), dev(n), dev(m)
        info = torch.tensor([5, 6, 0, 0, 0, 0, 0, 0], dtype=torch.int32, device='cuda')
        cd, sd, qd = dev(cnt), dev(tot), dev(cand)
        if case == 'tau0':
            want = CR.update(E, n, m, cnt, tot, None, 0.5, 0.0)
            K.vq_codebook_ema_step(Ed, nd, md, cnt=cd, sum=sd, cand=None, decay=0.5, restart=0.0, info=info)
            assert want[3].tolist() == [0, int((cnt > 0).sum())]
        elif case == 'skip1':
            want = (E, n, m, np.array([5, 6], np.int32))
            K.vq_codebook_ema_step(Ed, nd, md, cnt=cd, sum=sd, cand=qd, decay=0.5, restart=tau, info=info,
                                   skip=torch.ones(1, dtype=torch.int32, device='cuda'))
        else:
            want = (E_w, n_w, m_w, info_w)
            skip = torch.zeros(1, dtype=torch.int32, device='cuda') if case == 'skip0' else None
            for _ in range(2 if case == 'restart' else 1):       # info is that of the call, not a running total
                Ed, nd, md = dev(E), dev(n), dev(m)
                K.vq_codebook_ema_step(Ed, nd, md, cnt=cd, sum=sd, cand=qd, decay=0.5, restart=tau, info=info, skip=skip)
        assert same_bits(Ed, want[0]), case
        assert same_bits(nd, want[1]), case
        assert same_bits(md, want[2]), case
        assert info.cpu().tolist() == want[3].tolist() + [0] * 6, case
        assert torch.equal(cd.cpu(), torch.from_numpy(cnt)) and same_bits(sd, tot) and same_bits(qd, cand)


# ------------------------------------------------------------------ 3: argument checks
def test_argument_checks_return_errors(pkg, K):
    L = pkg._lib
    lib, ptr, st = L.lib(), L.ptr, L.stream()
    B, D, Tz, Kc = 2, 4, 9, 6
    z = torch.randn(B, D, Tz, device='cuda')
    idx = torch.zeros(B, Tz, dtype=torch.int64, device='cuda')
    pick = torch.zeros(Kc, dtype=torch.int32, device='cuda')
    cnt = torch.full((Kc,), -7, dtype=torch.int32, device='cuda')
    tot, cand = torch.full((Kc, D), -3.5, device='cuda'), torch.full((Kc, D), -3.5, device='cuda')
    stats, step = lib.vqw_vq_cluster_stats, lib.vqw_vq_codebook_ema_step
    good = [ptr(z), ptr(idx), ptr(pick), ptr(cnt), ptr(tot), ptr(cand)]
    for i in range(6):
        args = list(good)
        args[i] = None
        assert stats(*args, B, D, Tz, Kc, st) != 0
        assert b'null pointer' in lib.vqw_last_error()
    for dims in ((0, D, Tz, Kc), (B, 0, Tz, Kc), (B, D, 0, Kc), (B, D, Tz, 0), (B, D, -3, Kc)):
        assert stats(*good, *dims, st) != 0
        assert b'positive' in lib.vqw_last_error()
    big = torch.full((B * D * Tz,), -3.5, device='cuda')            # an output inside an input
    assert stats(ptr(big), ptr(idx), ptr(pick), ptr(cnt), ptr(big[8:]), ptr(cand), B, D, Tz, Kc, st) != 0
    assert b'alias' in lib.vqw_last_error()
    assert stats(ptr(z), ptr(idx), ptr(pick), ptr(cnt), ptr(tot), ptr(tot), B, D, Tz, Kc, st) != 0
    assert b'alias' in lib.vqw_last_error()
    assert stats(ptr(z), ptr(idx), ptr(pick), ptr(pick), ptr(tot), ptr(cand), B, D, Tz, Kc, st) != 0
    emb, m = torch.full((Kc, D), 2.5, device='cuda'), torch.full((Kc, D), 2.5, device='cuda')
    n = torch.full((Kc,), 2.5, device='cuda')
    info = torch.full((8,), 0, dtype=torch.int32, device='cuda')
    cnt2 = torch.ones(Kc, dtype=torch.int32, device='cuda')
    good = [ptr(emb), ptr(n), ptr(m), ptr(cnt2), ptr(tot), ptr(cand)]
    tail = (0.5, 0.5, 0.25, ptr(info), None, Kc, D, st)
    for i in range(6):
        args = list(good)
        args[i] = None
        assert step(*args, *tail) != 0
        assert b'null pointer' in lib.vqw_last_error()
    assert step(*good, 0.5, 0.5, 0.25, None, None, Kc, D, st) != 0
    assert step(*good[:5], None, 0.5, 0.5, 0.0, ptr(info), None, Kc, D, st) == 0            # tau = 0: cand may be NULL (this one runs)
    torch.cuda.synchronize()
    assert info[:2].tolist() == [0, Kc] and int(info[2:].abs().max()) == 0
    emb.fill_(2.5), n.fill_(2.5), m.fill_(2.5), info.zero_()
    for dims in ((0, D), (Kc, 0), (-1, D)):
        assert step(*good, 0.5, 0.5, 0.25, ptr(info), None, *dims, st) != 0
        assert b'positive' in lib.vqw_last_error()
    for g, h, tau in ((0.0, 0.5, 0.1), (1.0, 0.5, 0.1), (0.5, 0.0, 0.1), (0.5, 0.5, 1.0), (0.5, 0.5, -0.1), (float('nan'), 0.5, 0.1)):
        assert step(*good, g, h, tau, ptr(info), None, Kc, D, st) != 0
    assert step(ptr(emb), ptr(n), ptr(emb), ptr(cnt2), ptr(tot), ptr(cand), *tail) != 0
    assert b'alias' in lib.vqw_last_error()
    assert step(ptr(emb), ptr(n), ptr(m), ptr(cnt2), ptr(m), ptr(cand), *tail) != 0
    assert b'alias' in lib.vqw_last_error()
    assert step(ptr(emb), ptr(n), ptr(m), ptr(cnt2), ptr(tot), ptr(cand), 0.5, 0.5, 0.25, ptr(info), ptr(info[1:]), Kc, D, st) != 0
    with pytest.raises(ValueError):
        K.vq_cluster_stats(z, idx, cnt=cnt, sum=tot, pick=pick, cand=None, K=Kc)
    with pytest.raises(ValueError):
        K.vq_cluster_stats(z, idx, cnt=cnt, sum=tot[:, :D - 1].contiguous(), K=Kc)          # sum too small
    with pytest.raises(ValueError):
        K.vq_codebook_ema_step(emb, n, m, cnt=cnt2, sum=tot, cand=None, decay=0.5, restart=0.25, info=info)
    with pytest.raises(ValueError):
        K.vq_codebook_ema_step(emb, n, m, cnt=cnt2, sum=tot, cand=cand, decay=1.0, info=info)
    torch.cuda.synchronize()                             # nothing else was launched
    assert int((cnt != -7).sum()) == 0 and bool((tot == -3.5).all()) and bool((cand == -3.5).all())
    assert bool((emb == 2.5).all()) and bool((n == 2.5).all()) and bool((m == 2.5).all()) and int(info.abs().max()) == 0


# ------------------------------------------------------------------ 4: the model's step against autograd
def ref_step_ema(x, spk, P, m, w):
    """ref_step of tests/test_jitter_gpu.py without jitter and with loss = CE + beta * commitment: no codebook term."""
    for n_, p_ in P.items():
        p_.requires_grad_(M.is_trainable(n_))
        p_.grad = None
    z_e = M.encoder_64(x, P)
    q, e_k, z_q = M.discretise(z_e, P['embedding/embedding'])
    h = P['speaker_embedding'][spk].unsqueeze(1)
    logits, labels = M.wavenet_build(x, M.R.concat(z_q, h), P, w)
    out = {'q': q, 'z_e': z_e, 'logits': logits, 'labels': labels,
           'reconstruction_loss': torch.nn.functional.cross_entropy(logits, labels.long(), reduction='mean')}
    out['vq_loss'] = torch.mean((z_e.detach() - e_k.detach()) ** 2)
    out['loss'] = out['reconstruction_loss'] + m['beta'] * torch.mean((z_e - e_k.detach()) ** 2)
    out['loss'].backward()
    grads = {n_: p_.grad.detach().clone() for n_, p_ in P.items() if p_.grad is not None}
    for p_ in P.values():
        p_.requires_grad_(False)
    return out, grads


@pytest.mark.parametrize('tau', [0.0, 0.999], ids=['no_restart', 'restart'])
def test_model_step_matches_autograd(pkg, tau):
    """The tiny configuration, B = 2, T = 512 (Tz = 8, 16 frames), decay 0.9.  Bars: those run_parity holds for this configuration
    (test_tiny_model_two_steps: gradients 2e-3 of the tensor's max, idx equal, losses rtol 2e-5).  tau = 0.999: n' = 0.9 < tau for
    every code that won no frame, so each of them restarts."""
    m, w = tiny_cfg()
    P = M.init_params(m, w, 10, seed=11, randomize_all=True)
    x, spk, _ = M.synthetic_batch(2, 512, 10, 1234)
    xd, sd = x[:, :, 0].contiguous().cuda(), spk.cuda()
    out, grads = ref_step_ema(x, spk, P, m, w)
    model = build(pkg, dict(m, codebook_ema=0.9, codebook_restart=tau), w, 10, P)
    Kc, D = model.Kc, model.D
    E0 = P['embedding/embedding'].detach().numpy().astype(f32).copy()
    shadow0 = model.E['embedding'].clone()
    ws = model.train_step(xd, sd)
    assert ws['cb_stats'] and model.global_step == 1
    assert torch.equal(ws['idx'].cpu(), out['q'])
    assert relerr(ws['z_e'].permute(0, 2, 1), out['z_e']) < 2e-4
    loss, recon, vq, commit = model.losses(ws)
    np.testing.assert_allclose(recon, out['reconstruction_loss'].item(), rtol=2e-5)
    np.testing.assert_allclose(vq, out['vq_loss'].item(), rtol=2e-5)
    np.testing.assert_allclose(commit, m['beta'] * out['vq_loss'].item(), rtol=2e-5)
    np.testing.assert_allclose(loss, out['loss'].item(), rtol=2e-5)
    got = model.named_gradients()
    assert 'embedding/embedding' not in grads
    for name, gref in grads.items():
        e = relerr(got[name], gref)
        assert e < 2e-3, 'grad %s err %.3e' % (name, e)
    assert int((got['embedding/embedding'] != 0).sum()) == 0
    o, shp = model.seg_off['embedding']
    assert int((model.adam_m[o:o + Kc * D] != 0).sum()) == 0 and int((model.adam_v[o:o + Kc * D] != 0).sum()) == 0
    u = model.codebook_uniforms(Kc, 0).cpu().numpy()
    z_dev, idx_dev = ws['z_e'].cpu().numpy(), ws['idx'].cpu().numpy()
    E1, n1, m1, info = CR.step(E0, np.ones(Kc, f32), E0, z_dev, idx_dev, u, 0.9, tau)
    assert same_bits(model.P['embedding'], E1) and same_bits(model.vq_ema_n, n1) and same_bits(model.vq_ema_m, m1)
    used = len(set(idx_dev.reshape(-1).tolist()))
    assert info.tolist() == [Kc - used if tau > 0 else 0, used]
    assert model.codebook_info() == {'used': int(info[1]), 'restarted': int(info[0])}
    assert not np.array_equal(E1, E0)
    want = 0.999 * shadow0.double() + 0.001 * torch.from_numpy(E1).cuda().double()
    assert float((model.E['embedding'].double() - want).abs().max()) <= 1e-6 * float(want.abs().max())
    sd_ = model.state_dict()
    assert torch.equal(sd_['vq_ema_n'], model.vq_ema_n) and torch.equal(sd_['vq_ema_m'], model.vq_ema_m)


# ------------------------------------------------------------------ 5: off is off
def test_off_is_off(pkg):
    m, w, B, T = reproducible_cfg()
    P = M.init_params(m, w, 10, seed=21, randomize_all=True)
    batches = _batches(2, B, T, 10, 1234)
    absent, zero = build(pkg, m, w, 10, P), build(pkg, dict(m, codebook_ema=0, codebook_restart=0), w, 10, P)
    assert 'codebook_ema' not in m and absent.codebook_ema == 0.0 and zero.codebook_ema == 0.0 and zero.codebook_restart == 0.0
    for model in (absent, zero):
        for xd, sd in batches:
            ws = model.train_step(xd, sd)
        model.finish_steps()
        assert model.global_step == 2
        assert not any(k.startswith('cb_') for ws_ in model._ws.values() for k in ws_)
        assert not any(k.startswith('vq_ema') or k.startswith('codebook') for k in model.state_dict())
        assert model.vq_ema_n is None and model.vq_ema_m is None and model.codebook_info() == {'used': 0, 'restarted': 0}
        assert sorted(absent._ws[(B, T, True)]) == sorted(ws)
    for k in STATE:
        assert torch.equal(bits(getattr(absent, k)), bits(getattr(zero, k))), k
    o, shp = absent.seg_off['embedding']
    assert float(absent.adam_v[o:o + absent.Kc * absent.D].abs().max()) > 0        # (Adam does train the codebook here)


# ------------------------------------------------------------------ 6: only train_step updates
def test_only_train_step_updates(pkg):
    """The tiny configuration with the Magenta encoder (two forward passes of Encoder_64 are not bit-equal, see
    test_only_train_step_jitters)."""
    m, w = tiny_cfg()
    m = dict(m, encoder='Magenta')
    P = M.init_params(m, w, 10, seed=21, randomize_all=True)
    (xd, sd), = _batches(1, 2, 512, 10, 1234)
    plain, on = build(pkg, m, w, 10, P), build(pkg, dict(m, codebook_ema=0.9, codebook_restart=0.999), w, 10, P)

    def calls_agree(weights):
        state = [None if t is None else t.clone() for t in (on.vq_ema_n, on.vq_ema_m, on.P['embedding'])]
        a, b = plain.forward(xd, sd, compute_grad_seed=False), on.forward(xd, sd, compute_grad_seed=False)
        assert not b['cb_stats']
        for k in ('cond', 'logits', 'idx'):
            assert torch.equal(a[k], b[k]), k
        sa, sb = plain.evaluate(xd, sd, weights=weights), on.evaluate(xd, sd, weights=weights)
        assert torch.equal(sa.nll_sum, sb.nll_sum) and torch.equal(sa.entropy_sum, sb.entropy_sum) and torch.equal(sa.codes, sb.codes)
        assert torch.equal(plain.encode(xd, sd), on.encode(xd, sd))
        assert torch.equal(plain.encode_codes(xd, sd), on.encode_codes(xd, sd))
        for was, t in zip(state, (on.vq_ema_n, on.vq_ema_m, on.P['embedding'])):
            assert (was is None and t is None) or torch.equal(bits(was), bits(t))
    calls_agree('ema')
    assert on.vq_ema_n is None and not any(k.startswith('cb_') and k != 'cb_stats' for ws in on._ws.values() for k in ws)
    E0 = on.P['embedding'].clone()
    ws = on.train_step(xd, sd)
    assert ws['cb_stats'] and on.vq_ema_n is not None and not torch.equal(on.P['embedding'], E0)
    plain.load_named(on.named_parameters())              # the same live parameters again, codebook included
    calls_agree('live')


# ------------------------------------------------------------------ 7: one update per applied step under the range guard
@pytest.mark.parametrize('defer', [False, True], ids=['immediate', 'deferred'])
def test_one_update_per_applied_step_under_the_guard(pkg, monkeypatch, defer):
    """_guarded_model's shape (reference widths, B = 1, T = 1024: 16 frames, K = 512), decay 0.9, no restarts, three steps, the
    second flagged as test_deferred_guard_matches_immediate flags one.  sum n = g^3 K + (1 - g^3) Nf = 377.6 after three updates;
    two or four would give 416.3 or 341.4."""
    m, w = dict(M.DEFAULT_MODEL, codebook_ema=0.9), dict(M.DEFAULT_WAVENET)
    P = M.init_params(m, w, 109, seed=3, randomize_all=True)
    batches = _batches(3, 1, 1024, 109, 4321)
    model = _guarded_model(pkg, monkeypatch, P, m, w)
    model.defer_guard = defer
    snap, checked = [], []
    if defer:
        resolve = model._resolve_oldest

        def checked_resolve():
            if len(model._pending) == 2 and snap and not checked:      # the flagged step and the speculative one are both enqueued
                torch.cuda.synchronize()
                for was, t in zip(snap, (model.vq_ema_n, model.vq_ema_m, model.P['embedding'])):
                    assert torch.equal(bits(was), bits(t)), 'a voided step wrote the codebook state'
                checked.append(True)
            resolve()
        model._resolve_oldest = checked_resolve
    for i, (xd, sd) in enumerate(batches):
        if i == 1:
            model.finish_steps()                         # step 1 is resolved
            snap = [t.clone() for t in (model.vq_ema_n, model.vq_ema_m, model.P['embedding'])]
            model.x3_scale[model.SL['X'] + 2] *= 2.0 ** 24
        model.train_step(xd, sd)
    model.finish_steps()
    assert model.global_step == 3 and model.x3_fallbacks == 1
    assert bool(checked) == defer
    g = 0.9
    want = g ** 3 * 512 + (1 - g ** 3) * 16
    got = float(model.vq_ema_n.double().sum())
    print('sum n %.4f, want %.4f' % (got, want))
    assert abs(got - want) <= 1e-4 * want


# ------------------------------------------------------------------ 8: deferred and immediate agree; the picks
def test_deferred_and_immediate_agree_bit_for_bit(pkg, monkeypatch):
    monkeypatch.setenv('VQW_ENGINE', 'f16x3')
    monkeypatch.delenv('VQW_GATE_F16X3', raising=False)
    m, w, B, T = reproducible_cfg()
    m = dict(m, codebook_ema=0.9, codebook_restart=0.999)
    P = M.init_params(m, w, 10, seed=21, randomize_all=True)
    batches = _batches(3, B, T, 10, 1234)
    runs = []
    for defer in (False, True):
        model = build(pkg, m, w, 10, P)
        assert model.x3_guard
        model.defer_guard = defer
        for xd, sd in batches:
            ws = model.train_step(xd, sd)
        model.finish_steps()
        assert model.global_step == 3 and ws['cb_stats']
        runs.append(model)
    a, b = runs
    for k in STATE + ('vq_ema_n', 'vq_ema_m'):
        assert torch.equal(bits(getattr(a, k)), bits(getattr(b, k))), k
    assert a.codebook_info() == b.codebook_info() and a.codebook_info()['restarted'] > 0


def test_uniforms_are_a_pure_function_of_seed_and_step(pkg):
    m, w = tiny_cfg()
    model = pkg.model.VQVAE(dict(m, codebook_ema=0.99, time_jitter=0.12), w, 10, device='cuda', seed=0)
    torch.cuda.manual_seed(1234)
    state, cpu_state = torch.cuda.get_rng_state(), torch.get_rng_state()
    a, b, c = model.codebook_uniforms(512, 5), model.codebook_uniforms(512, 5), model.codebook_uniforms(512, 6)
    model.codebook_seed = 1
    d = model.codebook_uniforms(512, 5)
    assert torch.equal(torch.cuda.get_rng_state(), state) and torch.equal(torch.get_rng_state(), cpu_state)
    assert a.dtype == torch.float32 and a.is_cuda and tuple(a.shape) == (512,)
    assert torch.equal(a, b) and not torch.equal(a, c) and not torch.equal(a, d)
    assert float(a.min()) >= 0.0 and float(a.max()) < 1.0
    assert not torch.equal(d, model.jitter_uniforms(1, 512, 5).view(-1))          # not the jitter's stream
    assert 'codebook_seed' not in model.state_dict()


# ------------------------------------------------------------------ 9: resume
def test_resume_continues_bit_for_bit(pkg):
    m, w, B, T = reproducible_cfg()
    on = dict(m, codebook_ema=0.9, codebook_restart=0.999)
    P = M.init_params(m, w, 10, seed=21, randomize_all=True)
    batches = _batches(3, B, T, 10, 1234)
    whole, first = build(pkg, on, w, 10, P), build(pkg, on, w, 10, P)
    for xd, sd in batches:
        whole.train_step(xd, sd)
    for xd, sd in batches[:2]:
        first.train_step(xd, sd)
    sd_ = {k: v.clone().cpu() for k, v in first.state_dict().items()}
    assert 'vq_ema_n' in sd_ and 'vq_ema_m' in sd_
    second = pkg.model.VQVAE(on, w, 10, device='cuda', seed=0)
    second.load_state_dict(sd_)
    second.train_step(*batches[2])
    assert second.global_step == whole.global_step == 3
    for k in STATE + ('vq_ema_n', 'vq_ema_m'):
        assert torch.equal(bits(getattr(whole, k)), bits(getattr(second, k))), k
    # a state trained the old way, continued with the feature on
    old = build(pkg, m, w, 10, P)
    for xd, sd in batches[:2]:
        old.train_step(xd, sd)
    sd_old = {k: v.clone().cpu() for k, v in old.state_dict().items()}
    assert 'vq_ema_n' not in sd_old
    o, shp = old.seg_off['embedding']
    emb = slice(o, o + old.Kc * old.D)
    assert float(sd_old['adam_v'][emb].abs().max()) > 0
    cont = pkg.model.VQVAE(on, w, 10, device='cuda', seed=0)
    cont.load_state_dict(sd_old)
    assert bool((cont.vq_ema_n == 1).all()) and torch.equal(bits(cont.vq_ema_m), bits(cont.P['embedding']))
    assert torch.equal(cont.P['embedding'].cpu(), sd_old['flat'][emb].view(old.Kc, old.D))
    assert int((cont.adam_m[emb] != 0).sum()) == 0 and int((cont.adam_v[emb] != 0).sum()) == 0
    rest = torch.ones(cont.n_flat, dtype=torch.bool)
    rest[emb] = False
    assert torch.equal(cont.adam_v.cpu()[rest], sd_old['adam_v'][rest])


# ------------------------------------------------------------------ 10: two data-parallel ranks
@pytest.mark.parametrize('tau', [0.999, 0.0], ids=['restart', 'no_restart'])
def test_two_ranks_apply_the_same_update(pkg, tmp_path, tau):
    run_ranks([os.path.join(ROOT, 'tests', 'codebook_dp_worker.py'), str(tmp_path), str(tau)], 2)
    r = [torch.load(str(tmp_path / ('rank%d.pt' % i)), weights_only=True) for i in range(2)]
    for k in ('embedding', 'vq_ema_n', 'vq_ema_m', 'embedding_1', 'cnt_1'):
        assert torch.equal(bits(r[0][k]), bits(r[1][k])), k
    Kc, Nf = r[0]['vq_ema_n'].numel(), int(r[0]['frames']) + int(r[1]['frames'])
    cnt = r[0]['cnt_1']
    assert int(cnt.sum()) == Nf and int(r[0]['frames']) == int(r[1]['frames'])
    if tau > 0:
        dead = (cnt == 0).nonzero().view(-1).tolist()
        assert len(dead) >= 2 and r[0]['info_1'].tolist() == [len(dead), Kc - len(dead)]
        for k in dead:                                   # the owning rank's frame, bit for bit
            z = r[k % 2]['z_e_1']
            frames = z.permute(0, 2, 1).reshape(-1, z.shape[1])
            assert bool((bits(frames) == bits(r[0]['embedding_1'][k])[None, :]).all(1).any()), k
        assert {k % 2 for k in dead} == {0, 1}
    else:
        g = 0.9
        want = g ** 2 * Kc + (1 - g ** 2) * Nf
        assert abs(float(r[0]['vq_ema_n'].double().sum()) - want) <= 1e-5 * want
        assert r[0]['info_1'].tolist() == [0, int((cnt > 0).sum())]


# ------------------------------------------------------------------ 11: command line
def test_train_cli_logs_the_codebook(tmp_path):
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
                          str(tmp_path / 'm.json'), '-codebook_ema', '0.99', '-codebook_restart', '0.05'], cwd=str(tmp_path),
                         env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert '[codebook used' in out.stdout
    lines = [json.loads(ln) for ln in (tmp_path / 'saved_model' / 'summaries.jsonl').read_text().splitlines()]
    assert [ln['global_step'] for ln in lines] == [1, 2]
    for ln in lines:
        assert 0 < ln['codebook_used'] <= 32 and 0 <= ln['codebook_restarted'] <= 32
    sd = torch.load(str(tmp_path / 'saved_model' / 'weights-2.pt'), map_location='cpu', weights_only=True)
    assert tuple(sd['vq_ema_n'].shape) == (32,) and tuple(sd['vq_ema_m'].shape) == (32, 16)
