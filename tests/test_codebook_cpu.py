"""CPU tests of the codebook by moving averages: the properties of the numpy restatement the GPU tests compare
against (codebook_ref.py), the constants, the configuration keys, the command-line checks of train.py and the wrappers'
refusal of CPU tensors."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import codebook_ref as CR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def problem(B, D, Tz, K, seed):
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((B, D, Tz)).astype(f32)
    idx = rng.integers(0, K, (B, Tz))
    E, m = rng.standard_normal((K, D)).astype(f32), rng.standard_normal((K, D)).astype(f32)
    n = (rng.random(K) * 3).astype(f32)
    return z, idx, E, n, m


@pytest.mark.parametrize('B,D,Tz,K', [(1, 4, 1, 3), (2, 8, 65, 70), (3, 16, 40, 7)])
def test_restatement_against_float64_closed_form(B, D, Tz, K):
    z, idx, E, n, m = problem(B, D, Tz, K, seed=B + Tz)
    pick = CR.picks(np.random.default_rng(1).random(K, dtype=f32), B * Tz)
    cnt, tot, cand = CR.stats(z, idx, K, pick)
    zf = z.transpose(0, 2, 1).reshape(B * Tz, D).astype(np.float64)
    flat = idx.reshape(-1)
    want_cnt = np.bincount(flat, minlength=K)
    want_sum = np.zeros((K, D))
    np.add.at(want_sum, flat, zf)
    assert cnt.dtype == np.int32 and tot.dtype == f32 and cand.dtype == f32
    assert (cnt == want_cnt).all() and cnt.sum() == B * Tz
    np.testing.assert_allclose(tot, want_sum, rtol=1e-6, atol=1e-6 * np.abs(zf).max() * max(1, want_cnt.max()) ** 0.5)
    assert (pick >= 0).all() and (pick < B * Tz).all() and np.array_equal(cand, zf[pick].astype(f32))
    E1, n1, m1, info = CR.update(E, n, m, cnt, tot, None, 0.9)
    g, h = 0.9, 1.0 - 0.9
    np.testing.assert_allclose(n1, g * n.astype(np.float64) + h * want_cnt, rtol=1e-6)
    np.testing.assert_allclose(m1, g * m.astype(np.float64) + h * want_sum, rtol=1e-6, atol=2e-6)
    used = want_cnt > 0
    want_E = (g * m.astype(np.float64) + h * want_sum) / (g * n.astype(np.float64) + h * want_cnt)[:, None]
    np.testing.assert_allclose(E1[used], want_E[used], rtol=1e-6, atol=2e-6 / float(n1[used].min()))
    assert info.tolist() == [0, int(used.sum())]


def test_picks_cover_both_ends_and_clamp():
    top = np.nextafter(f32(1), f32(0))
    assert CR.picks(np.array([0.0, 0.5, top], f32), 832).tolist() == [0, 416, 831]      # top * 832 rounds to 832.0 in fp32: clamped
    assert CR.picks(np.array([top], f32), 1).tolist() == [0]


def test_count_invariant_without_restarts():
    """sum n' = g sum n + h Nf up to rounding: every frame is counted once."""
    z, idx, E, n, m = problem(3, 8, 104, 50, seed=2)
    cnt, tot, _ = CR.stats(z, idx, 50)
    g, h, _ = CR.constants(0.99)
    _, n1, _, _ = CR.update(E, n, m, cnt, tot, None, 0.99)
    want = float(g) * float(n.astype(np.float64).sum()) + float(h) * 3 * 104
    assert abs(float(n1.astype(np.float64).sum()) - want) <= 1e-6 * want


def test_unused_codes_keep_their_bits_and_still_decay():
    z, idx, E, n, m = problem(2, 8, 10, 30, seed=3)
    idx[idx == 7] = 8
    E[7, 0], E[7, 1] = f32(-0.0), f32(1e-42)          # a signed zero and a denormal survive
    cnt, tot, _ = CR.stats(z, idx, 30)
    assert cnt[7] == 0 and (tot[7].view(np.int32) == 0).all()
    E1, n1, m1, _ = CR.update(E, n, m, cnt, tot, None, 0.9)
    assert np.array_equal(E1[7].view(np.int32), E[7].view(np.int32))
    assert n1[7] == f32(f32(0.9) * n[7]) + f32(0) and np.array_equal(m1[7], (f32(0.9) * m[7]).astype(f32) + f32(0))
    assert not np.array_equal(E1[8], E[8])


def boundary_state(tau, decay=0.5):
    """n for two unused codes whose n' = g n lands exactly on tau and on its fp32 neighbour below (decay 0.5: g n is exact)."""
    t = f32(tau)
    below = np.nextafter(t, f32(0))
    return np.array([t / f32(decay), below / f32(decay)], f32), t, below


def test_restart_happens_exactly_below_the_threshold():
    tau = 0.05
    n, t, below = boundary_state(tau)
    E = np.arange(8, dtype=f32).reshape(2, 4)
    m = E * 2
    cand = np.full((2, 4), 7.5, f32)
    cnt, tot = np.zeros(2, np.int32), np.zeros((2, 4), f32)
    E1, n1, m1, info = CR.update(E, n, m, cnt, tot, cand, 0.5, tau)
    assert info.tolist() == [1, 0]
    assert n1[0] == t and np.array_equal(E1[0], E[0]) and np.array_equal(m1[0], E[0])            # n' == tau: alive, decayed
    assert n1[1] == 1 and (E1[1] == 7.5).all() and (m1[1] == 7.5).all()                          # n' just below: restarted
    E2, n2, _, info2 = CR.update(E, n, m, cnt, tot, None, 0.5, 0.0)                              # tau = 0 never restarts
    assert info2.tolist() == [0, 0] and n2[1] == below and np.array_equal(E2, E)
    # a used code that is dead is restarted too (the restart wins over the average)
    E3, n3, m3, info3 = CR.update(E, n, m, np.array([0, 0], np.int32), tot, cand, 0.5, 0.9)
    assert info3.tolist() == [2, 0] and (E3 == 7.5).all() and (n3 == 1).all()


def test_constants(pkg):
    K = pkg.kernels
    for decay, restart in ((0.99, 0.0), (0.9, 0.05), (0.5, 0.999), (1e-3, 0.0)):
        g, h, tau = K.codebook_ema_constants(decay, restart)
        rg, rh, rt = CR.constants(decay, restart)
        assert (g, h, tau) == (float(rg), float(rh), float(rt))
    g, h, _ = K.codebook_ema_constants(0.99)
    assert g == float(f32(0.99)) and h == float(f32(0.01)) and h != float(f32(1) - f32(0.99))     # 1 - decay in float64, rounded once
    assert K.codebook_ema_constants(0, 0) == (0.0, 1.0, 0.0)
    for bad in ((1.0, 0), (-0.1, 0), (1.5, 0), (float('nan'), 0), (1.0 - 1e-12, 0), (1e-60, 0)):
        with pytest.raises(ValueError, match='codebook_ema'):
            K.codebook_ema_constants(*bad)
    for bad in ((0.9, 1.0), (0.9, -0.1), (0.9, float('nan')), (0.9, 1.0 - 1e-12)):
        with pytest.raises(ValueError, match='codebook_restart'):
            K.codebook_ema_constants(*bad)
    with pytest.raises(ValueError, match='needs codebook_ema'):
        K.codebook_ema_constants(0, 0.05)


def test_config_keys(pkg):
    VQVAE = pkg.model.VQVAE
    probe = VQVAE.__new__(VQVAE)
    assert probe.codebook_ema == 0.0 and probe.codebook_restart == 0.0 and probe.codebook_seed == 0
    cfg = {'latent_dim': 16, 'k': 32, 'speaker_embedding': 16, 'beta': 0.25, 'encoder_filters': 48}
    probe._setup_front(cfg, 10)
    assert probe.codebook_ema == 0.0 and probe.codebook_restart == 0.0
    probe._setup_front(dict(cfg, codebook_ema=0, codebook_restart=0), 10)
    assert probe.codebook_ema == 0.0
    probe._setup_front(dict(cfg, codebook_ema=0.99, codebook_restart=0.05), 10)
    assert probe.codebook_ema == 0.99 and probe.codebook_restart == 0.05
    probe.codebook_restart = 0.0
    probe.codebook_ema = 0.9
    assert (probe.codebook_ema, probe.codebook_restart) == (0.9, 0.0)
    with pytest.raises(ValueError, match='codebook_restart'):
        probe.codebook_restart = 1.0
    probe.codebook_restart = 0.1
    with pytest.raises(ValueError, match='needs codebook_ema'):
        probe.codebook_ema = 0.0
    assert (probe.codebook_ema, probe.codebook_restart) == (0.9, 0.1)
    for bad in (dict(codebook_ema=1.0), dict(codebook_ema=-0.5), dict(codebook_ema=float('nan')), dict(codebook_restart=0.05),
                dict(codebook_ema=0.9, codebook_restart=1.0), dict(codebook_ema=0.9, codebook_restart=-1)):
        with pytest.raises(ValueError, match='codebook_'):
            VQVAE.__new__(VQVAE)._setup_front(dict(cfg, **bad), 10)
    with pytest.raises(ValueError, match='use_vq'):
        VQVAE.__new__(VQVAE)._setup_front(dict(cfg, use_vq=False, codebook_ema=0.99), 10)
    VQVAE.__new__(VQVAE)._setup_front(dict(cfg, use_vq=False, codebook_ema=0), 10)
    P = pkg.prior.LatentPrior
    with pytest.raises(ValueError, match='codebook'):
        P.__new__(P)._setup_front({'quantization_channels': 32, 'speaker_embedding': 16, 'codebook_ema': 0.99}, 10)


@pytest.mark.parametrize('flags,msg', [(['-codebook_ema', '1.0'], '-codebook_ema must be'), (['-codebook_ema', '-0.1'], '-codebook_ema must be'),
                                       (['-codebook_ema', '0.9', '-codebook_restart', '1.5'], '-codebook_restart must be'),
                                       (['-codebook_ema', '0', '-codebook_restart', '0.05'], '-codebook_restart needs -codebook_ema')])
def test_bad_flags_exit_before_anything_is_loaded(tmp_path, flags, msg):
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'train.py')] + flags, cwd=str(tmp_path),
                         env=dict(os.environ, HIP_VISIBLE_DEVICES='', CUDA_VISIBLE_DEVICES=''), capture_output=True, text=True, timeout=120)
    assert out.returncode == 2, (out.returncode, out.stderr[-500:])
    assert msg in out.stderr


def test_wrappers_refuse_cpu_tensors(pkg):
    import torch
    K = pkg.kernels
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)  # noqa: E731
    with pytest.raises(ValueError, match='GPU'):
        K.vq_cluster_stats(torch.zeros(1, 2, 3), torch.zeros(1, 3, dtype=torch.int64), cnt=i32(4), sum=torch.zeros(4, 2),
                           pick=i32(4), cand=torch.zeros(4, 2), K=4)
    with pytest.raises(ValueError, match='GPU'):
        K.vq_codebook_ema_step(torch.zeros(4, 2), torch.zeros(4), torch.zeros(4, 2), cnt=i32(4), sum=torch.zeros(4, 2),
                               decay=0.9, info=i32(8))
