"""GPU tests of both stepping generators past ring wrap, on every instantiation pick_kernel (csrc/ar_persist.hip) dispatches
and on the launch-per-phase path (csrc/ar_decode.hip), against the float64 PARALLEL references of gen_ref.py (the training
graph teacher-forced on what the generator produced; no queue logic in common with the kernels).

Every case: dilations [1..512] * 2 and n = 2112 steps, more than two depths of the deepest ring ((ks-1) 512 + 1 slots), so
every tap of every layer is live and every ring has wrapped; mode 'sample' with supplied uniforms, so the history is varied
(each row must show at least 100 distinct indices: a constant history hides a shifted tap).

  1. ONE generate call (a single persistent launch over all n steps: the history role's prefetch crosses every step):
     audio is mu_law_decode(idx); every index is searchsorted(cumsum(p64), u), excused only where u sits within 2e-6 of a
     cdf edge, and at most 0.2 % of the steps may need that excuse.
  2. reset, then the same run in chunks ending at gen_ref.checkpoints (around the steps where the deepest layer's taps go
     live and its ring wraps): the indices equal the single run's bit for bit, and the distribution of each chunk's last
     step is the reference's (rtol 2e-4, atol 1e-7: the bars of test_fast_generation_reference_width).
  3. The back end that ran is asserted: R / cpb workgroups per persistent handle, 0 on the launch-per-phase path.

Each case prints its wall time, its excused steps and its largest relative probability error (python -m pytest -s)."""
import json
import os
import sys
import time

import numpy as np
import pytest
import torch

from oracle import ref_model as M

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_ref as G  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIL = [2 ** i for i in range(10)] * 2
N = 2112                      # 33 condition frames; > 2 * 1025
MAX_EXCUSED = 0.002           # of B * N
ENV = ('VQW_AR_PERSISTENT', 'VQW_AR_CPB', 'VQW_AR_ROWS', 'VQW_AR_PLACE')

# (RL, nS, ks, cpb) of pick_kernel -> R, S, ks, VQW_AR_CPB, rows in one handle
PERSISTENT = [
    ((1, 2, 3, 8), 32, 64, 3, 8, 2),
    ((1, 2, 2, 8), 32, 64, 2, 8, 2),
    ((1, 2, 3, 4), 64, 128, 3, 4, 2),
    ((2, 2, 3, 8), 64, 128, 3, 8, 2),
    ((2, 2, 3, 4), 128, 256, 3, 4, 2),
    ((4, 2, 3, 8), 128, 256, 3, 8, 2),
    ((4, 4, 3, 8), 128, 512, 3, 8, 2),
    ((8, 1, 3, 8), 256, 256, 3, 8, 1),
    ((4, 2, 3, 4), 256, 512, 3, 4, 1),
    ((8, 2, 3, 8), 256, 512, 3, 8, 1),
    ((4, 2, 2, 4), 256, 512, 2, 4, 1),
    ((8, 2, 2, 8), 256, 512, 2, 8, 1),
]
PHASED = [(32, 64, 3, 2), (32, 64, 2, 2), (256, 512, 3, 1)]        # R, S, ks, B


def configs(R, S, ks):
    m, w = G.tiny_cfg()                  # encoder 48 filters, latent 16, speaker embedding 16
    w.update(dilation_rates=list(DIL), num_cycles=2, num_cycle_layers=10, kernel_size=ks, dilation_filters=R,
             residual_filters=R, skip_filters=S, preprocess={"kernel_size": 32, "filters": R})
    return m, w


@pytest.fixture(scope='module')
def decoders(pkg):
    """One model per decoder shape, shared by the cases that run it on different back ends and layouts."""
    made = {}

    def get(R, S, ks):
        if (R, S, ks) not in made:
            m, w = configs(R, S, ks)
            P = M.init_params(m, w, 10, seed=100 + R + S + ks, randomize_all=True)
            model = pkg.model.VQVAE(m, w, 10, device='cuda', seed=0)
            model.load_named(P)
            made[(R, S, ks)] = (model, P, w)
        return made[(R, S, ks)]
    yield get
    made.clear()
    torch.cuda.empty_cache()


@pytest.fixture(scope='module')
def refs():
    """Float64 passes already made, by what they were made of: back ends that produce the same sequence share one."""
    return {}


def set_env(monkeypatch, persistent='1', cpb=None, rows=None):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('VQW_AR_PERSISTENT', persistent)
    if cpb:
        monkeypatch.setenv('VQW_AR_CPB', str(cpb))
    if rows:
        monkeypatch.setenv('VQW_AR_ROWS', str(rows))


def assert_backend(pkg, gen, parts, nwg):
    assert gen._parts == parts
    got = [pkg._lib.lib().vqw_ar_decode_workgroups(h) for h in gen._hs]
    assert got == [nwg] * len(parts), 'workgroups per handle %s, expected %d: another back end or variant ran' % (got, nwg)


def rel_err(p, p64):
    """Largest |p - p64| / p64 over the classes the atol of the comparison does not already cover."""
    big = p64 >= 1e-6
    return float((np.abs(p - p64)[big] / p64[big]).max())


def report(name, wall, excused, steps, err):
    print('\n[long-run] %-28s single run %.2f s, chunked %.2f s, float64 pass %.2f s; excused %d of %d; max rel. prob. error '
          'at the checkpoints %.2e' % (name, wall[0], wall[1], wall[2], excused, steps, err))


def run_decoder_case(pkg, decoders, refs, name, R, S, ks, B, parts, nwg):
    model, P, w = decoders(R, S, ks)
    g = torch.Generator().manual_seed(7 * R + ks + B)
    enc = 0.5 * torch.randn(B, model.Cc, N // 64, generator=g)               # [B][Cc][Tz]: no encoder run needed
    u = torch.rand(B, N, generator=g)
    enc_d, u_d = enc.cuda(), u.cuda()
    gen = pkg.generator.FastGenerator(model, batch=B)
    try:
        assert_backend(pkg, gen, parts, nwg)
        # 1. one run over all steps
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        audio, idx = gen.generate(enc_d, N, mode='sample', uniforms=u_d)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        idx_h, audio_h = idx.cpu().numpy(), audio.cpu().numpy()
        np.testing.assert_allclose(audio_h, M.R.mu_law_decode_np(idx_h.astype(np.float32)), rtol=1e-5, atol=1e-6)
        distinct = [len(np.unique(r)) for r in idx_h]
        assert min(distinct) >= 100, 'degenerate history: %s distinct indices per row' % distinct
        key = (R, S, ks, B, idx_h.tobytes())
        if key not in refs:
            refs[key] = G.decoder_probs64(P, w, audio_h, enc.permute(0, 2, 1), idx=idx_h)
        p64 = refs[key]
        t2 = time.perf_counter()
        depths = G.ring_depths(ks, DIL, persistent=nwg > 0)
        excused = G.check_sampled(p64, u, idx_h, depths)
        assert excused <= MAX_EXCUSED * B * N, '%d of %d steps needed the cdf-edge excuse' % (excused, B * N)
        # 2. the same run in chunks around the steps where taps go live and rings wrap
        gen.reset()
        t3 = time.perf_counter()
        parts_idx, err, prev = [], 0.0, 0
        for t in G.checkpoints(N, ks, 512):
            a_c, i_c, p_c = gen.generate(enc_d, t - prev, mode='sample', uniforms=u_d[:, prev:t].contiguous(), return_probs=True)
            parts_idx.append(i_c)
            got = p_c.cpu().numpy()
            err = max(err, rel_err(got, p64[:, t - 1]))
            np.testing.assert_allclose(got, p64[:, t - 1], rtol=2e-4, atol=1e-7, err_msg='distribution of step %d' % (t - 1))
            prev = t
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        assert prev == N and torch.equal(torch.cat(parts_idx, 1), idx), 'continuing a run differs from one long run'
        # 3. still the back end asked for
        assert_backend(pkg, gen, parts, nwg)
    finally:
        gen.close()
    report(name, (t1 - t0, t4 - t3, t2 - t1), excused, B * N, err)


# ------------------------------------------------------------------ the persistent kernel, one case per instantiation
@pytest.mark.parametrize('variant, R, S, ks, cpb, rows', PERSISTENT,
                         ids=['RL%d-nS%d-ks%d-cpb%d-rows%d' % (v + (r,)) for v, _, _, _, _, r in PERSISTENT])
def test_persistent_variant_past_ring_wrap(pkg, decoders, refs, monkeypatch, variant, R, S, ks, cpb, rows):
    assert variant == (R * cpb // 256, S // R, ks, cpb)
    set_env(monkeypatch, '1', cpb, rows if rows > 1 else None)
    run_decoder_case(pkg, decoders, refs, 'persistent %s B=%d' % (variant, rows), R, S, ks, rows, [rows], R // cpb)


def test_persistent_three_one_row_handles_in_one_launch(pkg, decoders, refs, monkeypatch):
    set_env(monkeypatch, '1')
    run_decoder_case(pkg, decoders, refs, 'persistent 3 x one row', 32, 64, 3, 3, [1, 1, 1], 32 // 8)


# ------------------------------------------------------------------ the launch-per-phase path
@pytest.mark.parametrize('R, S, ks, B', PHASED, ids=['R%d-S%d-ks%d-B%d' % c for c in PHASED])
def test_launch_per_phase_past_ring_wrap(pkg, decoders, refs, monkeypatch, R, S, ks, B):
    set_env(monkeypatch, '0', None, B if B > 1 else None)
    run_decoder_case(pkg, decoders, refs, 'launch-per-phase R%d ks%d B=%d' % (R, ks, B), R, S, ks, B, [B], 0)


# ------------------------------------------------------------------ the prior (code-input mode, persistent only)
def run_prior_case(pkg, name, cfg, B, parts, nwg, min_distinct):
    pt = G.prior_tests()
    k = cfg['quantization_channels']
    prior = pkg.prior.LatentPrior(cfg, 10, device='cuda', seed=0)
    P = pt.random_params(prior, 11)
    prior.load_named(P)
    spk = torch.tensor([2, 9][:B])                                        # distinct speakers: the only condition
    sd = spk.cuda()
    u = torch.rand(B, N, generator=torch.Generator().manual_seed(k + B))
    u_d = u.cuda()
    gen = pkg.generator.PriorGenerator(prior, batch=B)
    try:
        assert_backend(pkg, gen, parts, nwg)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        codes = gen.sample(N, sd, mode='sample', uniforms=u_d)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        codes_h = codes.cpu().numpy()
        assert codes_h.min() >= 0 and codes_h.max() < k
        distinct = [len(np.unique(r)) for r in codes_h]
        assert min(distinct) >= min_distinct, 'degenerate history: %s distinct codes per row' % distinct
        p64 = G.prior_probs64(P, cfg, codes_h, spk)
        t2 = time.perf_counter()
        depths = G.ring_depths(cfg['kernel_size'], DIL)
        excused = G.check_sampled(p64, u, codes_h, depths)
        assert excused <= MAX_EXCUSED * B * N, '%d of %d steps needed the cdf-edge excuse' % (excused, B * N)
        gen.reset()
        t3 = time.perf_counter()
        chunks, err, prev = [], 0.0, 0
        for t in G.checkpoints(N, cfg['kernel_size'], 512):
            c, p_c = gen.sample(t - prev, sd, mode='sample', uniforms=u_d[:, prev:t].contiguous(), return_probs=True)
            chunks.append(c)
            got = p_c.cpu().numpy()
            err = max(err, rel_err(got, p64[:, t - 1]))
            np.testing.assert_allclose(got, p64[:, t - 1], rtol=2e-4, atol=1e-7, err_msg='distribution of step %d' % (t - 1))
            prev = t
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        assert prev == N and torch.equal(torch.cat(chunks, 1), codes), 'continuing a run differs from one long run'
        assert_backend(pkg, gen, parts, nwg)
    finally:
        gen.close()
    report(name, (t1 - t0, t4 - t3, t2 - t1), excused, B * N, err)


@pytest.mark.parametrize('pre_k, rows', [(3, 2), (1, None)], ids=['pre_k3-one-handle-of-2-rows', 'pre_k1-two-one-row-handles'])
def test_prior_past_ring_wrap(pkg, monkeypatch, pre_k, rows):
    """32 codes cannot show 100 distinct indices: at least half of the codebook in every row instead."""
    set_env(monkeypatch, '1', None, rows)
    cfg = G.prior_tests().tiny_prior(k=32, pre_k=pre_k)
    cfg.update(dilation_rates=list(DIL), num_cycles=2, num_cycle_layers=10)
    run_prior_case(pkg, 'prior k32 pre_k%d' % pre_k, cfg, 2, [2] if rows else [1, 1], 32 // 8, 16)


def test_prior_default_widths_past_ring_wrap(pkg, monkeypatch):
    """prior_parameters.json (R 256, S 512, k 512, the dilations of this file's recipe), one row: the library's own choice
    of 4 channels per workgroup on a chip with at least R / 4 CUs."""
    set_env(monkeypatch, '1')
    with open(os.path.join(ROOT, 'prior_parameters.json')) as f:
        cfg = json.load(f)
    assert cfg['dilation_rates'] == DIL and cfg['kernel_size'] == 3
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    cpb = 4 if cfg['residual_filters'] // 4 <= cus else 8
    run_prior_case(pkg, 'prior default widths', cfg, 1, [1], cfg['residual_filters'] // cpb, 100)
