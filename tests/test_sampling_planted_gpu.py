"""GPU tests of truncated sampling (csrc/ar_sampling.h, ar_sample_truncated) on the planted logits of sampling_cases.py, in
every kernel that inlines it.  Ties at the cuts are the subject here: test_sampling_gpu.py and test_recon_gpu.py feed
continuous logits and excuse them (sampling_ref.fp32_edge).  NOTHING is excused here: every case is clean by construction
(sampling_ref.planted_faults == [], asserted), so every index is the float64 restatement's, every class outside the kept set
has probability 0.0 bit for bit, and kept classes of one level -- the same pure function of the same input -- hold
bit-equal q.

A. the all-positions kernel (sample.hip, K.softmax_sample): logits [B][Q][T], row b under setting b of the staircase, position
   t with its own shuffle and its own u; T = 101 is a multiple of no tile width (NT = 64, 32, 16, 8), so the partial last tile
   runs.  probs on the kept classes within 1e-6 of the restated q, rows summing to 1 within 1e-5 (the bars of
   test_recon_gpu.py); the worst error is recorded as `worst_probs_err`.
B. the generators read their logits from the network, so the staircase is planted through the weights: postprocess2/kernel
   all zero and postprocess2/bias the staircase make every step's logits the bias whatever the rest of the random stack
   computes.  That premise is asserted first on every back end (a default row's probs_last is float64 softmax(bias) at
   rtol 2e-4, atol 1e-7, bit-equal between a 1-step run and the last step of a longer one); then every step of mixed
   per-row settings must give the restated index, and greedy the lowest index of the top plateau."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampling_cases as C  # noqa: E402
import sampling_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu
T_A = 101


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def kw_of(rows):
    t, k, p = zip(*rows)
    return dict(temperature=list(t), top_k=list(k), top_p=list(p))


@functools.lru_cache(maxsize=None)
def planted(Q, index):
    """The float64 restatement of one staircase under all its settings: computed once, shared, never written to."""
    st = C.staircase(Q, index)
    return C.plant(st, C.settings(st), T_A)


def bits(x):
    return x.contiguous().view(torch.int32).cpu().numpy()


def check_probs(got, z, keep, q, where):
    """got fp32 [...][Q] against the restated keep / q (same shape), z the logits [...][Q]: exact zeros off the kept set, the
    bars of test_recon_gpu.py on it, bit-equal q within a level.  Returns the worst error."""
    gb = got.view(np.int32)
    assert (gb[~keep] == 0).all(), '%s: %d unkept classes are not 0.0 bit for bit' % (where, (gb[~keep] != 0).sum())
    g64 = got.astype(np.float64)
    err = np.abs(g64 - q)[keep].max()
    assert err <= 1e-6, '%s: probs error %.3g' % (where, err)
    assert np.abs(g64.sum(-1) - 1).max() <= 1e-5, where
    for v in np.unique(z):
        m = keep & (z == v)
        hi, lo = np.where(m, gb, -1).max(-1), np.where(m, gb, np.iinfo(np.int32).max).min(-1)
        assert ((hi == lo) | ~m.any(-1)).all(), '%s: kept classes of level %g differ in their bits' % (where, v)
    return err


def run_a(K, Q, pl, rows=None, t_begin=None, t_end=None):
    """One launch of the all-positions kernel over rows (default: all) of the planted tensor pl, fully checked."""
    rows = list(range(len(pl.rows))) if rows is None else rows
    B, T = len(rows), pl.z.shape[2]
    assert pl.faults == []                                    # the condition of this file: no position is left out
    z, u = pl.z[rows], pl.u[rows]
    levels = Q if Q in (256, 512, 1024) else None
    probs = torch.full((B, T, Q), float('nan'), device='cuda')
    audio = torch.full((B, T), float('nan'), device='cuda') if levels else None
    idx = K.softmax_sample(dev(z), mode='sample', uniforms=dev(u), audio=audio, probs=probs, t_begin=dev(t_begin), t_end=dev(t_end),
                           levels=levels or 256, **kw_of([pl.rows[b] for b in rows]))
    got, pr = idx.cpu().numpy(), probs.cpu().numpy()
    mask = np.ones((B, T), bool)
    if t_begin is not None:
        mask = (np.arange(T)[None] >= t_begin[:, None]) & (np.arange(T)[None] < t_end[:, None])
        assert mask.any() and not mask.all()
    want = np.where(mask, pl.idx[rows], -1)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, 'Q %d: %d of %d positions differ; first (row, position): %s settings %s u %r: GPU %d, restated %d' % (
        Q, len(bad), mask.sum(), bad[0], pl.rows[rows[bad[0][0]]], float(u[tuple(bad[0])]), got[tuple(bad[0])], want[tuple(bad[0])])
    assert (pr.view(np.int32)[~mask] == 0).all()
    err = check_probs(pr[mask], z.transpose(0, 2, 1)[mask], pl.keep[rows][mask], pl.q[rows][mask], 'Q %d' % Q)
    if levels:
        dec = K.mu_law_decode_f32(idx.clamp(min=0).float(), levels=levels)
        dec = torch.where(idx >= 0, dec, torch.zeros_like(dec))
        assert np.array_equal(bits(audio), bits(dec))
    return err


# ------------------------------------------------------------------ A. the all-positions kernel
@pytest.mark.parametrize('index', range(C.N_STAIRCASES))
@pytest.mark.parametrize('Q', C.QS)
def test_all_positions(K, record_property, Q, index):
    pl = planted(Q, index)
    err = run_a(K, Q, pl)
    print('Q %d staircase %d %s: %d rows x %d positions, worst probs error %.3g' % (Q, index, C.staircase(Q, index).counts,
                                                                                   len(pl.rows), T_A, err))
    record_property('worst_probs_err', float(err))


def test_all_positions_with_ranges(K, record_property):
    """Q = 1020 (the last lane partial at nj = 16, tiles of 16 positions): ranges that begin and end inside a tile, an empty
    one, one that is a prefix; the same tensor as the unranged run of test_all_positions."""
    pl = planted(1020, 2)
    pats = [(T_A // 3, T_A - 5), (10, 10), (0, T_A // 2 + 1), (0, T_A), (17, 18)]
    tb, te = (np.array(a, np.int32) for a in zip(*[pats[b % 5] for b in range(len(pl.rows))]))
    record_property('worst_probs_err', float(run_a(K, 1020, pl, t_begin=tb, t_end=te)))


def test_35_rows_cross_the_row_group(K, record_property):
    """B = 35 at Q = 64, every row another setting: rows 32..34 go out in the second launch, whose settings are read from
    the second group (a row reading rows.r[b % 32] of the FIRST group would sample under row b - 32's settings)."""
    pl = planted(64, 1)
    untruncated = [b for b, r in enumerate(pl.rows) if r[1:] == (0, 1.0)]       # rows 0..2: one per temperature
    argmax = [b for b, r in enumerate(pl.rows) if r[1:] == (1, 1.0)]            # rows 32..34: top_k = 1
    others = [b for b in range(len(pl.rows)) if b not in untruncated + argmax]
    rows = untruncated + [others[int(i)] for i in np.linspace(0, len(others) - 1, 29).round()] + argmax
    assert len(rows) == 35 and len({pl.rows[b] for b in rows}) == 35
    for b in (32, 33, 34):                                    # ... and that would show: the restated indices differ
        assert (pl.idx[rows[b]] != pl.idx[rows[b - 32]]).mean() > 0.5
    record_property('worst_probs_err', float(run_a(K, 64, pl, rows=rows)))


# ------------------------------------------------------------------ B. the generators
N_B = 96                      # steps per run: two condition frames
DEFAULT = (1.0, 0, 1.0)
ENV = ('VQW_AR_PERSISTENT', 'VQW_AR_CPB', 'VQW_AR_ROWS', 'VQW_AR_PLACE')


def rows_for(st, count):
    """count truncated settings of the staircase, spread over all of them (temperatures, cuts and nucleus targets alike)."""
    pool = [r for r in C.settings(st) if r != DEFAULT]
    return [pool[int(i)] for i in np.linspace(0, len(pool) - 1, count).round()]


def plant_bias(model, P, scope, z):
    """Every variable as in P, but postprocess2's kernel zero and its bias z: the logits of every step are z."""
    P = dict(P)
    P[scope + '/postprocess2/kernel'] = torch.zeros_like(P[scope + '/postprocess2/kernel'])
    assert P[scope + '/postprocess2/bias'].shape == (len(z),)
    P[scope + '/postprocess2/bias'] = torch.from_numpy(z.copy())
    model.load_named(P)


def drive(gen, run, st, z, B, n_runs, decode=None):
    """One generator whose logits are z at every step.  run(n, mode, uniforms [B][n] or None, rows or None) -> (idx, probs of
    the last step, audio or None) from reset.  The premise on default rows, n_runs launches of a default row 0 beside B - 1
    truncated rows, greedy."""
    Q = len(z)
    u0 = torch.rand(B, N_B, generator=torch.Generator().manual_seed(Q + st.index))
    _, p1, _ = run(1, 'sample', u0[:, :1].contiguous(), None)
    solo_i, solo_p, solo_a = run(N_B, 'sample', u0, None)
    assert np.array_equal(bits(p1), bits(solo_p)), 'the logits move with the history: not the bias alone'
    for b in range(B):
        np.testing.assert_allclose(solo_p[b].cpu().double().numpy(), S.softmax_t(z.astype(np.float64), 1.0), rtol=2e-4, atol=1e-7)
    picked = rows_for(st, n_runs * (B - 1))
    for r in range(n_runs):
        rows = [DEFAULT] + picked[r * (B - 1):(r + 1) * (B - 1)]
        u, want = u0.clone(), [None]
        for b in range(1, B):
            ub, wb, keep, q = C.steps(st, rows[b], N_B)
            assert S.planted_faults(z, *rows[b], ub) == []
            u[b] = torch.from_numpy(ub)
            want.append((wb, keep, q))
        idx, probs, audio = run(N_B, 'sample', u, rows)
        assert torch.equal(idx[0], solo_i[0]) and np.array_equal(bits(probs[0]), bits(solo_p[0]))
        got, pl = idx.cpu().numpy(), probs.cpu().numpy()
        for b in range(1, B):
            wb, keep, q = want[b]
            bad = np.nonzero(got[b] != wb)[0]
            assert len(bad) == 0, 'Q %d staircase %d settings %s: %d of %d steps differ; first: step %d, u %r: GPU %d, restated %d' % (
                Q, st.index, rows[b], len(bad), N_B, bad[0], float(u[b, bad[0]]), got[b, bad[0]], wb[bad[0]])
            assert (pl[b].view(np.int32)[~keep] == 0).all(), 'settings %s: probs_last is not 0.0 off the kept set' % (rows[b],)
            np.testing.assert_allclose(pl[b].astype(np.float64), q, rtol=2e-4, atol=1e-7)
        if audio is not None:
            assert torch.equal(audio[0], solo_a[0])
            np.testing.assert_allclose(audio.cpu().numpy(), decode(got), rtol=1e-5, atol=1e-6)
    gi, _, _ = run(N_B, 'greedy', None, None)
    top = int(np.argmax(z))                                   # the lowest index of the top level (a plateau but for staircase 0)
    assert (gi.cpu().numpy() == top).all(), 'greedy is not the lowest index %d of the top level' % top


def audio_runner(gen, model, B):
    enc = (0.5 * torch.randn(B, model.Cc, 2, generator=torch.Generator().manual_seed(3))).cuda()

    def run(n, mode, u, rows):
        gen.reset()
        kw = dict(kw_of(rows), uniforms=u.cuda()) if rows else ({} if u is None else dict(uniforms=u.cuda()))
        audio, idx, probs = gen.generate(enc, n, mode=mode, return_probs=True, **kw)
        return idx, probs, audio
    return run


def code_runner(gen, B):
    spk = torch.tensor([(3 * b + 1) % 10 for b in range(B)], dtype=torch.int64).cuda()

    def run(n, mode, u, rows):
        gen.reset()
        kw = dict(kw_of(rows), uniforms=u.cuda()) if rows else ({} if u is None else dict(uniforms=u.cuda()))
        idx, probs = gen.sample(n, spk, mode=mode, return_probs=True, **kw)
        return idx, probs, None
    return run


@pytest.fixture(scope='module')
def decoders(pkg):
    """Q -> (model, its random parameters): the tiny decoder of test_sampling_gpu.py at 256 levels, test_levels_gpu.py's at 1024."""
    from oracle import ref_model as M
    import gen_ref as G
    from test_levels_gpu import configs
    made = {}

    def get(Q):
        if Q not in made:
            m, w = G.tiny_cfg() if Q == 256 else configs(128, 256, Q)
            P = M.init_params(m, w, 10, seed=11, randomize_all=True)
            model = pkg.model.VQVAE(m, w, 10, device='cuda', seed=0)
            assert model.Q == Q and model.levels == Q
            made[Q] = (model, P)
        return made[Q]
    yield get
    made.clear()
    torch.cuda.empty_cache()


@pytest.fixture(scope='module')
def priors(pkg):
    import gen_ref as G
    T = G.prior_tests()
    made = {}

    def get(k):
        if k not in made:
            prior = pkg.prior.LatentPrior(T.tiny_prior(k=k, pre_k=3), 10, device='cuda', seed=0)
            made[k] = (prior, T.random_params(prior, 21))
        return made[k]
    yield get
    made.clear()
    torch.cuda.empty_cache()


def set_env(monkeypatch, persistent, rows):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    if persistent is not None:
        monkeypatch.setenv('VQW_AR_PERSISTENT', persistent)
    if rows:
        monkeypatch.setenv('VQW_AR_ROWS', rows)


def decoder_of(Q):
    import levels_ref as LR
    return lambda idx: LR.decode(idx, Q)


# (levels, VQW_AR_PERSISTENT, VQW_AR_ROWS): test_sampling_gpu.LAYOUTS at 256 levels; 1024 levels (nj = 16) on the persistent kernel
FAST = [(256, '1', None), (256, '1', '2'), (256, '0', '2'), (1024, '1', None)]


@pytest.mark.parametrize('index', range(C.N_STAIRCASES))
@pytest.mark.parametrize('Q, persistent, rows', FAST)
def test_fast_generator(pkg, decoders, monkeypatch, Q, persistent, rows, index):
    set_env(monkeypatch, persistent, rows)
    model, P = decoders(Q)
    st = C.staircase(Q, index)
    z = C.logits(st)
    plant_bias(model, P, 'decoder', z)
    gen = pkg.generator.FastGenerator(model, batch=2)
    try:
        assert gen._parts == ([2] if rows else [1, 1])
        nwg = [pkg._lib.lib().vqw_ar_decode_workgroups(h) for h in gen._hs]
        assert all((v > 0) == (persistent == '1') for v in nwg), 'workgroups per handle %s: another back end ran' % nwg
        drive(gen, audio_runner(gen, model, 2), st, z, 2, 6, decoder_of(Q))
    finally:
        gen.close()


@pytest.mark.parametrize('index', range(C.N_STAIRCASES))
@pytest.mark.parametrize('Q', [256, 1024])
def test_wide_generator(pkg, decoders, monkeypatch, Q, index):
    set_env(monkeypatch, None, None)
    model, P = decoders(Q)
    st = C.staircase(Q, index)
    z = C.logits(st)
    plant_bias(model, P, 'decoder', z)
    gen = pkg.generator.WideGenerator(model, batch=5)
    try:
        drive(gen, audio_runner(gen, model, 5), st, z, 5, 3, decoder_of(Q))
    finally:
        gen.close()


@pytest.mark.parametrize('index', range(C.N_STAIRCASES))
@pytest.mark.parametrize('rows', [None, '2'])
def test_prior_generator(pkg, priors, monkeypatch, rows, index):
    """32 codes: nj = 1, lanes 32 to 63 hold no class."""
    set_env(monkeypatch, None, rows)
    prior, P = priors(32)
    st = C.staircase(32, index)
    z = C.logits(st)
    plant_bias(prior, P, 'prior', z)
    gen = pkg.generator.PriorGenerator(prior, batch=2)
    try:
        assert gen._parts == ([2] if rows else [1, 1])
        drive(gen, code_runner(gen, 2), st, z, 2, 6)
    finally:
        gen.close()


@pytest.mark.parametrize('index', range(C.N_STAIRCASES))
@pytest.mark.parametrize('k', C.CODE_QS)
def test_wide_prior_generator(pkg, priors, monkeypatch, k, index):
    """k = 32 (lanes 32 to 63 empty) and k = 96: vqw_ar_wide_prior_create takes multiples of 32 in 32..1024 (wide_create in
    csrc/ar_wide.hip), so 96 is the smallest k above 64 that is no multiple of 64: nj = 2, lanes 48 to 63 empty."""
    set_env(monkeypatch, None, None)
    prior, P = priors(k)
    st = C.staircase(k, index)
    z = C.logits(st)
    plant_bias(prior, P, 'prior', z)
    gen = pkg.generator.WidePriorGenerator(prior, batch=5)
    try:
        drive(gen, code_runner(gen, 5), st, z, 5, 3)
    finally:
        gen.close()
