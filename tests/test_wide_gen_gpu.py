"""GPU tests of the wide generator (generator.WideGenerator, csrc/ar_wide.hip) against the float64 PARALLEL reference of
gen_ref.py: the training graph teacher-forced on what the generator produced, nothing in common with ring or window logic.

The contract pinned here:
  (a) every index is searchsorted(cumsum(p64), u), excused only where u lies within gen_ref.EDGE of a cdf value, at most
      0.2 % of the steps; probs_last at a chunk end is p64 within rtol 2e-4, atol 1e-7 (the bars test_generation_long_gpu.py
      holds the other fp32 generators to);
  (b) a row's indices, audio and probs_last are bit for bit independent of the batch: of B, of the row's position, of the
      other rows' inputs and sampling settings;
  (c) a run cut into chunks equals the single run bit for bit, also with chunk ends inside a condition frame and across a
      refresh of the condition window (4 frames);
  (d) audio is mu_law_decode(indices); greedy is the lowest index among the maxima;
  (e) a truncated row follows tests/sampling_ref.py on the reference's logits at the bars of test_sampling_gpu.py, and a
      default row beside truncated rows equals the same row of an all-default launch bit for bit.

Tiny width: R 32, S 64, Q 256, Cc 32, pre_k 32, dilations [1,2,4,8,16] * 2, ratio 16, n = 160 (ten condition frames, more
than two depths of the deepest ring).  B = 70 is three column tiles of 32 with a partial last one.  The reference widths
(R 256, S 512) run once: the only case whose tile loops go round more than once along M and K."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from oracle import ref_model as M

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_ref as G  # noqa: E402
import sampling_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu
DIL = [1, 2, 4, 8, 16] * 2
N, RATIO = 160, 16
MAX_EXCUSED = 0.002           # of B * n
SEED = 2024                   # of the B = 70 run: every row's history shows at least 16 distinct indices (checked on the CPU
#                               with oracle.ref_model.FastGenerator before it was committed, and asserted below)


def configs(R, S, ks, dil):
    m, w = G.tiny_cfg()                  # encoder 48 filters, latent 16, speaker embedding 16
    w.update(dilation_rates=list(dil), num_cycles=2, num_cycle_layers=len(dil) // 2, kernel_size=ks, dilation_filters=R,
             residual_filters=R, skip_filters=S, preprocess={"kernel_size": 32, "filters": R})
    return m, w


@pytest.fixture(scope='module')
def decoders(pkg):
    made = {}

    def get(R, S, ks, dil=DIL):
        key = (R, S, ks, tuple(dil))
        if key not in made:
            m, w = configs(R, S, ks, dil)
            P = M.init_params(m, w, 10, seed=100 + R + S + ks, randomize_all=True)
            model = pkg.model.VQVAE(m, w, 10, device='cuda', seed=0)
            model.load_named(P)
            made[key] = (model, P, w)
        return made[key]
    yield get
    made.clear()
    torch.cuda.empty_cache()


def inputs(model, B, n, ratio, seed):
    g = torch.Generator().manual_seed(seed)
    enc = 0.5 * torch.randn(B, model.Cc, n // ratio, generator=g)            # [B][Cc][Tz]: no encoder run needed
    u = torch.rand(B, n, generator=g)
    return enc, u


def check_audio(audio, idx):
    np.testing.assert_allclose(audio.cpu().numpy(), M.R.mu_law_decode_np(idx.cpu().numpy().astype(np.float32)), rtol=1e-5, atol=1e-6)


def check_a(P, w, enc, u, audio, idx, probs, depths=()):
    """(a) and (d) of one run from reset; returns p64."""
    check_audio(audio, idx)
    idx_h = idx.cpu().numpy()
    p64 = G.decoder_probs64(P, w, audio.cpu().numpy(), enc.permute(0, 2, 1), idx=idx_h)
    B, n = idx_h.shape
    excused = G.check_sampled(p64, u, idx_h, depths)
    print('\n[wide] B=%d n=%d: excused %d of %d' % (B, n, excused, B * n))
    assert excused <= MAX_EXCUSED * B * n, '%d of %d steps needed the cdf-edge excuse' % (excused, B * n)
    np.testing.assert_allclose(probs.cpu().numpy(), p64[:, -1], rtol=2e-4, atol=1e-7, err_msg='distribution of the last step')
    return p64


@pytest.fixture(scope='module')
def run70(pkg, decoders):
    """The B = 70 run every tiny-width test compares against: one generate call from reset, and its float64 reference."""
    model, P, w = decoders(32, 64, 3)
    enc, u = inputs(model, 70, N, RATIO, SEED)
    gen = pkg.generator.WideGenerator(model, batch=70)
    audio, idx, probs = gen.generate(enc.cuda(), N, mode='sample', uniforms=u.cuda(), ratio=RATIO, return_probs=True)
    p64 = check_a(P, w, enc, u, audio, idx, probs, G.ring_depths(3, DIL, persistent=False))
    yield dict(model=model, P=P, w=w, enc=enc, u=u, gen=gen, audio=audio, idx=idx, probs=probs, p64=p64)
    gen.close()


def test_b70_distribution_is_the_training_graphs(run70):
    """(a), (d): asserted when the fixture is made; here the history is shown to be varied."""
    distinct = [len(np.unique(r)) for r in run70['idx'].cpu().numpy()]
    assert min(distinct) >= 16, 'degenerate history: %s distinct indices per row' % distinct


def test_chunked_run_equals_single_run(run70):
    """(c): chunk ends around the steps where taps go live and rings wrap, one inside a condition frame (100), chunks that
    cross the refreshes of the condition window at steps 64 and 128 and chunks that start in the middle of a window."""
    r = run70
    gen, enc_d, u_d = r['gen'], r['enc'].cuda(), r['u'].cuda()
    ends = sorted(set(G.checkpoints(N, 3, 16)) | {100})
    assert any(t % RATIO for t in ends) and ends[-1] == N
    gen.reset()
    ia, aa, prev = [], [], 0
    for t in ends:
        a_c, i_c, p_c = gen.generate(enc_d, t - prev, mode='sample', uniforms=u_d[:, prev:t].contiguous(), ratio=RATIO,
                                     return_probs=True)
        ia.append(i_c)
        aa.append(a_c)
        np.testing.assert_allclose(p_c.cpu().numpy(), r['p64'][:, t - 1], rtol=2e-4, atol=1e-7, err_msg='distribution of step %d' % (t - 1))
        prev = t
    assert torch.equal(torch.cat(ia, 1), r['idx']) and torch.equal(torch.cat(aa, 1), r['audio'])
    assert torch.equal(p_c, r['probs'])


def test_rows_do_not_depend_on_the_batch(pkg, run70):
    """(b): rows 0..4 as a B = 5 generator, and as rows 65..69 of another B = 70 batch whose other rows differ."""
    r = run70
    model = r['model']
    want = (r['idx'][:5], r['audio'][:5], r['probs'][:5])
    g5 = pkg.generator.WideGenerator(model, batch=5)
    a, i, p = g5.generate(r['enc'][:5].contiguous().cuda(), N, mode='sample', uniforms=r['u'][:5].contiguous().cuda(), ratio=RATIO,
                          return_probs=True)
    g5.close()
    assert torch.equal(i, want[0]) and torch.equal(a, want[1]) and torch.equal(p, want[2])
    enc2, u2 = inputs(model, 70, N, RATIO, SEED + 1)
    enc2[65:], u2[65:] = r['enc'][:5], r['u'][:5]
    gen = r['gen']
    gen.reset()
    a, i, p = gen.generate(enc2.cuda(), N, mode='sample', uniforms=u2.cuda(), ratio=RATIO, return_probs=True)
    assert not torch.equal(i[:5], want[0])
    assert torch.equal(i[65:], want[0]) and torch.equal(a[65:], want[1]) and torch.equal(p[65:], want[2])


def test_kernel_size_two(pkg, decoders):
    model, P, w = decoders(32, 64, 2)
    enc, u = inputs(model, 33, N, RATIO, 5)
    gen = pkg.generator.WideGenerator(model, batch=33)
    audio, idx, probs = gen.generate(enc.cuda(), N, mode='sample', uniforms=u.cuda(), ratio=RATIO, return_probs=True)
    gen.close()
    check_a(P, w, enc, u, audio, idx, probs, G.ring_depths(2, DIL, persistent=False))


def test_one_row_and_refused_shapes(pkg, decoders):
    model, P, w = decoders(32, 64, 3)
    enc, u = inputs(model, 1, N, RATIO, 6)
    gen = pkg.generator.WideGenerator(model, batch=1)
    audio, idx, probs = gen.generate(enc.cuda(), N, mode='sample', uniforms=u.cuda(), ratio=RATIO, return_probs=True)
    gen.close()
    check_a(P, w, enc, u, audio, idx, probs)
    with pytest.raises(RuntimeError, match='batch=1025'):
        pkg.generator.WideGenerator(model, batch=1025)
    for field, value, match in (('R', 48, 'R=48'), ('Q', 1056, 'Q=1056')):
        keep = []
        wts = pkg.generator._weights_of(model, keep)
        setattr(wts, field, value)
        h = ctypes.c_void_p()
        assert pkg._lib.lib().vqw_ar_wide_create(ctypes.byref(h), ctypes.byref(wts), 4) != 0
        assert match in pkg._lib.lib().vqw_last_error().decode()


def test_truncated_rows(pkg, decoders):
    """(e): B = 12, rows alternating default / (0.8, 50, 0.9) / (1.3, 0, 0.5)."""
    model, P, w = decoders(32, 64, 3)
    B = 12
    sets = [(1.0, 0, 1.0), (0.8, 50, 0.9), (1.3, 0, 0.5)]
    enc, u = inputs(model, B, N, RATIO, 8)
    gen = pkg.generator.WideGenerator(model, batch=B)
    pa, pi, pp = gen.generate(enc.cuda(), N, mode='sample', uniforms=u.cuda(), ratio=RATIO, return_probs=True)
    gen.reset()
    ta, ti, tp = gen.generate(enc.cuda(), N, mode='sample', uniforms=u.cuda(), ratio=RATIO, return_probs=True,
                              temperature=[sets[b % 3][0] for b in range(B)], top_k=[sets[b % 3][1] for b in range(B)],
                              top_p=[sets[b % 3][2] for b in range(B)])
    gen.close()
    d = list(range(0, B, 3))
    assert torch.equal(ti[d], pi[d]) and torch.equal(ta[d], pa[d]) and torch.equal(tp[d], pp[d])
    check_audio(ta, ti)
    got = ti.cpu().numpy()
    p64 = G.decoder_probs64(P, w, ta.cpu().numpy(), enc.permute(0, 2, 1), idx=got)
    z = np.log(np.maximum(p64, 1e-300))                  # the reference's logits up to a constant per step
    un = u.double().numpy()
    for b in range(B):
        t, k, p = sets[b % 3]
        if b % 3 == 0:
            continue
        for i in range(N):
            pr, keep, q, want = S.restate(z[b, i], t, k, p, un[b, i])
            if got[b, i] != want or not keep[got[b, i]]:
                assert S.fp32_edge(pr, keep, q, k, p, un[b, i]), 'row %d step %d: GPU %d, restated %d' % (b, i, got[b, i], want)
        pl = tp[b].cpu().double().numpy()
        np.testing.assert_allclose(pl, q, rtol=2e-4, atol=1e-7)
        assert (pl[~keep] == 0).all()
        if k:
            assert keep.sum() <= k


def test_reference_widths(pkg, decoders):
    """R 256, S 512, dilations [1,2,4,8] * 2, B = 40, ratio 64, n = 128: (a) and (d)."""
    dil = [1, 2, 4, 8] * 2
    model, P, w = decoders(256, 512, 3, dil)
    enc, u = inputs(model, 40, 128, 64, 9)
    gen = pkg.generator.WideGenerator(model, batch=40)
    audio, idx, probs = gen.generate(enc.cuda(), 128, mode='sample', uniforms=u.cuda(), ratio=64, return_probs=True)
    gen.close()
    check_a(P, w, enc, u, audio, idx, probs, G.ring_depths(3, dil, persistent=False))


def test_lifecycle(pkg, run70, decoders):
    """Greedy is argmax(p64) up to ties within gen_ref.EDGE; reset then rerun reproduces the run; a second handle alive and
    running in between does not disturb the first."""
    r = run70
    model, P, w = r['model'], r['P'], r['w']
    B, n = 6, 96
    enc, u = inputs(model, B, n, RATIO, 10)
    enc_d, u_d = enc.cuda(), u.cuda()
    gen = pkg.generator.WideGenerator(model, batch=B)
    ga, gi, gp = gen.generate(enc_d, n, ratio=RATIO, return_probs=True)
    check_audio(ga, gi)
    got = gi.cpu().numpy().astype(np.int64)
    p64 = G.decoder_probs64(P, w, ga.cpu().numpy(), enc.permute(0, 2, 1), idx=got)
    want = p64.argmax(-1)                                  # the lowest index among the maxima
    gap = p64.max(-1) - np.take_along_axis(p64, got[:, :, None], -1)[:, :, 0]
    differ = got != want
    assert (gap[differ] < G.EDGE).all(), 'greedy is not argmax(p64) at %s' % (np.argwhere(differ & (gap >= G.EDGE))[:4],)
    assert differ.sum() <= MAX_EXCUSED * B * n
    np.testing.assert_allclose(gp.cpu().numpy(), p64[:, -1], rtol=2e-4, atol=1e-7)
    # reset + rerun, sampled, with a second handle working between the first one's chunks
    sa, si, sp = gen.generate(enc_d, n, mode='sample', uniforms=u_d, ratio=RATIO, return_probs=True)      # continues: other state
    gen.reset()
    a1, i1, p1 = gen.generate(enc_d, n, mode='sample', uniforms=u_d, ratio=RATIO, return_probs=True)
    other = pkg.generator.WideGenerator(model, batch=3)
    enc3, u3 = inputs(model, 3, n, RATIO, 11)
    gen.reset()
    a2, i2 = gen.generate(enc_d, 40, mode='sample', uniforms=u_d[:, :40].contiguous(), ratio=RATIO)
    oa, oi = other.generate(enc3.cuda(), n, mode='sample', uniforms=u3.cuda(), ratio=RATIO)
    a3, i3, p3 = gen.generate(enc_d, n - 40, mode='sample', uniforms=u_d[:, 40:].contiguous(), ratio=RATIO, return_probs=True)
    other.reset()
    ob, oj = other.generate(enc3.cuda(), n, mode='sample', uniforms=u3.cuda(), ratio=RATIO)
    other.close()
    gen.close()
    assert torch.equal(torch.cat([i2, i3], 1), i1) and torch.equal(torch.cat([a2, a3], 1), a1) and torch.equal(p3, p1)
    assert torch.equal(oi, oj) and torch.equal(oa, ob)
