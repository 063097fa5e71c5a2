"""Seeded runs of every generator (generator.FastGenerator on its three layouts, WideGenerator, PriorGenerator,
WidePriorGenerator) through their public methods only.  Every case returns the raw bytes of every tensor it was handed back:
indices, audio and the probabilities of the last step.  tests/golden/make_generator_digests.py hashes them into
tests/golden/generator_digests.json; tests/test_generator_digests_gpu.py compares against that file.

Tiny widths (gen_ref.tiny_cfg: R 32, S 64, Q 256, pre_k 32; test_prior_gpu.tiny_prior(k=32, pre_k=3)), B = 3 rows (more than
one row per handle is what reuses a sampling block's scratch from row to row), N = 96 steps as one call and as 40 + 56 (the
second condition frame starts at step 64, inside the second chunk).  A case name is backend/draw; its outputs carry the suffix
`_split` for the 40 + 56 run."""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_ref as G  # noqa: E402
from oracle import ref_model as M  # noqa: E402

B, N, CUT, RATIO = 3, 96, 40, 64
ENV = ('VQW_AR_PERSISTENT', 'VQW_AR_CPB', 'VQW_AR_ROWS', 'VQW_AR_PLACE')
# backend -> (generator class, model, the environment it is constructed under [the rest of ENV unset], _parts)
BACKENDS = {
    'fast-phased': ('FastGenerator', 'audio', {'VQW_AR_PERSISTENT': '0', 'VQW_AR_ROWS': '3'}, [3]),
    'fast-one-handle': ('FastGenerator', 'audio', {'VQW_AR_PERSISTENT': '1', 'VQW_AR_ROWS': '3'}, [3]),
    'fast-one-row-handles': ('FastGenerator', 'audio', {'VQW_AR_PERSISTENT': '1'}, [1, 1, 1]),
    'wide': ('WideGenerator', 'audio', {}, None),
    'prior': ('PriorGenerator', 'prior', {'VQW_AR_PERSISTENT': '1'}, [1, 1, 1]),
    'wide-prior': ('WidePriorGenerator', 'prior', {}, None),
    # equal logits (postprocess2 all zero): the first-maximum rule decides greedy, the cdf is a ramp
    'flat/fast-phased': ('FastGenerator', 'flat', {'VQW_AR_PERSISTENT': '0', 'VQW_AR_ROWS': '3'}, [3]),
    'flat/fast-one-handle': ('FastGenerator', 'flat', {'VQW_AR_PERSISTENT': '1', 'VQW_AR_ROWS': '3'}, [3]),
    'flat/wide': ('WideGenerator', 'flat', {}, None),
}
# draw -> keywords of generate() / sample() beside the uniforms
DRAWS = {
    'greedy': dict(mode='greedy'),
    'sample': dict(mode='sample'),
    'mixed': dict(mode='sample', temperature=[1.0, 0.7, 1.0], top_k=[0, 5, 0], top_p=[1.0, 1.0, 0.6]),
}


def environment(backend):
    """{variable: value or None (unset)} a backend's generator is constructed under."""
    return {k: BACKENDS[backend][2].get(k) for k in ENV}


def make_models(pkg):
    """The three models of the cases, built as test_sampling_gpu.py and test_wide_prior_gpu.py build theirs."""
    m, w = G.tiny_cfg()
    P = M.init_params(m, w, 10, seed=11, randomize_all=True)
    audio = pkg.model.VQVAE(m, w, 10, device='cuda', seed=0)
    audio.load_named(P)
    Pf = dict(P)
    for n in ('decoder/postprocess2/kernel', 'decoder/postprocess2/bias'):
        Pf[n] = torch.zeros_like(P[n])
    flat = pkg.model.VQVAE(m, w, 10, device='cuda', seed=0)
    flat.load_named(Pf)
    T = G.prior_tests()
    prior = pkg.prior.LatentPrior(T.tiny_prior(k=32, pre_k=3), 10, device='cuda', seed=0)
    prior.load_named(T.random_params(prior, 21))
    return {'audio': audio, 'flat': flat, 'prior': prior}


def inputs():
    """(encoding [B][Cc][2], speakers [B], uniforms [B][N]) on the CPU; one uniform lies above every cdf."""
    g = torch.Generator().manual_seed(2025)
    enc = 0.5 * torch.randn(B, 32, -(-N // RATIO), generator=g)
    u = torch.rand(B, N, generator=g)
    u[1, 7] = 2.0
    return enc, torch.tensor([4, 0, 7], dtype=torch.int64), u


def raw(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


def digest(outputs):
    return {k: hashlib.sha256(raw(v)).hexdigest() for k, v in sorted(outputs.items())}


def run_backend(pkg, models, backend):
    """{case: {output: sha256}} of one backend; the caller has set environment(backend)."""
    cls, which, _, parts = BACKENDS[backend]
    model = models[which]
    enc, spk, u = (t.cuda() for t in inputs())
    code = which == 'prior'
    assert code or enc.shape[1] == model.Cc
    gen = getattr(pkg.generator, cls)(model, batch=B)
    if parts is not None:
        assert gen._parts == parts, 'layout %s, expected %s' % (gen._parts, parts)
    names = ('idx', 'probs') if code else ('audio', 'idx', 'probs')

    def call(n, kw, t0):
        if kw['mode'] == 'sample':
            kw = dict(kw, uniforms=u[:, t0:t0 + n].contiguous())
        if code:
            return gen.sample(n, spk, return_probs=True, **kw)
        return gen.generate(enc, n, ratio=RATIO, return_probs=True, **kw)

    out = {}
    try:
        for draw, kw in DRAWS.items():
            if which == 'flat' and draw == 'mixed':
                continue
            gen.reset()
            res = dict(zip(names, call(N, kw, 0)))
            gen.reset()
            a, b = call(CUT, kw, 0), call(N - CUT, kw, CUT)
            for i, n in enumerate(names):
                res[n + '_split'] = b[i] if n == 'probs' else torch.cat([a[i], b[i]], 1)
            out['%s/%s' % (backend, draw)] = digest(res)
    finally:
        gen.close()
    return out
