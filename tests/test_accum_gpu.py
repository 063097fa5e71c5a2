"""Gradient accumulation on the GPU (WaveNet.accumulate).

* vqw_grad_accumulate against numpy, bit for bit: every size at which the kernel takes another path (below one vector, a tail,
  a second and third sweep of the grid), every aliasing form, every pointer 16-byte aligned and each one float off, guard bands,
  the skip guard, n = 0 and null pointers, non-finite values by class.
* The window's plumbing, exact: with the backward pass replaced by supplied gradients (the real step is not bitwise reproducible:
  split-K atomics), the closing call leaves fl(fl(g0 + g1) + g2) in the flat gradient and the optimiser's state is bitwise that
  of a twin that was handed the sum; the calls before it change nothing.
* N micro-batches against the oracle's gradient of the N * B rows as one batch, at the bars tests/test_model_gpu.py holds one
  step to (relative L2 5e-3 per variable, loss rtol 2e-5), for the VQ-VAE and the prior.
* The guarded engine: a flagged micro-step that closes a window with the next window's first enqueued behind it, deferred
  against immediate at test_deferred_guard_matches_immediate's bars; while the voided pair is pending nothing has changed.
* Two data-parallel ranks: one exchange per window.  The command lines.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import ref_model as M

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accum_ref as AR  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x7FA5A5A5      # (as int32) a NaN pattern no sum of the inputs produces
PAD = 8                # floats of guard band on either side (the view starts 16-byte aligned at PAD, + one float when offset)
SIZES = [1, 3, 4, 5, 1023, 2 * 2097152 + 1203]
# (out, acc, grad) roles: which of the three share one buffer.  'o' a buffer of its own, 'a' / 'g': out IS acc / grad
FORMS = [('copy', 'o'), ('copy', 'g'), ('add', 'o'), ('add', 'a'), ('add', 'g')]


def l2err(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm()) / max(float(b.norm()), 1e-30)


def bits(t):
    return t.view(torch.int32)


def inputs(n, seed):
    rng = np.random.default_rng(seed)
    mk = lambda: (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 21, n)).astype(np.float32)      # noqa: E731
    return mk(), mk()


class Buf:
    """n floats inside a sentinel-filled allocation: .view (offset `off` floats from a 16-byte boundary), .intact() = both guard
    bands still hold the sentinel."""

    def __init__(self, n, off, fill=None):
        self.base = torch.empty(n + 2 * PAD, device='cuda')
        bits(self.base).fill_(SENTINEL)
        self.lo, self.n = PAD + off, n
        self.view = self.base[self.lo:self.lo + n]
        assert self.view.data_ptr() % 16 == 4 * off
        if fill is not None:
            self.view.copy_(fill)

    def intact(self):
        b = bits(self.base)
        return bool((b[:self.lo] == SENTINEL).all()) and bool((b[self.lo + self.n:] == SENTINEL).all())


def run_form(K, form, alias, n, acc_d, grad_d, offs, skip=None):
    """One call in the given form with the buffers (out, acc, grad) `offs` floats off a 16-byte boundary; returns the three Bufs
    (acc None in the copy form; out is acc or grad where they alias)."""
    o_off, a_off, g_off = offs
    g = Buf(n, g_off, grad_d)
    a = Buf(n, a_off, acc_d) if form == 'add' else None
    out = Buf(n, o_off) if alias == 'o' else {'a': a, 'g': g}[alias]
    K.grad_accumulate(out.view, g.view, acc=a.view if a is not None else None, skip=skip)
    return out, a, g


def alignments(form, alias):
    """Every pointer aligned, then each distinct buffer one float off (offsets of out, acc, grad)."""
    distinct = (['o'] if alias == 'o' else []) + (['a'] if form == 'add' else []) + ['g']
    return [(0, 0, 0)] + [tuple(int(which == r) for r in 'oag') for which in distinct]


@pytest.mark.parametrize('n', SIZES)
def test_kernel_matches_numpy_bit_for_bit(K, n):
    acc, grad = inputs(n, n)
    want = {'copy': torch.from_numpy(AR.kernel(None, grad)).cuda(), 'add': torch.from_numpy(AR.kernel(acc, grad)).cuda()}
    acc_d, grad_d = torch.from_numpy(acc).cuda(), torch.from_numpy(grad).cuda()
    one, zero = torch.ones(1, dtype=torch.int32, device='cuda'), torch.zeros(1, dtype=torch.int32, device='cuda')
    for form, alias in FORMS:
        for offs in alignments(form, alias):
            for skip in (None, zero):
                out, a, g = run_form(K, form, alias, n, acc_d, grad_d, offs, skip)
                assert torch.equal(bits(out.view), bits(want[form])), (form, alias, offs)
                assert all(b.intact() for b in (out, a, g) if b is not None), (form, alias, offs)
                if a is not None and a is not out:          # the inputs that are not the output are read only
                    assert torch.equal(bits(a.view), bits(acc_d))
                if g is not out:
                    assert torch.equal(bits(g.view), bits(grad_d))
            # the guard: nothing is written, whatever the form (an aliased output keeps its input, a fresh one its sentinel)
            out, a, g = run_form(K, form, alias, n, acc_d, grad_d, offs, one)
            if alias == 'o':
                assert bool((bits(out.view) == SENTINEL).all()), (form, alias, offs)
            else:
                assert torch.equal(bits(out.view), bits(acc_d if alias == 'a' else grad_d)), (form, alias, offs)
            assert all(b.intact() for b in (out, a, g) if b is not None)


def test_kernel_empty_and_null(pkg, K):
    L = pkg._lib
    lib, st = L.lib(), L.stream()
    g = torch.ones(8, device='cuda')
    o = torch.zeros(8, device='cuda')
    assert lib.vqw_grad_accumulate(None, None, None, 0, None, st) == 0          # n = 0: no launch, nothing looked at
    K.grad_accumulate(o[:0], g)
    assert lib.vqw_grad_accumulate(None, None, L.ptr(g), 8, None, st) != 0 and b'null' in lib.vqw_last_error()
    assert lib.vqw_grad_accumulate(L.ptr(o), L.ptr(g), None, 8, None, st) != 0 and b'null' in lib.vqw_last_error()
    torch.cuda.synchronize()
    assert float(o.abs().max()) == 0.0
    with pytest.raises(ValueError):
        K.grad_accumulate(o, g[:4])
    with pytest.raises(ValueError):
        K.grad_accumulate(o, g, acc=g.double())
    with pytest.raises(ValueError):
        K.grad_accumulate(o, g, skip=torch.zeros(1, device='cuda'))


def test_kernel_non_finite_values_by_class(K):
    n = 1023
    acc, grad = inputs(n, 99)
    special = [np.nan, np.inf, -np.inf]
    for i, v in enumerate(special):           # alone in acc, alone in grad, and against each other (inf - inf = NaN)
        acc[10 + i] = v
        grad[20 + i] = v
        for j, u in enumerate(special):
            acc[40 + 3 * i + j], grad[40 + 3 * i + j] = v, u
    acc[1000], grad[1000] = np.float32(3e38), np.float32(3e38)          # overflows to +Inf
    want = AR.kernel(acc, grad)
    assert np.isnan(want).sum() >= 8 and np.isposinf(want).sum() >= 3 and np.isneginf(want).sum() >= 2
    for alias in 'oag':
        out = run_form(K, 'add', alias, n, torch.from_numpy(acc).cuda(), torch.from_numpy(grad).cuda(), (0, 0, 0))[0]
        assert AR.same_by_class(out.view.cpu().numpy(), want), alias
    out = run_form(K, 'copy', 'o', n, None, torch.from_numpy(grad).cuda(), (1, 0, 0))[0]
    assert AR.same_by_class(out.view.cpu().numpy(), AR.kernel(None, grad))


# ------------------------------------------------------------------ the window's plumbing, exact
def tiny_cfg():
    import importlib.util
    spec = importlib.util.spec_from_file_location('make_golden', os.path.join(ROOT, 'tests', 'golden', 'make_golden.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.tiny_cfg()


def tiny_model(pkg, P):
    m, w = tiny_cfg()
    model = pkg.model.VQVAE(m, w, 10, device='cuda', seed=0)
    model.load_named(P)
    return model


@pytest.mark.parametrize('clip', [None, 0.5])
def test_window_plumbing_is_exact(pkg, monkeypatch, clip):
    monkeypatch.setenv('VQW_ENGINE', 'fp32')
    m, w = tiny_cfg()
    P = M.init_params(m, w, 10, seed=11, randomize_all=True)
    model, twin = tiny_model(pkg, P), tiny_model(pkg, P)
    x, spk, _ = M.synthetic_batch(2, 512, 10, 1234)
    xd, sd = x[:, :, 0].contiguous().cuda(), spk.cuda()
    rng = np.random.default_rng(3)
    gs = [(rng.standard_normal(model.n_flat) * 2.0 ** rng.integers(-20, 21, model.n_flat)).astype(np.float32) * np.float32(1e-3)
          for _ in range(3)]
    gd = [torch.from_numpy(g).cuda() for g in gs]
    calls = []

    def supplied(x_, spk_, ws_):             # in place of the backward pass (the forward pass is the real one)
        model.grad.copy_(gd[len(calls)])
        calls.append(1)
    model.backward = supplied
    model.accumulate, model.clip_norm, twin.clip_norm = 3, clip, clip
    state = lambda mdl: [getattr(mdl, k).clone() for k in ('flat', 'ema', 'adam_m', 'adam_v')]      # noqa: E731
    before = state(model)
    for k in range(2):
        model.train_step(xd, sd)
        assert model.global_step == 0 and model.accum_index == k + 1
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(state(model), before)), 'micro-step %d changed the optimiser state' % k
    model.train_step(xd, sd)
    assert model.global_step == 1 and model.accum_index == 0 and len(calls) == 3
    want = AR.window_sum(gs)
    assert not np.array_equal(want, AR.window_sum_right_to_left(gs))            # (the order shows at this size)
    assert torch.equal(bits(model.grad), bits(torch.from_numpy(want).cuda()))
    twin.grad.copy_(torch.from_numpy(want))
    twin.apply_gradients(1.0 / 3)
    for name, a, b in zip(('flat', 'ema', 'adam_m', 'adam_v'), state(model), state(twin)):
        assert torch.equal(bits(a), bits(b)), name
    assert not torch.equal(model.flat, before[0])
    if clip is not None:
        na, nb = model.grad_norms(), twin.grad_norms()
        assert na['global'] == nb['global'] and na['scale'] == nb['scale'] and na['global'] > 0


# ------------------------------------------------------------------ equivalence to the big batch
def test_window_equals_the_big_batch_vqvae(pkg, monkeypatch):
    monkeypatch.setenv('VQW_ENGINE', 'fp32')
    m, w = tiny_cfg()
    N, B, T = 3, 2, 512
    P = M.init_params(m, w, 10, seed=11, randomize_all=True)
    x, spk, _ = M.synthetic_batch(N * B, T, 10, 1234)
    model, big = tiny_model(pkg, P), tiny_model(pkg, P)
    out, grads = M.train_step(x, spk, {k: v.clone() for k, v in P.items()}, m, w, {'t': 0, 'm': {}, 'v': {}, 'ema': {}}, 0)
    xd, sd = x[:, :, 0].contiguous().cuda(), spk.cuda()
    model.accumulate = N
    losses = []
    for k in range(N):
        ws = model.train_step(xd[k * B:(k + 1) * B].contiguous(), sd[k * B:(k + 1) * B].contiguous())
        losses.append(model.losses(ws)[0])
    assert model.global_step == 1 and model.accum_index == 0
    big.train_step(xd, sd)
    got, own = model.named_gradients(), big.named_gradients()
    worst = (0.0, '')
    for name, gref in grads.items():
        e, e_own = l2err(got[name] / N, gref), l2err(got[name] / N, own[name])
        print('%-60s window vs oracle %.3e   window vs the library\'s big batch %.3e' % (name, e, e_own))
        worst = max(worst, (e, name))
    print('loss: mean of the micro losses %.8f, oracle big batch %.8f' % (float(np.mean(losses)), out['loss'].item()))
    assert worst[0] < 5e-3, worst
    np.testing.assert_allclose(np.mean(losses), out['loss'].item(), rtol=2e-5)


def test_window_equals_the_big_batch_prior(pkg, monkeypatch):
    from test_prior_gpu import rand_codes, random_params, ref_step, tiny_prior
    monkeypatch.setenv('VQW_ENGINE', 'fp32')
    cfg = tiny_prior(k=32, pre_k=3)
    N, B, T = 2, 2, 256
    prior, big = (pkg.prior.LatentPrior(cfg, 10, device='cuda', seed=0) for _ in range(2))
    P = random_params(prior, 7)
    prior.load_named(P)
    big.load_named(P)
    codes, spk = rand_codes(N * B, T, 32, 10), torch.tensor([3, 8, 0, 9])
    _, ref_loss, grads = ref_step(codes, spk, {k: v.clone() for k, v in P.items()}, cfg, {'t': 0, 'm': {}, 'v': {}, 'ema': {}})
    cd, sd = codes.int().cuda(), spk.cuda()
    prior.accumulate = N
    losses = []
    for k in range(N):
        ws = prior.train_step(cd[k * B:(k + 1) * B].contiguous(), sd[k * B:(k + 1) * B].contiguous())
        losses.append(prior.losses(ws)[0])
    assert prior.global_step == 1 and prior.accum_index == 0
    big.train_step(cd, sd)
    got, own = prior.named_gradients(), big.named_gradients()
    worst = (0.0, '')
    for name, gref in grads.items():
        e, e_own = l2err(got[name] / N, gref), l2err(got[name] / N, own[name])
        print('%-60s window vs restatement %.3e   window vs the library\'s big batch %.3e' % (name, e, e_own))
        worst = max(worst, (e, name))
    print('loss: mean of the micro losses %.8f, restatement big batch %.8f' % (float(np.mean(losses)), ref_loss))
    assert worst[0] < 5e-3, worst
    np.testing.assert_allclose(np.mean(losses), ref_loss, rtol=2e-5)


# ------------------------------------------------------------------ the guarded engine: deferred against immediate
def test_flagged_closing_micro_step_deferred_matches_immediate(pkg, monkeypatch):
    """dp_worker.guard_problem's recipe, accumulate = 2, micro-batches silent, loud, silent, silent: the loud one closes window 0
    and is flagged; deferred, the first micro-step of window 1 is enqueued behind it and both are voided.  While the pair is
    pending, the accumulator (window 0's first gradient, which the replay needs), parameters, optimiser state and the plane
    scales the optimiser's guard covers are bitwise what they were before the loud micro-step was enqueued."""
    import dp_worker
    monkeypatch.setenv('VQW_ENGINE', 'f16x3')
    monkeypatch.delenv('VQW_GATE_F16X3', raising=False)
    m, w, P, x, spk = dp_worker.guard_problem()
    silent, loud = (x[:2].contiguous().cuda(), spk[:2].contiguous().cuda()), (x[2:].contiguous().cuda(), spk[2:].contiguous().cuda())
    order = [silent, loud, silent, silent]
    kept = ('_acc', 'flat', 'ema', 'adam_m', 'adam_v')
    models = []
    for defer in (False, True):
        model = pkg.model.VQVAE(m, w, 10, device='cuda', seed=0)
        model.load_named(P)
        assert model.x3_guard
        model.defer_guard, model.accumulate = defer, 2
        # the scales every pass makes again from its own weights and input before it uses them: no part of the guarded state
        SL = model.SL
        guarded = [i for i in range(SL['N']) if i not in (SL['WG'], SL['WO'], SL['X'], SL['WH'])]
        seen = {}
        if defer:
            resolve = model._resolve_oldest

            def watched():
                if len(model._pending) == 2 and model._pending[0]['x'] is loud[0]:
                    torch.cuda.synchronize()
                    now = [getattr(model, k) for k in kept] + [model.x3_scale[guarded]]
                    seen['intact'] = [bool(torch.equal(bits(a), bits(b))) for a, b in zip(now, seen['before'])]
                    seen['k'] = [p['k'] for p in model._pending]
                resolve()
            model._resolve_oldest = watched
        for i, (xd, sd) in enumerate(order):
            if i == 1:
                seen['before'] = [getattr(model, k).clone() for k in kept] + [model.x3_scale[guarded].clone()]
            model.train_step(xd, sd)
        model.finish_steps()
        if defer:
            assert seen.get('intact') == [True] * 6 and seen['k'] == [1, 0], seen
        assert model.global_step == 2 and model.accum_index == 0 and not model._pending and int(model.x3_void.item()) == 0
        models.append(model)
    a, b = models
    assert a.x3_fallbacks == b.x3_fallbacks >= 1, (a.x3_fallbacks, b.x3_fallbacks)
    for name, bar in (('flat', 3e-3), ('ema', 3e-3), ('adam_v', 2e-1), ('adam_m', 3e-1)):      # test_deferred_guard_matches_immediate's
        ta, tb = getattr(a, name), getattr(b, name)
        assert torch.isfinite(tb).all(), name
        print('%s: deferred vs immediate rel. L2 %.3e' % (name, l2err(tb, ta)))
        assert l2err(tb, ta) < bar, '%s: deferred vs immediate rel. L2 %.3e' % (name, l2err(tb, ta))


# ------------------------------------------------------------------ data parallel
def test_two_ranks_exchange_once_per_window(pkg, tmp_path):
    from test_multirank_gpu import run_ranks
    import accum_dp_worker
    run_ranks([os.path.join(ROOT, 'tests', 'accum_dp_worker.py'), str(tmp_path), 'gloo'], 2)
    r0 = torch.load(str(tmp_path / 'rank0.pt'), weights_only=True)
    r1 = torch.load(str(tmp_path / 'rank1.pt'), weights_only=True)
    assert torch.equal(bits(r0['flat']), bits(r1['flat'])) and torch.equal(bits(r0['ema']), bits(r1['ema'])), 'ranks diverged'
    assert torch.equal(bits(r0['grad']), bits(r1['grad']))
    for r in (r0, r1):
        assert int(r['global_step']) == 1 and int(r['accum_index']) == 0
        assert int(r['sum_calls_window']) == int(r['sum_calls_normal']) >= 3, (r['sum_calls_window'], r['sum_calls_normal'])
    # a single-process window of N = 4 over the same eight rows in the same order
    m, w, P, x, spk = accum_dp_worker.problem()
    single = pkg.model.VQVAE(m, w, 10, device='cuda', seed=0)
    single.load_named(P)
    single.accumulate = 4
    for k in range(4):
        single.train_step(x[2 * k:2 * k + 2].contiguous().cuda(), spk[2 * k:2 * k + 2].contiguous().cuda())
    assert single.global_step == 1
    want = single.named_gradients()
    twin = pkg.model.VQVAE(m, w, 10, device='cuda', seed=0)      # (rank 0's flat gradient under the variables' names)
    twin.grad.copy_(r0['grad'])
    got = twin.named_gradients()
    for name in want:
        e = l2err(got[name] / 4, want[name] / 4)
        assert e < 5e-3, (name, e)


# ------------------------------------------------------------------ command lines
def _tiny_files(tmp_path):
    from test_prior_gpu import tiny_prior
    w = {"verbose": False, "quantization_channels": 256, "num_cycles": 1, "num_cycle_layers": 4,
         "dilation_rates": [1, 2, 4, 8], "kernel_size": 3, "dilation_filters": 32, "skip_filters": 64,
         "residual_filters": 32, "preprocess": {"kernel_size": 32, "filters": 32}}
    m = {"encoder": "64", "use_vq": True, "speaker_embedding": 16, "k": 32, "latent_dim": 16, "beta": 0.25,
         "encoder_filters": 48, "wavenet_parameters": str(tmp_path / 'w.json'), "verbose": False,
         "learning_rate_schedule": {"0": 1e-3}}
    (tmp_path / 'w.json').write_text(json.dumps(w))
    (tmp_path / 'm.json').write_text(json.dumps(m))
    (tmp_path / 'p.json').write_text(json.dumps(tiny_prior(k=32, pre_k=2)))


def _summaries(path):
    with open(str(path)) as f:
        return [json.loads(ln) for ln in f if ln.strip()]


def test_cli_train_and_train_prior_accumulate(tmp_path):
    _tiny_files(tmp_path)
    env = dict(os.environ, PYTHONPATH=ROOT)
    run = lambda args: subprocess.run([sys.executable] + args, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)  # noqa: E731
    out = run([os.path.join(ROOT, 'train.py'), '-dataset', 'synthetic', '-length', '512', '-batch', '2', '-accumulate', '2', '-step', '2',
               '-interval', '1', '-save', 'saved_model/weights', '-params', str(tmp_path / 'm.json')])
    assert out.returncode == 0, out.stderr[-2000:]
    assert (tmp_path / 'saved_model' / 'weights-2.pt').exists()
    lines = _summaries(tmp_path / 'saved_model' / 'summaries.jsonl')
    assert [ln['global_step'] for ln in lines] == [1, 2] and all(ln['accumulate'] == 2 for ln in lines), lines
    assert out.stdout.count('[accum 2]') == 2, out.stdout[-500:]
    out = run([os.path.join(ROOT, 'train_prior.py'), '-restore', 'saved_model/weights-2.pt', '-dataset', 'synthetic', '-length', '256',
               '-batch', '2', '-accumulate', '2', '-step', '2', '-interval', '1', '-save', 'saved_prior/prior',
               '-params', str(tmp_path / 'p.json'), '-vqvae_params', str(tmp_path / 'm.json')])
    assert out.returncode == 0, out.stderr[-2000:]
    assert (tmp_path / 'saved_prior' / 'prior-2.pt').exists()
    lines = _summaries(tmp_path / 'saved_prior' / 'summaries.jsonl')
    assert [ln['global_step'] for ln in lines] == [1, 2] and all(ln['accumulate'] == 2 for ln in lines), lines
    assert out.stdout.count('[accum 2]') == 2, out.stdout[-500:]
