"""Gradient accumulation without a GPU (WaveNet.accumulate): the facts the GPU comparison rests on (the fp32 sum's
order is part of the contract, and a wrong order is caught), the host's launch sequence over a window recorded on the CPU
(tests/launch_trace.py) -- which call copies, adds, closes; where the norm pass, Adam and the gradient exchange sit; what a voided
pair is replayed as -- and the refusals, each raised before a launch."""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import accum_ref as AR  # noqa: E402
import launch_trace as LT  # noqa: E402
from test_launch_trace_cpu import GOLDEN  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ reference facts
def planted():
    """Three gradients whose fp32 sum depends on the order: 2^24 + 1 is not an fp32 number."""
    g0 = np.array([2.0 ** 24, 1.0, -1.0], np.float32)
    g1 = np.array([1.0, 2.0 ** 24, 2.0 ** 24], np.float32)
    g2 = np.array([1.0, 1.0, 2.0], np.float32)
    return [g0, g1, g2]


def test_the_fp32_order_is_part_of_the_contract():
    grads = planted()
    want = AR.window_sum(grads)
    assert want.dtype == np.float32
    assert want.tolist() == [2.0 ** 24] * 3         # every add of 1 to 2^24 is a tie and goes to the even neighbour, 2^24; (2^24 - 1) + 2 likewise
    assert AR.window_sum_fp64(grads).tolist() == [2.0 ** 24 + 2, 2.0 ** 24 + 2, 2.0 ** 24 + 1]
    assert not np.array_equal(want.astype(np.float64), AR.window_sum_fp64(grads))
    assert np.array_equal(AR.kernel(AR.kernel(AR.kernel(None, grads[0]), grads[1]), grads[2]), want)


def test_a_wrong_sum_fails_the_comparison_the_gpu_test_makes():
    grads = planted()
    want = AR.window_sum(grads)
    assert AR.same_by_class(AR.window_sum(grads), want)
    assert not AR.same_by_class(AR.window_sum_right_to_left(grads), want)
    assert not AR.same_by_class(AR.window_sum_closing_twice(grads), want)
    rng = np.random.default_rng(5)
    rnd = [(rng.standard_normal(4096) * 2.0 ** rng.integers(-20, 21, 4096)).astype(np.float32) for _ in range(3)]
    assert not AR.same_by_class(AR.window_sum_right_to_left(rnd), AR.window_sum(rnd))
    assert not AR.same_by_class(AR.window_sum_closing_twice(rnd), AR.window_sum(rnd))


def test_same_by_class_compares_non_finite_values_by_class():
    nan2 = np.array([0x7FC00001], np.uint32).view(np.float32)[0]
    a = np.array([np.nan, np.inf, -np.inf, 1.0, 0.0], np.float32)
    assert AR.same_by_class(a, np.array([nan2, np.inf, -np.inf, 1.0, 0.0], np.float32))
    for i, v in enumerate([1.0, -np.inf, np.inf, np.nan, -0.0]):
        b = a.copy()
        b[i] = v
        assert not AR.same_by_class(a, b), i


def test_schedule_is_the_window_bookkeeping():
    s = AR.schedule(3, 4)
    assert [c['form'] for c in s] == ['copy', 'add', 'close', 'copy']
    assert [c['global_step'] for c in s] == [0, 0, 1, 1] and [c['accum_index'] for c in s] == [1, 2, 0, 1]
    assert [c['form'] for c in AR.schedule(2, 4)] == ['copy', 'close', 'copy', 'close']
    assert [c['form'] for c in AR.schedule(1, 2)] == ['step', 'step'] and AR.schedule(1, 2)[-1]['global_step'] == 2


# ------------------------------------------------------------------ the launch sequence
class HoldingStub(LT.GradSyncStub):
    """The recording stub with GradAllReduce's hold switch: held, bucket_ready records no exchange (the range is kept for the
    release, as there) and finish() waits for nothing."""
    hold = False

    def __init__(self, rec):
        super().__init__(rec)
        self.held, self.last_held = [], []

    def bucket_ready(self, lo, hi):
        if self.hold:
            self.held.append((lo, hi))
        else:
            super().bucket_ready(lo, hi)

    def finish(self):
        if self.hold:
            self.last_held, self.held = self.held, []
        return self.world


@contextlib.contextmanager
def recorded(pkg, kind=None, keys=None):
    """(recorder, model) of a fresh CPU model of launch_trace's configs under the recorder; the host-side helpers of the norm
    pass, which the recorder would replace too, stay what they are."""
    keep = {n: getattr(pkg.kernels, n) for n in ('clip_as_fp32', 'grad_norm_plan_runs')}
    with pytest.MonkeyPatch.context() as mp:
        LT.set_switches(mp, {})
        rec = LT.install(mp, pkg)
        for n, fn in keep.items():
            mp.setattr(pkg.kernels, n, fn)
        model = LT.make_model(pkg, kind, keys or {})
        del rec.trace[:]
        yield rec, model


def batch(kind, B=1, T=1024):
    return torch.zeros(B, T, dtype=torch.int32 if kind == 'prior' else torch.float32), torch.zeros(B, dtype=torch.int64)


def ordinal(rec, t):
    return rec.tensor(t)[1]


def roles(rec, model, entry):
    """(out, acc, grad) of a grad_accumulate entry as 'acc' / 'grad' / None (not passed)."""
    names = {ordinal(rec, model.grad): 'grad', ordinal(rec, model._acc): 'acc'}
    return tuple(names[entry[3][k][1]] if k in entry[3] else None for k in ('out', 'acc', 'grad'))


def named(trace, name):
    return [i for i, e in enumerate(trace) if e[0] == name]


@pytest.mark.parametrize('kind', [None, 'prior'])
def test_a_window_of_three(pkg, kind):
    with recorded(pkg, kind) as (rec, model):
        assert model.accumulate == 1 and model.accum_index == 0 and model._acc is None
        model.accumulate = 3
        model.clip_norm = 1.0
        assert model._acc is None and rec.trace == []            # nothing allocated or launched by the setters
        x, spk = batch(kind)
        ends, seen = [], []
        want = AR.schedule(3, 4)
        for c in want:
            model.train_step(x, spk)
            ends.append(len(rec.trace))
            seen.append((model.global_step, model.accum_index))
        assert seen == [(c['global_step'], c['accum_index']) for c in want] == [(0, 1), (0, 2), (1, 0), (1, 1)]
        trace = rec.trace
        acc = named(trace, 'grad_accumulate')
        assert len(acc) == 4 and [sum(1 for i in acc if i < e) for e in ends] == [1, 2, 3, 4]       # one per call
        assert [roles(rec, model, trace[i]) for i in acc] == [('acc', None, 'grad'), ('acc', 'acc', 'grad'), ('grad', 'acc', 'grad'),
                                                              ('acc', None, 'grad')]
        for i in acc:
            assert 'skip' not in trace[i][3] and trace[i][3]['out'][2:] == [0, model.n_flat, 'torch.float32']
        # one optimiser step, after the third pass: norm pass and Adam behind the closing sum, both on 1/3 of the flat gradient
        adam, norm = named(trace, 'adam_ema_step'), named(trace, 'grad_norm')
        assert len(adam) == 1 and len(norm) == 1 and ends[1] <= acc[2] < norm[0] < adam[0] < ends[2]
        g = ordinal(rec, model.grad)
        assert trace[adam[0]][3]['grad'][1] == g and trace[norm[0]][3]['buf'][1] == g
        assert trace[adam[0]][2]['grad_scale'] == trace[norm[0]][2]['grad_scale'] == 1.0 / 3
        # the accumulator's storage is first seen in the first accumulating call
        a = ordinal(rec, model._acc)
        uses = [i for i, e in enumerate(trace) if any(isinstance(v, list) and v[:1] == ['tensor'] and v[1] == a for v in e[3].values())]
        assert uses == acc


@pytest.mark.parametrize('kind', [None, 'prior'])
def test_accumulate_one_is_the_step_as_it_was(pkg, kind):
    traces = []
    for touch in (False, True):
        with recorded(pkg, kind) as (rec, model):
            if touch:
                model.accumulate = 1
            model.train_step(*batch(kind))
            assert model.global_step == 1 and model.accum_index == 0 and model._acc is None
            traces.append(list(rec.trace))
    assert traces[0] == traces[1] and not named(traces[0], 'grad_accumulate')
    assert LT.digest(traces[1]) == GOLDEN['cases']['prior-train-step' if kind else 'train-step']['sha256']


def test_a_voided_pair_is_replayed_with_its_own_k(pkg):
    """launch_trace's run='deferred', void=True recipe with accumulate = 2: both first attempts run behind the skip guard, the
    older is repeated on the fp32 engine as micro-step 0 (a copy), the younger runs again as micro-step 1 (it closes)."""
    with recorded(pkg) as (rec, model):
        model.accumulate = 2
        model.defer_guard = True
        model.x3_void.fill_(1)
        x, spk = batch(None)
        model.train_step(x, spk)
        assert (model.global_step, model.accum_index) == (0, 1)
        n1 = len(rec.trace)
        model.train_step(x, spk)
        model.finish_steps()
        assert (model.global_step, model.accum_index) == (1, 0)
        trace = rec.trace
        acc, adam = named(trace, 'grad_accumulate'), named(trace, 'adam_ema_step')
        assert [roles(rec, model, trace[i]) for i in acc] == [('acc', None, 'grad'), ('grad', 'acc', 'grad')] * 2
        assert acc[0] < n1 <= acc[1] and len(adam) == 2 and acc[1] < adam[0] < acc[2] and acc[3] < adam[1]
        void = ordinal(rec, model.x3_void)
        first = adam[0]                  # everything up to the first Adam entry: the two first attempts
        for i, e in enumerate(trace):
            if e[0] in ('grad_accumulate', 'f16x3_update_scales', 'adam_ema_step') and i <= first:
                if e[0] == 'f16x3_update_scales' and 'flag' in e[3]:
                    continue             # (the forward pass's exact weight / input scales raise the flag: unguarded as they always were)
                assert e[3]['skip'][1] == void, (i, e[0])
            elif e[0] in ('grad_accumulate', 'adam_ema_step'):
                assert 'skip' not in e[3], (i, e[0])
        # the fp32 engine's gate-kernel weight gradient (layer 1): only in the older entry's replay
        fp32 = [i for i, e in enumerate(trace) if e[0] == 'wgrad_gemm' and e[2]['taps'] == [-2, -1, 0]]
        assert len(fp32) == 1 and adam[0] < fp32[0] < acc[2]
        assert trace[adam[1]][2]['grad_scale'] == 0.5


def test_the_exchange_runs_once_per_window_behind_the_closing_sum(pkg):
    with recorded(pkg) as (rec, model):
        model.grad_sync = HoldingStub(rec)
        model.accumulate = 3
        x, spk = batch(None)
        ends = []
        for _ in range(3):
            model.train_step(x, spk)
            ends.append(len(rec.trace))
        trace = rec.trace
        ready, acc = named(trace, 'grad_sync.bucket_ready'), named(trace, 'grad_accumulate')
        assert ready and all(acc[2] < i < named(trace, 'adam_ema_step')[0] for i in ready)
        ranges = sorted((trace[i][2]['lo'], trace[i][2]['hi']) for i in ready)
        assert ranges[0][0] == 0 and ranges[-1][1] == model.n_flat
        assert all(lo < hi for lo, hi in ranges) and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
        assert model.grad_sync.hold is False
        # accumulate = 1 again: the buckets leave during the backward pass, as they always did
        model.accumulate = 1
        del trace[:]
        model.train_step(x, spk)
        assert len(named(trace, 'grad_sync.bucket_ready')) == 7 and not named(trace, 'grad_accumulate')


def test_grad_all_reduce_hold(pkg, monkeypatch):
    calls = []
    monkeypatch.setattr(pkg.parallel.dist, 'all_reduce', lambda t, **kw: calls.append((t.numel(), kw.get('op'))))
    g = pkg.parallel.GradAllReduce(torch.zeros(64))
    assert g.hold is False and g.world == 1
    g.active = True                     # (what force=True gives under an initialised process group)
    g.hold = True
    g.bucket_ready(0, 40)
    g.bucket_ready(40, 64)
    assert calls == [] and g.buckets == [] and g.pending == [] and g.held == [(0, 40), (40, 64)]
    assert g.finish() == 1 and calls == [] and g.last_held == [(0, 40), (40, 64)] and g.held == []
    g.all_reduce_max(torch.zeros(1, dtype=torch.int32))      # the range flag's exchange is never held
    assert [c[0] for c in calls] == [1]
    g.hold = False
    g.bucket_ready(0, 48)
    g.bucket_ready(48, 64)
    assert [c[0] for c in calls] == [1, 48, 16] and g.buckets == [(0, 48), (48, 64)]


def test_jitter_draws_apart_inside_a_window_and_again_the_same_in_a_replay(pkg):
    def words_of(run):
        with recorded(pkg, keys={'time_jitter': 0.12}) as (rec, model):
            seen = []
            real = pkg.model.mix_seed
            with pytest.MonkeyPatch.context() as mp:
                mp.setattr(pkg.model, 'mix_seed', lambda *w: seen.append(tuple(int(v) for v in w)) or real(*w))
                run(model, *batch(None))
            return seen, model.jitter_seed

    def window(model, x, spk):
        model.accumulate = 2
        for _ in range(4):
            model.train_step(x, spk)
    seen, seed = words_of(window)
    assert seen == [(seed, 0, 0, 0), (seed, 0, 0, 1), (seed, 1, 0, 0), (seed, 1, 0, 1)] and len(set(seen)) == 4

    def voided(model, x, spk):
        model.accumulate = 2
        model.defer_guard = True
        model.x3_void.fill_(1)
        model.train_step(x, spk)
        model.train_step(x, spk)
        model.finish_steps()
    seen, seed = words_of(voided)
    assert seen == [(seed, 0, 0, 0), (seed, 0, 0, 1)] * 2          # first attempts, then the replays

    def plain(model, x, spk):
        model.train_step(x, spk)
        model.train_step(x, spk)
    seen, seed = words_of(plain)
    assert seen == [(seed, 0, 0), (seed, 1, 0)]                    # accumulate = 1: the seed words are what they were


# ------------------------------------------------------------------ refusals
@pytest.mark.parametrize('kind', [None, 'prior'])
def test_refusals_come_before_any_launch(pkg, kind):
    with recorded(pkg, kind) as (rec, model):
        for bad in (0, -1, 2.0, '2', None, True):
            with pytest.raises(ValueError, match='accumulate'):
                model.accumulate = bad
        assert model.accumulate == 1
        model.accumulate = 2
        model.train_step(*batch(kind))
        assert model.accum_index == 1
        del rec.trace[:]
        with pytest.raises(ValueError, match='window'):
            model.accumulate = 3
        with pytest.raises(ValueError, match='window'):
            model.accumulate = 1
        with pytest.raises(ValueError, match='window'):
            model.state_dict()
        with pytest.raises(AttributeError):
            model.accum_index = 0
        assert rec.trace == [] and model.accumulate == 2 and model.accum_index == 1
        model.train_step(*batch(kind))
        sd = model.state_dict()                                   # at a window boundary a checkpoint is what it always was
        assert 'accumulate' not in sd and not any('acc' == k for k in sd)
        model.train_step(*batch(kind))
        assert model.accum_index == 1
        model.load_state_dict(sd)
        assert model.accum_index == 0 and model.global_step == 1
        model.accumulate = 1


def test_codebook_ema_and_accumulate_refuse_each_other(pkg):
    with recorded(pkg, keys={'codebook_ema': 0.99}) as (rec, model):
        with pytest.raises(ValueError, match='codebook_ema'):
            model.accumulate = 2
        assert model.accumulate == 1 and rec.trace == []
    with recorded(pkg) as (rec, model):
        model.accumulate = 2
        with pytest.raises(ValueError, match='accumulate'):
            model.codebook_ema = 0.99
        assert model.codebook_ema == 0.0
        assert [e[0] for e in rec.trace] == ['codebook_ema_constants']      # (a host-side check of the decay: no launch)


@pytest.mark.parametrize('script,args,message', [
    ('train.py', ['-accumulate', '0'], 'error: -accumulate must be an integer >= 1'),
    ('train.py', ['-accumulate', '2', '-codebook_ema', '0.99'], 'error: -accumulate > 1 cannot be combined with -codebook_ema'),
    ('train_prior.py', ['-restore', 'none.pt', '-accumulate', '0'], 'error: -accumulate must be an integer >= 1'),
    ('train_prior.py', ['-restore', 'none.pt', '-accumulate', '2', '-codebook_ema', '0.99'],
     'error: unrecognized arguments: -codebook_ema 0.99'),            # (the prior has no codebook: no such flag there, and -accumulate 2 is none of the unrecognised)
])
def test_command_lines_refuse_before_anything_is_loaded(tmp_path, script, args, message):
    r = subprocess.run([sys.executable, os.path.join(ROOT, script), '-dataset', 'synthetic', '-save', str(tmp_path / 'out' / 'w')] + args,
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and message in r.stderr, r.stderr[-500:]
    assert not (tmp_path / 'out').exists()
