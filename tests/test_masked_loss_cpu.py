"""CPU tests of length-masked prior training: the float64 restatement pinned against itself (padded batch with a
mask == every row run alone: the padding cannot matter), the ranged loss reference against torch, the host logic of
train_step(lengths=) through the launch recorder, the whole-utterance sources and the generalised Prefetcher, and the flag
refusals of train_prior.py."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import launch_trace as LT  # noqa: E402
import masked_ref as MR  # noqa: E402
import pointwise_ref as PR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tiny_prior(k=32, pre_k=3):
    return {"quantization_channels": k, "num_cycles": 2, "num_cycle_layers": 4, "dilation_rates": [1, 2, 4, 8, 1, 2, 4, 8],
            "kernel_size": 3, "dilation_filters": 32, "skip_filters": 64, "residual_filters": 32,
            "preprocess": {"kernel_size": pre_k, "filters": 32}, "speaker_embedding": 16, "learning_rate_schedule": {"0": 1e-3}}


# ---------------------------------------------------------------------------------------------------- the restatement
def test_padding_cannot_matter_in_the_restatement(pkg):
    """(a) the padded batch with a mask and (b) the sum over rows run alone agree to 1e-12 in the loss and in every gradient,
    with RANDOM codes in the padding; and changing the padding changes nothing at all."""
    cfg = tiny_prior()
    prior = pkg.prior.LatentPrior(cfg, 10, device='cpu', seed=0)
    P = MR.random_params(prior.named_parameters(), 7)
    B, T, lengths = 3, 256, (256, 193, 64)
    g = torch.Generator().manual_seed(5)
    codes = torch.randint(0, 32, (B, T), generator=g)           # (the padding holds random codes too)
    spk = torch.tensor([3, 8, 0])
    la, ga = MR.loss_and_grads(MR.padded_loss, codes, spk, lengths, P, cfg)
    lb, gb = MR.loss_and_grads(MR.rowwise_loss, codes, spk, lengths, P, cfg)
    assert abs(la - lb) <= 1e-12 * abs(lb)
    assert set(ga) == set(gb) == set(P)
    for n in P:
        scale = float(gb[n].abs().max())
        assert float((ga[n] - gb[n]).abs().max()) <= 1e-12 * max(scale, 1e-300), n
    assert any(float(v.abs().max()) > 0 for v in ga.values())
    other = codes.clone()
    for b, n in enumerate(lengths):
        other[b, n:] = torch.randint(0, 32, (T - n,), generator=g)
    assert not torch.equal(other, codes)
    lc, gc = MR.loss_and_grads(MR.padded_loss, other, spk, lengths, P, cfg)
    assert abs(lc - la) <= 1e-12 * abs(la)
    for n in P:
        assert float((gc[n] - ga[n]).abs().max()) <= 1e-12 * max(float(ga[n].abs().max()), 1e-300), n
    # ... and the mask is not vacuous: the unmasked mean is another number
    full, _ = MR.loss_and_grads(MR.padded_loss, codes, spk, (T,) * B, P, cfg)
    assert abs(full - la) > 1e-6


@pytest.mark.parametrize('Q,T', [(4, 1), (68, 65), (256, 200)])
def test_xent_ranged_ref_is_cross_entropy_times_the_mask(Q, T):
    B = 4
    x = PR.randn(PR.seed_of('ranged-ref', Q, T), B, Q, T) * np.float32(3.0)
    lab = np.random.RandomState(Q + T).randint(0, Q, (B, T)).astype(np.int32)
    tb, te = [0, 1, 64, 5], [T, T - 1, 65, 3]
    gs = 0.25
    ref = MR.xent_ranged_ref(x, lab, gs, tb, te)
    mask = torch.from_numpy(ref['mask'])
    want_mask = np.array([[min(max(tb[b], 0), T) <= t < min(max(te[b], 0), T) for t in range(T)] for b in range(B)])
    assert np.array_equal(ref['mask'], want_mask) and not ref['mask'][3].any()
    xt = torch.from_numpy(x).double().requires_grad_(True)
    ce = Fn.cross_entropy(xt, torch.from_numpy(lab).long(), reduction='none') * mask
    np.testing.assert_allclose(ref['loss'], ce.detach().numpy(), rtol=1e-12, atol=1e-12)
    (ce.sum() * gs).backward()
    np.testing.assert_allclose(ref['d'], xt.grad.numpy(), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(ref['p'], (torch.softmax(xt.detach(), 1) * mask[:, None, :]).numpy(), rtol=1e-12, atol=1e-300)
    # what lies outside the ranges may be anything
    nan = np.where(ref['mask'][:, None, :], x, np.float32('nan'))
    again = MR.xent_ranged_ref(nan, lab, gs, tb, te)
    for name in ('p', 'd', 'loss'):
        assert np.array_equal(again[name], ref[name])
    bars = MR.xent_ranged_bars(ref, lab, gs)
    assert (bars['p'][~np.broadcast_to(ref['mask'][:, None, :], x.shape)] == 0).all() and bars['loss_sum'] > 0
    # None: 0 / T
    assert MR.range_mask(2, 5).all() and np.array_equal(MR.range_mask(2, 5, None, [2, 9]).sum(1), [2, 5])


# ---------------------------------------------------------------------------------------------------- host logic, recorded
def _prior_trace(monkeypatch, pkg, lengths, B=2, T=1024):
    LT.set_switches(monkeypatch, {})
    rec = LT.install(monkeypatch, pkg)
    model = LT.make_model(pkg, 'prior', {})
    codes, spk = torch.zeros(B, T, dtype=torch.int32), torch.zeros(B, dtype=torch.int64)
    del rec.trace[:]
    ws = model.train_step(codes, spk) if lengths is None else model.train_step(codes, spk, lengths=lengths)
    return copy.deepcopy(rec.trace), ws, model


def _renumbered(trace, drop=()):
    """The trace with the tensor arguments named in `drop` removed and the storage ordinals numbered again in order of first
    appearance: two traces that differ by one extra tensor argument then read the same everywhere else."""
    seen, out = {}, []

    def walk(v):
        if isinstance(v, list) and len(v) == 5 and v[0] == 'tensor':
            return ['tensor', seen.setdefault(v[1], len(seen))] + v[2:]
        if isinstance(v, list):
            return [walk(x) for x in v]
        if isinstance(v, dict):
            return {k: walk(x) for k, x in v.items()}
        return v
    for name, stream, scalars, tensors in trace:
        out.append([name, stream, scalars, walk({k: v for k, v in tensors.items() if k not in drop})])
    return out


def test_train_step_with_lengths_swaps_the_loss_launch_and_nothing_else(pkg):
    with pytest.MonkeyPatch.context() as mp:
        plain, _, _ = _prior_trace(mp, pkg, None)
    with pytest.MonkeyPatch.context() as mp:
        lengths = [1024, 300]
        masked, ws, model = _prior_trace(mp, pkg, lengths)
    assert ws['count'] == 1324
    assert len(plain) == len(masked)
    a, b = _renumbered(plain), _renumbered(masked, drop=('t_end',))
    at = [i for i, e in enumerate(a) if e[0] == 'softmax_xent']
    assert len(at) == 1 and not any(e[0] == 'softmax_xent_ranged' for e in a)
    i = at[0]
    assert a[:i] == b[:i] and a[i + 1:] == b[i + 1:]
    name, stream, scalars, tensors = b[i]
    assert name == 'softmax_xent_ranged' and stream == a[i][1] and tensors == a[i][3]
    assert scalars['grad_scale'] == 1.0 / sum(lengths) and a[i][2]['grad_scale'] == 1.0 / (2 * 1024)
    assert {k: v for k, v in scalars.items() if k != 'grad_scale'} == {k: v for k, v in a[i][2].items() if k != 'grad_scale'}
    assert 't_begin' not in scalars and 't_begin' not in masked[i][3]       # (rows start at 0)
    t_end = masked[i][3]['t_end']
    assert t_end[2:] == [0, 2, 'torch.int32']


def test_train_step_without_lengths_is_the_golden_trace(pkg):
    import json
    with open(LT.GOLDEN) as f:
        golden = json.load(f)['cases']['prior-train-step']
    with pytest.MonkeyPatch.context() as mp:
        LT.set_switches(mp, {})
        trace = LT.run_case(mp, pkg, 'prior-train-step')
    assert LT.digest(trace) == golden['sha256'] and len(trace) == golden['entries']
    with pytest.MonkeyPatch.context() as mp:
        again, ws, _ = _prior_trace(mp, pkg, None, B=1)
    assert LT.digest(again) == golden['sha256'] and ws['count'] == 1024


def test_lengths_are_refused_before_any_launch(pkg):
    with pytest.MonkeyPatch.context() as mp:
        LT.set_switches(mp, {})
        rec = LT.install(mp, pkg)
        prior = LT.make_model(pkg, 'prior', {})
        vqvae = LT.make_model(pkg, None, {})
        codes, spk = torch.zeros(2, 1024, dtype=torch.int32), torch.zeros(2, dtype=torch.int64)
        del rec.trace[:]
        for bad, match in (([1024], '1 lengths for a batch of 2'), ([1024, 1024, 5], '3 lengths'), ([0, 1024], 'positive'),
                           ([1024, 1025], 'at most T = 1024'), (torch.tensor([-3, 7]), 'positive')):
            for call in (prior.train_step, prior.forward, prior.forward_checked):
                with pytest.raises(ValueError, match=match):
                    call(codes, spk, lengths=bad)
        with pytest.raises(NotImplementedError, match='VQ-VAE does not train on lengths'):
            vqvae.train_step(torch.zeros(2, 1024), spk, lengths=[1024, 512])
        prior.grad_sync = LT.GradSyncStub(rec)
        prior.grad_sync.active = True
        with pytest.raises(NotImplementedError, match='grad_sync'):
            prior.train_step(codes, spk, lengths=[1024, 512])
        assert rec.trace == [] and prior.global_step == 0 and vqvae.global_step == 0
        prior.grad_sync = None
        prior.train_step(codes, spk, lengths=torch.tensor([1024, 1], dtype=torch.int32))      # a CPU tensor; the prior's unit is one code
        assert prior.global_step == 1 and any(e[0] == 'softmax_xent_ranged' for e in rec.trace)


# ---------------------------------------------------------------------------------------------------- the sources
def _corpus(tmp_path, T):
    """Three speakers' WAVs: short (2.5 units), tiny (under min_len), long (3 T + 17 samples), exact (T samples)."""
    from scipy.io import wavfile
    rng = np.random.RandomState(3)
    sizes = {'a/short.wav': 160, 'b/tiny.wav': 100, 'c/long.wav': 3 * T + 17, 'a/exact.wav': T}
    wavs = {}
    for rel, n in sizes.items():
        os.makedirs(os.path.join(tmp_path, os.path.dirname(rel)), exist_ok=True)
        pcm = rng.randint(-20000, 20000, n).astype(np.int16)
        pcm[pcm == 0] = 1
        wavfile.write(os.path.join(tmp_path, rel), 16000, pcm)
        wavs[rel] = ((pcm.astype(np.float32) + 0.5) / 32767.5).astype(np.float32)
    with open(os.path.join(tmp_path, 'list.txt'), 'w') as f:
        f.write('\n'.join(sizes) + '\n')
    with open(os.path.join(tmp_path, 'speakers.txt'), 'w') as f:
        f.write('a, 0\nb, 1\nc, 2\n')
    return wavs


def test_whole_utterance_source(pkg, tmp_path):
    D, T = pkg.data, 512
    wavs = _corpus(str(tmp_path), T)
    mk = lambda **kw: D.WavDataset(4, T, str(tmp_path), 'list.txt', 'speakers.txt', device='cpu', seed=1, **kw)     # noqa: E731
    src = mk(whole=True, unit=64, min_len=128)
    seen = set()
    for _ in range(12):
        x, spk, lengths = src.next_host()
        assert x.dtype == torch.float32 and tuple(x.shape) == (4, T) and spk.dtype == torch.int64 and lengths.dtype == torch.int32
        for row, s, n in zip(x.numpy(), spk.tolist(), lengths.tolist()):
            assert s != 1, 'a file under min_len was served'
            assert n % 64 == 0 and 128 <= n <= T and (row[n:] == 0).all()
            if n == 128:        # short.wav: whole, from its first sample, trimmed to 2 units
                assert s == 0 and np.array_equal(row[:n], wavs['a/short.wav'][:128])
                seen.add('short')
            elif s == 2:        # long.wav: a window of T samples somewhere inside it
                w = wavs['c/long.wav']
                assert n == T and any(np.array_equal(row, w[i:i + T]) for i in np.flatnonzero(w[:len(w) - T + 1] == row[0]))
                seen.add('long')
            else:               # exact.wav: T samples, whole
                assert s == 0 and n == T and np.array_equal(row, wavs['a/exact.wav'])
                seen.add('exact')
    assert seen == {'short', 'long', 'exact'}
    # the same seed discipline as WavDataset, and nothing changes when the option is off
    a, b = mk(whole=True, min_len=128).next_host(), mk(whole=True, min_len=128).next_host()
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    off = mk().next_host()
    assert len(off) == 2 and tuple(off[0].shape) == (4, T)
    with pytest.raises(ValueError, match='min_len'):
        mk(min_len=128)
    with pytest.raises(ValueError, match='min_len'):
        mk(whole=True, min_len=T + 1)
    # Synthetic: the same audio with the option on, cut to random lengths from a generator of its own
    plain = D.Synthetic(3, T, seed=9, device='cpu').next_host()
    x, spk, lengths = D.Synthetic(3, T, seed=9, device='cpu', whole=True, unit=64, min_len=128).next_host()
    assert len(plain) == 2 and torch.equal(spk, plain[1]) and lengths.dtype == torch.int32
    for b, n in enumerate(lengths.tolist()):
        assert n % 64 == 0 and 128 <= n <= T and torch.equal(x[b, :n], plain[0][b, :n]) and not x[b, n:].any()


class _Counting:
    num_speakers = 5

    def __init__(self, with_lengths):
        self.n, self.with_lengths = 0, with_lengths

    def next_host(self):
        self.n += 1
        out = (torch.full((2, 8), float(self.n)), torch.full((2,), self.n, dtype=torch.int64))
        return out + ((torch.tensor([self.n, 8], dtype=torch.int32),) if self.with_lengths else ())


def test_prefetcher_carries_two_and_three_element_batches(pkg):
    for with_lengths in (False, True):
        pf = pkg.data.Prefetcher(_Counting(with_lengths), depth=3, device='cpu')
        try:
            kept = []
            for i in range(1, 8):        # past the depth: slots are reused
                out = pf.next()
                assert len(out) == (3 if with_lengths else 2)
                assert float(out[0][0, 0]) == i and int(out[1][0]) == i
                if with_lengths:
                    assert out[2].device.type == 'cpu' and out[2].dtype == torch.int32 and out[2].tolist() == [i, 8]
                    kept.append(out[2])
            assert [t.tolist()[0] for t in kept] == list(range(1, 8)[:len(kept)])       # a handed-out lengths tensor is the caller's own
            assert pf.num_speakers == 5 and pf.served == 7
        finally:
            pf.close()


# ---------------------------------------------------------------------------------------------------- command line
def _cli(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, 'train_prior.py')] + list(args), capture_output=True, text=True, timeout=120,
                          env=dict(os.environ, PYTHONPATH=ROOT))


def test_cli_help_shows_the_new_flags():
    out = _cli('-h')
    assert out.returncode == 0
    for flag in ('-whole_utterances', '-min_frames', '-eval_list', '-eval_interval', '-eval_batches'):
        assert flag in out.stdout, flag


@pytest.mark.parametrize('args,match', [
    (['-min_frames', '8'], '-min_frames needs -whole_utterances'),
    (['-whole_utterances', '-min_frames', '0'], '-min_frames must be in 1..-length'),
    (['-whole_utterances', '-length', '128', '-min_frames', '129'], '-min_frames must be in 1..-length = 128'),
    (['-eval_interval', '5'], '-eval_interval needs -eval_list'),
    (['-eval_list', 'no/such/list.txt', '-eval_interval', '5'], 'no such file'),
])
def test_cli_refuses_bad_flags_before_anything_is_loaded(args, match):
    out = _cli('-restore', 'no/such/weights.pt', *args)        # (a missing checkpoint would fail much later)
    assert out.returncode == 2 and match in out.stderr, out.stderr[-500:]
