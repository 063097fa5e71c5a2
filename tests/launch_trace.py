"""The host's launch sequence as data, recorded on the CPU: what test_launch_trace_cpu.py holds a host-side refactor to.

`install(monkeypatch, pkg)` replaces every public function of the `kernels` module by a recorder and torch.cuda's streams and
events by fakes, so a VQVAE on device='cpu' runs forward() and backward() without a GPU and leaves one entry per call:
    [name, stream, {scalar / list arguments}, {tensor arguments}]
with arguments under their parameter names.  A tensor reads [ordinal of its storage in order of first appearance, storage offset,
numel, dtype]: the role of a buffer, not its address.  Event records, stream waits and grad_sync.bucket_ready ranges are entries
too.  Nothing is computed; the tensors hold whatever torch.empty left in them.

`CASES` are the shapes and switches under which Encoder_64 takes each of its branches (plus the two other encoders), the decoder's
own branches (bf16, the development ladder, the weight-gradient, head and condition switches, a length the plane engine refuses),
the latent prior, train_step around the passes, the forward-only passes (score, decoder_states, encode) and the backward stack at 8
layers (`DEEP`: the chain runs ahead of per-layer weight gradients, batches flush inside the loop); `LAYOUTS` the
configurations whose flat-buffer layout, state_dict and reference names are pinned.  tests/golden/launch_trace.json holds the
SHA-256 of every case's JSON-serialised trace, its call names (for a readable failure; DIGEST_ONLY cases: their number) and the
layout facts (the prior's: their digest).

    python tests/launch_trace.py --write          # make the golden file again (only ever from a commit whose launches are the truth)
    python tests/launch_trace.py --dump CASE      # one case's whole trace as text (or a layout's facts), to diff two commits
"""
import contextlib
import hashlib
import importlib
import inspect
import json
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'launch_trace.json')

# the reference's widths, 2 decoder layers, encoder_filters 256: at B = 1, T = 1024 encoder layer 1 has B * T_out = 256 columns (the
# fp16x3 engine takes it), layers 2..5 are short (split-K)
WAVENET = {'quantization_channels': 256, 'num_cycles': 1, 'num_cycle_layers': 2, 'dilation_rates': [1, 2], 'kernel_size': 3,
           'dilation_filters': 256, 'skip_filters': 512, 'residual_filters': 256, 'preprocess': {'kernel_size': 32, 'filters': 256}}
MODEL = {'encoder': '64', 'use_vq': True, 'speaker_embedding': 64, 'k': 512, 'latent_dim': 64, 'beta': 0.25, 'encoder_filters': 256,
         'learning_rate_schedule': {'0': 8e-5}}
SPEAKERS = 109

PRIOR = dict(WAVENET, quantization_channels=512, speaker_embedding=64, learning_rate_schedule={'0': 1e-4})

# the deep stack: 8 layers in 2 cycles, where the chain runs two layers ahead of the per-layer weight gradients (the ring wait) and a
# weight-gradient batch fills and flushes inside the loop -- what 2 layers never reach
DEEP = dict(num_cycles=2, num_cycle_layers=4, dilation_rates=[1, 2, 4, 8, 1, 2, 4, 8])

# model: keys laid over MODEL (kind 'prior': over PRIOR); wavenet: keys laid over WAVENET (kind 'prior': over PRIOR, under `model`); env: VQW_* switches (every other VQW_* variable is unset); active:
# model._x3_active; grad_sync: with the recording stub; kind: 'prior' = prior.LatentPrior over int32 codes instead of a VQVAE;
# run: what is recorded instead of forward() + backward() -- '_encode': _encode(save=False) on a train=False workspace,
# 'train_step': one immediate train_step, 'score': _score_pass on the score workspace, 'states': decoder_states of a 700-step
# prompt, 'encode': encode() of one utterance for three speakers, 'deferred': defer_guard set (void: the sticky void flag preset, so
# both steps are voided, the older is repeated on the fp32 engine and the second runs again), two train_steps, finish_steps()
CASES = {
    'enc64': dict(),
    'magenta': dict(model={'encoder': 'Magenta'}),
    '2019': dict(model={'encoder': '2019'}, T=1280),
    'enc64-engine-fp32': dict(env={'VQW_ENGINE': 'fp32'}),
    'enc64-fp32-repeat': dict(active=False),
    'enc64-wgrad-pp-0': dict(env={'VQW_WGRAD_PP': '0'}),
    'enc64-enc-x3-0': dict(env={'VQW_ENC_X3': '0'}),
    'enc64-enc-wgrad-x3-0': dict(env={'VQW_ENC_WGRAD_X3': '0'}),
    'enc64-sconv-split-0': dict(env={'VQW_SCONV_SPLIT': '0'}),
    'enc64-overlap-0': dict(env={'VQW_OVERLAP': '0'}),
    'enc64-encode-nosave': dict(run='_encode'),
    'enc64-grad-sync': dict(grad_sync=True),
    # 768 filters: layer 1 has 12 x 8 x 8 = 768 blocks of 64 x 128 (more than 2 per CU: one unsplit conv_gemm, forward and input
    # gradient), layer 2 has 384 (split in two) -- VQVAE / Encoder64 _short_layer_split
    'enc64-unsplit': dict(model={'encoder_filters': 768}, env={'VQW_ENGINE': 'fp32'}, B=8, T=4096),
}
# ... and the cases of which the golden file holds the digest and the number of entries alone, no list of call names (--dump prints a
# trace): the file stays small enough to read
DIGEST_ONLY = {
    # the decoder's own branches
    'dec-bf16': dict(env={'VQW_DTYPE': 'bf16'}),
    **{'dec-ladder-%d' % n: dict(env={'VQW_GATE_F16X3': str(n)}) for n in (1, 2, 3, 4, 5)},
    'dec-wgrad-batch-0': dict(env={'VQW_WGRAD_BATCH': '0'}),
    'dec-wgrad-x3-0': dict(env={'VQW_WGRAD_X3': '0'}),
    'dec-head-x3-0': dict(env={'VQW_HEAD_X3': '0'}),
    'dec-wgrad-qp-0': dict(env={'VQW_WGRAD_QP': '0'}),
    'dec-save-tanh-1': dict(env={'VQW_SAVE_TANH': '1'}),
    'dec-cond-proj-0': dict(env={'VQW_COND_PROJ': '0'}),
    'dec-skip-groups-2': dict(env={'VQW_SKIP_GROUPS': '2'}),
    'dec-novq-onehot': dict(model={'use_vq': False, 'speaker_embedding': 0}),
    'dec-refused-length': dict(T=1088),      # no multiple of 256: the fp32-MFMA engine, with the one-line notice
    'dec-refused-length-enc-x3-0': dict(T=1088, env={'VQW_ENC_X3': '0'}),     # ... and the encoder's engine layers off: no plane kernel is left
    # the latent prior
    'prior': dict(kind='prior'),
    'prior-engine-fp32': dict(kind='prior', env={'VQW_ENGINE': 'fp32'}),
    'prior-train-step': dict(kind='prior', run='train_step'),
    'prior-score': dict(kind='prior', run='score'),
    # the step around the passes (guard-scale update, the codebook's own update, Adam + EMA), the forward-only passes
    'train-step': dict(run='train_step'),
    'train-step-jitter-ema': dict(run='train_step', model={'time_jitter': 0.12, 'codebook_ema': 0.99, 'codebook_restart': 0.5}),
    'score': dict(run='score'),
    'states': dict(run='states'),
    'encode': dict(run='encode'),
    # the deferred range flag: two steps and their resolution; with the void flag preset, the whole replay path
    'train-step-deferred': dict(run='deferred'),
    'train-step-deferred-flagged': dict(run='deferred', void=True),
    # the backward stack at 8 layers (DEEP), under every switch that changes its route, buffers or weight-gradient schedule
    'deep': dict(wavenet=DEEP),
    'deep-wg-batches-2-3': dict(wavenet=DEEP, env={'VQW_WG_GATE_BATCH': '2', 'VQW_WG_RES_BATCH': '3'}),     # batches flush inside the loop
    'deep-wgrad-batch-0': dict(wavenet=DEEP, env={'VQW_WGRAD_BATCH': '0'}),                                # per layer: the rings and their waits
    'deep-wgrad-batch-0-overlap-0': dict(wavenet=DEEP, env={'VQW_WGRAD_BATCH': '0', 'VQW_OVERLAP': '0'}),
    'deep-overlap-0': dict(wavenet=DEEP, env={'VQW_OVERLAP': '0'}),
    'deep-wgrad-x3-0': dict(wavenet=DEEP, env={'VQW_WGRAD_X3': '0'}),
    'deep-wgrad-qp-0': dict(wavenet=DEEP, env={'VQW_WGRAD_QP': '0'}),
    'deep-wgrad-pp-0': dict(wavenet=DEEP, env={'VQW_WGRAD_PP': '0'}),
    'deep-engine-fp32': dict(wavenet=DEEP, env={'VQW_ENGINE': 'fp32'}),
    'deep-fp32-repeat': dict(wavenet=DEEP, active=False),
    'deep-bf16': dict(wavenet=DEEP, env={'VQW_DTYPE': 'bf16'}),
    'deep-ladder-4': dict(wavenet=DEEP, env={'VQW_GATE_F16X3': '4'}),
    'deep-ladder-5': dict(wavenet=DEEP, env={'VQW_GATE_F16X3': '5'}),
    'deep-save-tanh-1': dict(wavenet=DEEP, env={'VQW_SAVE_TANH': '1'}),
    'deep-save-gated-1': dict(wavenet=DEEP, env={'VQW_SAVE_GATED': '1'}),
    'deep-head-x3-0': dict(wavenet=DEEP, env={'VQW_HEAD_X3': '0'}),
    'deep-grad-sync': dict(wavenet=DEEP, grad_sync=True),
    'deep-prior': dict(wavenet=DEEP, kind='prior'),
    'deep-refused-length': dict(wavenet=DEEP, T=1088),
}
CASES.update(DIGEST_ONLY)
LAYOUTS = {'%s-vq%d-spk%d' % (enc, vq, spk): {'encoder': enc, 'use_vq': bool(vq), 'speaker_embedding': spk}
           for enc in ('64', 'Magenta', '2019') for vq in (1, 0) for spk in (64, 0)}
LAYOUTS.update({'prior-spk%d' % spk: {'kind': 'prior', 'speaker_embedding': spk} for spk in (64, 0)})      # (golden: the facts' digest alone)


class Recorder:
    def __init__(self):
        self.trace, self.storages, self.keep = [], {}, []
        self.main = FakeStream(self, 'main')
        self.current, self.n_side, self.n_event = self.main, 0, 0

    def tensor(self, t):
        key = t.untyped_storage().data_ptr()
        if key not in self.storages:
            self.storages[key] = len(self.storages)
            self.keep.append(t)          # (alive until the case ends: no later storage gets this address)
        return ['tensor', self.storages[key], t.storage_offset(), t.numel(), str(t.dtype)]

    def describe(self, v):
        """(JSON value, holds a tensor)"""
        if torch.is_tensor(v):
            return self.tensor(v), True
        if isinstance(v, dict):
            items = {str(k): self.describe(x) for k, x in v.items()}
            return {k: d for k, (d, _) in items.items()}, any(h for _, h in items.values())
        if isinstance(v, (list, tuple)):
            items = [self.describe(x) for x in v]
            return [d for d, _ in items], any(h for _, h in items)
        if v is None or isinstance(v, (bool, int, float, str)):
            return v, False
        return repr(type(v)), False

    def add(self, name, args):
        scalars, tensors = {}, {}
        for k, v in args.items():
            d, has = self.describe(v)
            (tensors if has else scalars)[k] = d
        self.trace.append([name, self.current.name, scalars, tensors])

    def wrap(self, name, fn, result=None):
        sig = inspect.signature(fn)
        var_kw = [p.name for p in sig.parameters.values() if p.kind is p.VAR_KEYWORD]

        def recorded(*a, **kw):
            args = dict(sig.bind(*a, **kw).arguments)
            for k in var_kw:
                args.update(args.pop(k, {}))
            self.add(name, args)
            return result(*a, **kw) if result else None
        return recorded


class FakeStream:
    def __init__(self, rec, name):
        self.rec, self.name = rec, name

    def wait_event(self, ev):
        self.rec.trace.append(['wait_event', self.name, {'event': ev.n}, {}])

    def wait_stream(self, other):
        self.rec.trace.append(['wait_stream', self.name, {'stream': other.name}, {}])


class FakeEvent:
    def __init__(self, rec):
        self.rec, self.n = rec, rec.n_event
        rec.n_event += 1

    def record(self, stream=None):
        self.rec.trace.append(['record', (stream or self.rec.current).name, {'event': self.n}, {}])

    def synchronize(self):
        pass


class GradSyncStub:
    """parallel.GradAllReduce as far as a single-process backward pass uses it: the ranges it is told are final."""
    rank, world, active = 0, 1, False

    def __init__(self, rec):
        self.rec = rec

    def bucket_ready(self, lo, hi):
        self.rec.trace.append(['grad_sync.bucket_ready', self.rec.current.name, {'lo': int(lo), 'hi': int(hi)}, {}])


def install(monkeypatch, pkg):
    """Put the recorder in place of pkg.kernels' public functions and torch.cuda's streams / events; returns it."""
    rec, K = Recorder(), pkg.kernels
    results = {'cond_proj_dgrad_scratch': lambda *a, **kw: 4096,
               'prior_code_buckets': lambda codes, k: (torch.zeros(codes.numel(), dtype=torch.int32), torch.zeros(k + 1, dtype=torch.int32))}
    for name, fn in vars(K).items():
        if inspect.isfunction(fn) and fn.__module__ == K.__name__ and not name.startswith('_'):
            monkeypatch.setattr(K, name, rec.wrap(name, fn, results.get(name)))

    def side_stream(*a, **kw):
        rec.n_side += 1
        return FakeStream(rec, 'side%d' % rec.n_side)

    @contextlib.contextmanager
    def on_stream(s):
        prev, rec.current = rec.current, s
        try:
            yield
        finally:
            rec.current = prev
    monkeypatch.setattr(torch.cuda, 'current_stream', lambda *a, **kw: rec.current)
    monkeypatch.setattr(torch.cuda, 'Stream', side_stream)
    monkeypatch.setattr(torch.cuda, 'Event', lambda *a, **kw: FakeEvent(rec))
    monkeypatch.setattr(torch.cuda, 'stream', on_stream)
    monkeypatch.setattr(torch.cuda, 'get_device_properties', lambda *a, **kw: types.SimpleNamespace(multi_processor_count=256))
    monkeypatch.setattr(torch.Tensor, 'pin_memory', lambda self, *a, **kw: self)      # (the deferred step's host copy of the void flag)
    return rec


def set_switches(monkeypatch, env):
    for k in [k for k in os.environ if k.startswith('VQW_')]:
        monkeypatch.delenv(k)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def make_model(pkg, kind, keys, wavenet=None):
    """A fresh model on the CPU: a VQVAE of MODEL / WAVENET, or (kind 'prior') a LatentPrior of PRIOR, with `keys` (and `wavenet`) laid over."""
    if kind == 'prior':
        return pkg.prior.LatentPrior(dict(PRIOR, **dict(wavenet or {}, **keys)), SPEAKERS, device='cpu')
    return pkg.model.VQVAE(dict(MODEL, **keys), dict(WAVENET, **(wavenet or {})), SPEAKERS, device='cpu', seed=0)


def run_case(monkeypatch, pkg, name):
    """The trace of CASES[name]: a fresh model under the case's switches, then forward() + backward() (or what the case's `run` names)."""
    case = CASES[name]
    set_switches(monkeypatch, case.get('env', {}))
    rec = install(monkeypatch, pkg)
    prior, run = case.get('kind') == 'prior', case.get('run')
    model = make_model(pkg, case.get('kind'), case.get('model', {}), case.get('wavenet'))
    model._x3_active = case.get('active', True)
    if case.get('grad_sync'):
        model.grad_sync = GradSyncStub(rec)
    B, T = case.get('B', 1), case.get('T', 1024)
    x, spk = torch.zeros(B, T, dtype=torch.int32 if prior else torch.float32), torch.zeros(B, dtype=torch.int64)
    del rec.trace[:]                     # (what the constructor checked its settings with)
    if run == '_encode':
        model._encode(x, spk, model._workspace(B, T, train=False), save=False)
    elif run == 'train_step':
        model.train_step(x, spk)
    elif run == 'score':
        model._score_pass(x, spk, model._workspace(B, T, 'score'))
    elif run == 'states':
        model.decoder_states(x, torch.zeros(B, model.Cc, T // 64), 700, lambda l, net_l, s0: None)
    elif run == 'encode':
        model.encode(x, torch.zeros(3, dtype=torch.int64))
    elif run == 'deferred':
        model.defer_guard = True
        if case.get('void'):
            model.x3_void.fill_(1)
        model.train_step(x, spk)
        model.train_step(x, spk)
        model.finish_steps()
    else:
        model.backward(x, spk, model.forward(x, spk))
    return rec.trace


def digest(trace):
    return hashlib.sha256(json.dumps(trace, sort_keys=True, separators=(',', ':')).encode()).hexdigest()


def layout_facts(monkeypatch, pkg, name):
    """What checkpoints and the grad_sync bucket ranges depend on: segments with offsets, state_dict, reference names
    (a zero-length tensor holds nothing and is no part of them)."""
    set_switches(monkeypatch, {})
    keys = dict(LAYOUTS[name])
    model = make_model(pkg, keys.pop('kind', None), keys)
    shapes = lambda d: [[k, list(v.shape)] for k, v in d.items() if v.numel()]                      # noqa: E731
    return {'segments': [[n, off, list(shp)] for n, (off, shp) in model.seg_off.items()], 'n_flat': model.n_flat,
            'state_dict': shapes(model.state_dict()), 'named_parameters': shapes(model.named_parameters()),
            'named_parameters_ema': shapes(model.named_parameters(ema=True)), 'named_gradients': shapes(model.named_gradients())}


def as_text(trace):
    return '\n'.join(json.dumps(e, sort_keys=True) for e in trace)


def main(argv):
    import pytest
    sys.path.insert(0, os.path.dirname(HERE))
    pkg = importlib.import_module('vq-vae-wavenet_amd')
    if argv[:1] == ['--dump'] and len(argv) == 2 and (argv[1] in CASES or argv[1] in LAYOUTS):
        with pytest.MonkeyPatch.context() as mp:
            print(as_text(run_case(mp, pkg, argv[1])) if argv[1] in CASES else json.dumps(layout_facts(mp, pkg, argv[1]), indent=1))
        return 0
    if argv != ['--write']:
        print(__doc__)
        return 2
    golden = {'cases': {}, 'layouts': {}}
    for name in CASES:
        with pytest.MonkeyPatch.context() as mp:
            trace = run_case(mp, pkg, name)
        golden['cases'][name] = dict({'sha256': digest(trace)}, **({'entries': len(trace)} if name in DIGEST_ONLY else {'calls': [e[0] for e in trace]}))
        print('%-24s %4d entries  %s' % (name, len(trace), golden['cases'][name]['sha256'][:16]))
    for name in LAYOUTS:
        with pytest.MonkeyPatch.context() as mp:
            facts = layout_facts(mp, pkg, name)
        golden['layouts'][name] = {'sha256': digest(facts)} if 'kind' in LAYOUTS[name] else facts
    with open(GOLDEN, 'w') as f:
        json.dump(golden, f, indent=0, sort_keys=True)
        f.write('\n')
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
