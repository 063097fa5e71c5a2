"""CPU tests of what the wide generator's code-input mode adds outside the kernels: the refusals of `generate.py -count`
(before the package is imported), generate.row_uniforms' stages, the C boundary of vqw_ar_wide_prior_create (declared,
bound, exported, its argument checks with no device present) and the refusals of WidePriorGenerator.sample."""
import ctypes
import importlib.util
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, 'include', 'vqwave.h')

# runs generate.py with a guard on importlib.import_module: importing the package ends the process with status 97
GUARD = '''
import importlib, runpy, sys
_orig = importlib.import_module
def guard(name, *a, **k):
    if 'vq-vae-wavenet_amd' in name:
        sys.stderr.write('THE PACKAGE WAS IMPORTED\\n')
        sys.exit(97)
    return _orig(name, *a, **k)
importlib.import_module = guard
sys.argv = sys.argv[1:]
runpy.run_path(sys.argv[0], run_name='__main__')
'''


def run_cli(tmp_path, extra):
    env = dict(os.environ, HIP_VISIBLE_DEVICES='', CUDA_VISIBLE_DEVICES='')
    return subprocess.run([sys.executable, '-c', GUARD, os.path.join(ROOT, 'generate.py'), '-restore', 'none/weights-1.pt',
                           '-speakers', 'p225'] + extra, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=120)


# ------------------------------------------------------------------ generate.py -count
@pytest.mark.parametrize('extra, match', [
    (['-prior', 'p.pt', '-count', '0'], '-count 0 must be >= 1'),
    (['-prior', 'p.pt', '-count', '-3'], '-count -3 must be >= 1'),
    (['-audio', 'a.wav', '-count', '2'], '-count 2 needs -prior'),
    (['-prior', 'p.pt', '-audio', 'a.wav', '-prompt_frames', '2', '-count', '2'], 'the wide generators have no prefill'),
    (['-prior', 'p.pt', '-count', '2', '-rows', '0'], '-rows 0 must be in 1..1024'),
    (['-prior', 'p.pt', '-count', '2', '-rows', '1025'], '-rows 1025 must be in 1..1024'),
])
def test_count_refuses_bad_flags(tmp_path, extra, match):
    out = run_cli(tmp_path, extra)
    assert out.returncode == 2 and match in out.stderr, (out.returncode, out.stderr[-1000:])


def test_count_passes_its_checks_then_imports_the_package(tmp_path):
    """The guard works: a valid -prior -count 2 reaches the package import (status 97), nothing earlier stops it; so does
    -count 1 with a -rows that only -count > 1 looks at."""
    for extra in (['-prior', 'p.pt', '-count', '2'], ['-prior', 'p.pt', '-count', '2', '-rows', '1024'],
                  ['-prior', 'p.pt', '-rows', '0']):
        out = run_cli(tmp_path, extra)
        assert out.returncode == 97 and 'THE PACKAGE WAS IMPORTED' in out.stderr, (extra, out.returncode, out.stderr[-1000:])


# ------------------------------------------------------------------ row_uniforms
@pytest.fixture(scope='module')
def cli():
    spec = importlib.util.spec_from_file_location('generate_cli', os.path.join(ROOT, 'generate.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def formula(ss, n):
    s = int(ss.generate_state(1, np.uint64)[0] >> np.uint64(1))
    return torch.rand(n, generator=torch.Generator().manual_seed(s))


def test_row_uniforms_stages(cli):
    """Without `stage`: today's SeedSequence([seed, row]) values.  A stage draws from child `stage` of that sequence: numpy
    pads entropy with zeros, so SeedSequence([seed, row, 0]) would BE SeedSequence([seed, row]) and stage 0 could not differ
    from the unstaged draw."""
    SS = np.random.SeedSequence
    assert SS([1, 5, 0]).generate_state(1)[0] == SS([1, 5]).generate_state(1)[0]
    for seed, row in ((1, 0), (1, 5), (7, 300)):
        plain = cli.row_uniforms(seed, row, 100)
        assert torch.equal(plain, formula(SS([seed, row]), 100)), 'the default no longer draws from SeedSequence([seed, row])'
        assert torch.equal(plain, cli.row_uniforms(seed, row, 100, stage=None))
        s0, s1 = cli.row_uniforms(seed, row, 100, stage=0), cli.row_uniforms(seed, row, 100, stage=1)
        kids = SS([seed, row]).spawn(2)
        assert torch.equal(s0, formula(kids[0], 100)) and torch.equal(s1, formula(kids[1], 100))
        assert not torch.equal(s0, plain) and not torch.equal(s1, plain) and not torch.equal(s0, s1)
        assert torch.equal(s0, cli.row_uniforms(seed, row, 100, stage=0)) and torch.equal(s1, cli.row_uniforms(seed, row, 100, stage=1))
        assert s0.dtype == torch.float32 and float(s0.min()) >= 0 and float(s0.max()) < 1
    assert not torch.equal(cli.row_uniforms(1, 0, 100, stage=0), cli.row_uniforms(1, 1, 100, stage=0))
    assert cli.row_uniforms(None, 3, 16, stage=1).shape == (16,)


# ------------------------------------------------------------------ the C boundary
def test_prior_create_is_declared_and_exported(pkg):
    L = pkg._lib
    name = 'vqw_ar_wide_prior_create'
    src = re.sub(r'/\*.*?\*/', '', open(HDR).read(), flags=re.S)
    decl = re.search(r'\bint\s+%s\s*\(([^;]*)\)\s*;' % name, src)
    assert decl, '%s is not declared in vqwave.h' % name
    assert name in L.SIGNATURES, '%s is not declared in _lib.py' % name
    res, args = L.SIGNATURES[name]
    assert res is ctypes.c_int and len(args) == len(decl.group(1).split(',')) == 4
    assert hasattr(L.lib(), name)


def test_prior_create_refuses_arguments_by_name(pkg):
    """Errors are reported, not raised, and name the value; every check comes before the first device call."""
    L = pkg._lib
    lib = L.lib()
    assert lib.vqw_ar_wide_prior_create(None, None, 1, 32) != 0
    assert lib.vqw_last_error().decode() == 'vqw_ar_wide_prior_create: null pointer'

    def weights(**kw):
        w = L.ArWeights()
        w.n_layers, w.kernel_size, w.R, w.S, w.Q, w.Cc, w.pre_k = 2, 3, 32, 64, 32, 16, 3
        for k, v in kw.items():
            setattr(w, k, v)
        return w
    h = ctypes.c_void_p()
    assert lib.vqw_ar_wide_prior_create(None, ctypes.byref(weights()), 1, 32) != 0 and b'null pointer' in lib.vqw_last_error()
    for batch, n_codes, kw, match in [(1025, 32, {}, 'batch=1025'), (0, 32, {}, 'batch=0'), (4, 64, {}, 'n_codes=64 must equal w->Q=32'),
                                      (4, 48, dict(Q=48), 'n_codes=48'), (4, 0, {}, 'n_codes=0'), (4, 1056, dict(Q=1056), 'n_codes=1056'),
                                      (4, 32, dict(R=48), 'R=48'), (4, 32, dict(Cc=24), 'Cc=24'), (4, 32, dict(pre_k=65), 'pre_k=65')]:
        w = weights(**kw)
        assert lib.vqw_ar_wide_prior_create(ctypes.byref(h), ctypes.byref(w), batch, n_codes) != 0
        msg = lib.vqw_last_error().decode()
        assert msg.startswith('vqw_ar_wide_prior_create: ') and match in msg, msg
    assert h.value is None
    # the audio entry point keeps its own name in its messages
    assert lib.vqw_ar_wide_create(ctypes.byref(h), ctypes.byref(weights(Q=256)), 1025) != 0
    assert lib.vqw_last_error().decode().startswith('vqw_ar_wide_create: batch=1025')


# ------------------------------------------------------------------ WidePriorGenerator
def test_wide_prior_generator_refuses_bad_settings(pkg):
    """sampling_settings' refusals reach WidePriorGenerator.sample unchanged, before anything touches the GPU."""
    cls = pkg.generator.WidePriorGenerator
    gen = cls.__new__(cls)
    gen.B, gen.model, gen._h, gen._t = 2, None, None, 0
    cases = [('sample', dict(temperature=0.0)), ('sample', dict(temperature=float('inf'))), ('sample', dict(top_k=-1)),
             ('sample', dict(top_p=0.0)), ('sample', dict(top_p=1.01)), ('sample', dict(temperature=[0.5, 0.5, 0.5])),
             ('greedy', dict(temperature=0.5)), ('greedy', dict(top_k=3)), ('greedy', dict(top_p=0.5))]
    for mode, kw in cases:
        with pytest.raises(ValueError) as want:
            pkg.generator.sampling_settings(2, mode, **kw)
        with pytest.raises(ValueError) as got:
            gen.sample(8, None, mode=mode, **kw)
        assert str(got.value) == str(want.value)
    with pytest.raises(NotImplementedError):
        gen.sample(8, None, mode='beam')
    with pytest.raises(ValueError, match='3 speaker ids for a batch of 2'):
        gen.sample(8, torch.zeros(3, dtype=torch.int64))
    assert not hasattr(gen, 'prefill') and 'no prefill' in cls.__doc__ and 'PriorGenerator.prefill' in cls.__doc__
