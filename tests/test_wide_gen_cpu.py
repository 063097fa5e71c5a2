"""CPU tests of what the wide generator adds outside the kernels: generator.plan_rows, the refusals of
`generate.py -audio_list` (before the package is imported) and of WideGenerator.generate, and the C boundary (the five
vqw_ar_wide_* entry points, the struct they share with the other generators, the shapes refused at creation)."""
import ctypes
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, 'include', 'vqwave.h')
WIDE = ['vqw_ar_wide_create', 'vqw_ar_wide_reset', 'vqw_ar_wide_run_async', 'vqw_ar_wide_wait', 'vqw_ar_wide_destroy']


# ------------------------------------------------------------------ plan_rows
def check_plan(plan_rows, lengths, max_rows):
    batches, padded = plan_rows(lengths, max_rows)
    flat = [i for b in batches for i in b]
    assert sorted(flat) == list(range(len(lengths))), 'every row in exactly one batch'
    assert all(1 <= len(b) <= max_rows for b in batches)
    by_len = [lengths[i] for i in flat]
    assert by_len == sorted(by_len), 'batches, and the rows of each, in ascending length'
    assert padded == sum(max(lengths[i] for i in b) - lengths[i] for b in batches for i in b)
    assert len(batches) == -(-len(lengths) // max_rows)
    return batches, padded


def test_plan_rows(pkg):
    plan = pkg.generator.plan_rows
    rnd = random.Random(3)
    for _ in range(50):
        n = rnd.randint(1, 60)
        check_plan(plan, [512 * rnd.randint(1, 40) for _ in range(n)], rnd.randint(1, 17))
    assert check_plan(plan, [1024], 256) == ([[0]], 0)                       # one row
    assert check_plan(plan, [512] * 7, 3)[1] == 0                            # all equal: no padding
    assert check_plan(plan, [1536, 512, 1024], 1) == ([[1], [2], [0]], 0)    # one row per batch
    assert check_plan(plan, [1536, 512, 1024], 2) == ([[1, 2], [0]], 512)
    assert plan([], 4) == ([], 0)
    assert plan(np.array([512, 512]), 1024) == ([[0, 1]], 0)
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError):
            plan([512], bad)


# ------------------------------------------------------------------ generate.py -audio_list
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


def write_wav(path, n):
    from scipy.io import wavfile
    wavfile.write(str(path), 16000, (np.sin(np.arange(n) * 0.05) * 8000).astype(np.int16))


def run_cli(tmp_path, extra):
    env = dict(os.environ, HIP_VISIBLE_DEVICES='', CUDA_VISIBLE_DEVICES='')
    return subprocess.run([sys.executable, '-c', GUARD, os.path.join(ROOT, 'generate.py'), '-restore', 'none/weights-1.pt',
                           '-speakers', 'p225'] + extra, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize('extra, match', [
    (['-audio', 'a.wav'], 'not with -audio'),
    (['-prior', 'p.pt'], 'not with -prior'),
    (['-prompt_samples', '64'], 'not with -prompt_samples'),
    (['-prompt_frames', '2'], 'not with -prompt_frames'),
    (['-teacher_forced'], 'not with -teacher_forced'),
    (['-rows', '0'], '-rows 0 must be in 1..1024'),
    (['-rows', '1025'], '-rows 1025 must be in 1..1024'),
])
def test_audio_list_refuses_bad_flags(tmp_path, extra, match):
    write_wav(tmp_path / 'a.wav', 2048)
    (tmp_path / 'list.txt').write_text('a.wav\n')
    out = run_cli(tmp_path, ['-audio_list', 'list.txt'] + extra)
    assert out.returncode == 2 and match in out.stderr, (out.returncode, out.stderr[-1000:])


def test_audio_list_refuses_empty_and_short(tmp_path):
    (tmp_path / 'empty.txt').write_text('\n# nothing here\n\n')
    out = run_cli(tmp_path, ['-audio_list', 'empty.txt'])
    assert out.returncode == 2 and 'names no utterance' in out.stderr, (out.returncode, out.stderr[-1000:])
    write_wav(tmp_path / 'ok.wav', 2048)
    (tmp_path / 'sub').mkdir()
    write_wav(tmp_path / 'sub' / 'short.wav', 511)
    (tmp_path / 'list.txt').write_text('ok.wav\nsub/short.wav\n')
    out = run_cli(tmp_path, ['-audio_list', 'list.txt'])
    assert out.returncode == 2 and 'short.wav is shorter than 512 samples' in out.stderr, (out.returncode, out.stderr[-1000:])
    (tmp_path / 'gone.txt').write_text('nowhere.wav\n')
    out = run_cli(tmp_path, ['-audio_list', 'gone.txt', '-data_root', 'sub'])
    assert out.returncode == 2 and os.path.join('sub', 'nowhere.wav') in out.stderr, (out.returncode, out.stderr[-1000:])


def test_audio_list_passes_its_checks_then_imports_the_package(tmp_path):
    """The guard works: a list that passes every check reaches the package import (status 97), nothing earlier stops it."""
    write_wav(tmp_path / 'a.wav', 2048)
    (tmp_path / 'list.txt').write_text('a.wav\n')
    out = run_cli(tmp_path, ['-audio_list', 'list.txt', '-rows', '1024'])
    assert out.returncode == 97 and 'THE PACKAGE WAS IMPORTED' in out.stderr, (out.returncode, out.stderr[-1000:])


def test_wide_generator_refuses_bad_settings(pkg):
    """sampling_settings' refusals reach WideGenerator.generate unchanged, before anything touches the GPU."""
    gen = pkg.generator.WideGenerator.__new__(pkg.generator.WideGenerator)
    gen.B, gen.model, gen._h = 2, None, None
    cases = [('sample', dict(temperature=0.0)), ('sample', dict(temperature=float('inf'))), ('sample', dict(top_k=-1)),
             ('sample', dict(top_p=0.0)), ('sample', dict(top_p=1.01)), ('sample', dict(temperature=[0.5, 0.5, 0.5])),
             ('greedy', dict(temperature=0.5)), ('greedy', dict(top_k=3)), ('greedy', dict(top_p=0.5))]
    for mode, kw in cases:
        with pytest.raises(ValueError) as want:
            pkg.generator.sampling_settings(2, mode, **kw)
        with pytest.raises(ValueError) as got:
            gen.generate(None, 8, mode=mode, **kw)
        assert str(got.value) == str(want.value)
    with pytest.raises(NotImplementedError):
        gen.generate(None, 8, mode='beam')
    assert not hasattr(gen, 'prefill') and 'no prefill' in pkg.generator.WideGenerator.__doc__
    assert 'FastGenerator.prefill' in pkg.generator.WideGenerator.__doc__


# ------------------------------------------------------------------ the C boundary
def test_wide_symbols_are_declared_and_exported(pkg, tmp_path):
    L = pkg._lib
    src = re.sub(r'/\*.*?\*/', '', open(HDR).read(), flags=re.S)
    for name in WIDE:
        decl = re.search(r'\bint\s+%s\s*\(([^;]*)\)\s*;' % name, src)
        assert decl, '%s is not declared in vqwave.h' % name
        assert name in L.SIGNATURES, '%s is not declared in _lib.py' % name
        res, args = L.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(decl.group(1).split(','))
        assert hasattr(L.lib(), name)
    # the struct the run call takes per row
    prog = tmp_path / 'sz.c'
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vqwave.h"\nint main(){printf("%zu %zu %zu %zu\\n", '
                    'sizeof(vqw_ar_sampling), offsetof(vqw_ar_sampling, top_k), offsetof(vqw_ar_sampling, top_p), '
                    'sizeof(vqw_ar_weights));return 0;}\n')
    exe = tmp_path / 'sz'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(prog), '-o', str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(L.ArSampling), L.ArSampling.top_k.offset, L.ArSampling.top_p.offset, ctypes.sizeof(L.ArWeights)]


def test_wide_create_refuses_shapes_by_name(pkg):
    """Errors are reported, not raised, and name the value; every check comes before the first device call."""
    L = pkg._lib
    lib = L.lib()
    assert lib.vqw_ar_wide_create(None, None, 1) != 0 and b'null pointer' in lib.vqw_last_error()
    for name in ('vqw_ar_wide_reset', 'vqw_ar_wide_wait'):
        assert getattr(lib, name)(*([None] * len(L.SIGNATURES[name][1]))) != 0 and b'null handle' in lib.vqw_last_error()
    assert lib.vqw_ar_wide_run_async(None, None, 1, 1, 1, 0, None, None, None, None, None, None) != 0
    assert lib.vqw_ar_wide_destroy(None) == 0

    def weights(**kw):
        w = L.ArWeights()
        w.n_layers, w.kernel_size, w.R, w.S, w.Q, w.Cc, w.pre_k = 2, 3, 32, 64, 256, 32, 32
        for k, v in kw.items():
            setattr(w, k, v)
        return w
    h = ctypes.c_void_p()
    for batch, kw, match in [(1025, {}, 'batch=1025'), (0, {}, 'batch=0'), (4, dict(R=48), 'R=48'), (4, dict(Q=1056), 'Q=1056'),
                             (4, dict(S=80), 'S=80'), (4, dict(Cc=24), 'Cc=24'), (4, dict(pre_k=65), 'pre_k=65'),
                             (4, dict(kernel_size=1), 'kernel_size=1'), (4, dict(kernel_size=9), 'kernel_size=9')]:
        w = weights(**kw)
        assert lib.vqw_ar_wide_create(ctypes.byref(h), ctypes.byref(w), batch) != 0
        assert match in lib.vqw_last_error().decode(), lib.vqw_last_error()
    assert h.value is None
