"""CPU tests of what the wide generators' prefill adds outside the kernels: the refusals of `generate.py -takes` (before the
package is imported) and the path `-takes` chooses, generator.prefill_chunk, the C boundary of vqw_ar_wide_prefill_layer /
_finish (declared, bound, exported, a null handle refused with no device present), the argument checks of
WideGenerator.prefill_prompt / WidePriorGenerator.prefill_codes, and tools/ar_wide_plan_check.cpp, which sweeps the scatter's
range, slot and tile arithmetic (csrc/ar_wide_plan.h) on bounds-checked buffers."""
import ctypes
import importlib.util
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, 'include', 'vqwave.h')

# runs generate.py with a guard on importlib.import_module: importing the package ends the process with status 97
# (the pattern of test_wide_prior_cpu.py)
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


PROMPT = ['-audio', 'a.wav', '-prompt_samples', '100']
PRIOR_PROMPT = ['-prior', 'p.pt', '-audio', 'a.wav', '-prompt_frames', '2']


# ------------------------------------------------------------------ generate.py -takes
@pytest.mark.parametrize('extra, match', [
    (PROMPT + ['-takes', '0'], '-takes 0 must be >= 1'),
    (PROMPT + ['-takes', '-2'], '-takes -2 must be >= 1'),
    (['-audio', 'a.wav', '-takes', '4'], '-takes 4 needs a prompt (-prompt_samples, or -prompt_frames with -prior); without one, '
                                         '-audio_list converts many utterances and -prior -count samples many takes'),
    (['-prior', 'p.pt', '-takes', '2'], '-takes 2 needs a prompt'),
    (PROMPT + ['-takes', '2', '-mode', 'greedy'], '-takes 2 with -mode greedy: all takes of a prompt would be equal'),
    (['-audio_list', 'l.txt', '-takes', '2'], '-takes 2 continues one prompt several times: not with -audio_list'),
    (PRIOR_PROMPT + ['-takes', '2', '-count', '2'], '-takes 2 continues one prompt several times: not with -count above 1'),
    (PROMPT + ['-takes', '2', '-teacher_forced'], '-takes 2 continues one prompt several times: not with -teacher_forced'),
    (PROMPT + ['-takes', '2', '-rows', '0'], '-rows 0 must be in 1..1024'),
    (PRIOR_PROMPT + ['-takes', '2', '-rows', '1025'], '-rows 1025 must be in 1..1024'),
])
def test_takes_refuses_bad_flags(tmp_path, extra, match):
    """The message is looked for in the error line alone: the usage text before it names every flag on any argparse exit."""
    out = run_cli(tmp_path, extra)
    assert out.returncode == 2 and ': error: ' in out.stderr, (out.returncode, out.stderr[-1000:])
    assert match in out.stderr.split(': error: ', 1)[1], out.stderr[-1000:]


def test_takes_passes_its_checks_then_imports_the_package(tmp_path):
    """Valid combinations reach the package import (status 97); -takes 1 does not look at -rows."""
    for extra in (PROMPT + ['-takes', '2'], PROMPT + ['-takes', '3', '-rows', '1'], PRIOR_PROMPT + ['-takes', '2', '-rows', '1024'],
                  PROMPT + ['-takes', '1', '-rows', '0'], PROMPT + ['-takes', '1', '-mode', 'greedy']):
        out = run_cli(tmp_path, extra)
        assert out.returncode == 97 and 'THE PACKAGE WAS IMPORTED' in out.stderr, (extra, out.returncode, out.stderr[-1000:])


def test_existing_prompt_refusals_keep_their_messages(tmp_path):
    """-takes is looked at first only where it is above 1: the pinned refusals of a prompt with -audio_list / -count stay."""
    out = run_cli(tmp_path, ['-audio_list', 'l.txt', '-prompt_samples', '100', '-takes', '1'])
    assert out.returncode == 2 and 'not with -prompt_samples' in out.stderr.split(': error: ', 1)[-1], out.stderr[-1000:]
    out = run_cli(tmp_path, PRIOR_PROMPT + ['-count', '2', '-takes', '1'])
    assert out.returncode == 2 and 'the wide generators have no prefill' in out.stderr.split(': error: ', 1)[-1], out.stderr[-1000:]


@pytest.fixture(scope='module')
def cli():
    spec = importlib.util.spec_from_file_location('generate_cli_takes', os.path.join(ROOT, 'generate.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Reached(Exception):
    pass


@pytest.mark.parametrize('takes, want', [(None, 'read_wav'), ('1', 'read_wav'), ('2', 'prompted_takes')])
def test_takes_one_stays_on_the_old_path(pkg, cli, monkeypatch, takes, want):
    """-audio -prompt_samples: without -takes and with -takes 1 main() goes on to read the utterance itself (the FastGenerator
    path); only -takes above 1 hands over to prompted_takes."""
    def stop(name):
        def f(*a, **k):
            raise Reached(name)
        return f
    monkeypatch.setattr(cli, 'read_wav', stop('read_wav'))
    monkeypatch.setattr(cli, 'prompted_takes', stop('prompted_takes'))
    monkeypatch.setattr(torch.cuda, 'set_device', lambda *_: None)
    monkeypatch.setattr(sys, 'argv', ['generate.py', '-restore', 'none/weights-1.pt', '-speakers', 'p225'] + PROMPT
                        + ([] if takes is None else ['-takes', takes]))
    with pytest.raises(Reached, match=want):
        cli.main()


# ------------------------------------------------------------------ prefill_chunk
def test_prefill_chunk(pkg):
    pc = pkg.generator.prefill_chunk
    # tiny widths, T = 200: R 32, Mall = 10 * 64 + 64 = 704, window [32, 208): Tw 176, 11 frames
    row = 4 * (3 * 32 * 176 + 704 * 11)
    assert row == 98560
    assert pc(70, 32, 704, 176, 11, budget=7 * row) == 7 and pc(70, 32, 704, 176, 11, budget=7 * row - 1) == 6
    assert pc(70, 32, 704, 176, 11, budget=8 * row - 1) == 7
    assert pc(70, 32, 704, 176, 11, budget=0) == 1 and pc(70, 32, 704, 176, 11, budget=row - 1) == 1       # never below one row
    assert pc(70, 32, 704, 176, 11, budget=70 * row) == 70 and pc(70, 32, 704, 176, 11, budget=10 ** 12) == 70   # never above B
    assert pc(5, 32, 704, 0, 0) == 5                                      # an empty window costs nothing
    # reference widths, a saturated window: R 256, Mall = 30 * 512 + 512, Tw 6208, 97 frames: 25 229 312 bytes per row
    ref = 4 * (3 * 256 * 6208 + 15872 * 97)
    assert ref == 25229312
    assert pc(1024, 256, 15872, 6208, 97, budget=1 << 30) == 42 and pc(1024, 256, 15872, 6208, 97, budget=(1 << 30) + ref) == 43
    default = pc(1024, 256, 15872, 6208, 97)
    assert default == pkg.generator.PREFILL_BUDGET // ref and 32 <= default < 1024      # whole scatter tiles, far from 26 GB
    assert default * ref <= pkg.generator.PREFILL_BUDGET < (default + 1) * ref
    last = 0
    for budget in range(0, 80 * row, row // 3):                            # monotone in the budget, always in 1..B
        c = pc(70, 32, 704, 176, 11, budget=budget)
        assert 1 <= c <= 70 and c >= last and (c == 70 or c == max(1, budget // row))
        last = c
    assert last == 70
    for B in (1, 2, 1024):
        assert 1 <= pc(B, 256, 15872, 6208, 97) <= B
    for bad in (dict(batch=0), dict(R=0), dict(Mall=-1), dict(Tw=-1), dict(budget=-1), dict(batch=True), dict(batch=2.0)):
        kw = dict(batch=4, R=32, Mall=704, Tw=176, Tzw=11, budget=1 << 20)
        kw.update(bad)
        with pytest.raises(ValueError, match='prefill_chunk'):
            pc(**kw)


def test_even_chunk(pkg):
    """The fewest passes of at most max_rows rows, cut evenly: never more rows than the budget allows, never more passes."""
    ec = pkg.generator.even_chunk
    assert ec(256, 85) == 64 and ec(1024, 85) == 79 and ec(70, 32) == 24 and ec(70, 70) == 70 and ec(70, 100) == 70
    assert ec(8, 85) == 8 and ec(1, 1) == 1 and ec(7, 1) == 1 and ec(65, 64) == 33
    for B in range(1, 200):
        for mx in (1, 2, 7, 32, 33, 85, 300):
            c = ec(B, mx)
            passes = -(-B // c)
            assert 1 <= c <= min(B, mx) and passes == -(-B // mx), (B, mx, c)      # within the budget, no extra pass
            assert c - (B - (passes - 1) * c) < passes, (B, mx, c)                 # the last chunk is short by less than a row per pass
    for bad in ((0, 4), (4, 0), (True, 4), (4, 2.0)):
        with pytest.raises(ValueError, match='even_chunk'):
            ec(*bad)


# ------------------------------------------------------------------ the C boundary
@pytest.mark.parametrize('name, nargs', [('vqw_ar_wide_prefill_layer', 9), ('vqw_ar_wide_prefill_finish', 5)])
def test_prefill_calls_are_declared_and_exported(pkg, name, nargs):
    L = pkg._lib
    src = re.sub(r'/\*.*?\*/', '', open(HDR).read(), flags=re.S)
    decl = re.search(r'\bint\s+%s\s*\(([^;]*)\)\s*;' % name, src)
    assert decl, '%s is not declared in vqwave.h' % name
    assert name in L.SIGNATURES, '%s is not declared in _lib.py' % name
    res, args = L.SIGNATURES[name]
    assert res is ctypes.c_int and len(args) == len(decl.group(1).split(',')) == nargs
    assert hasattr(L.lib(), name)


def test_prefill_calls_refuse_a_null_handle(pkg):
    """Reported, not raised, with no device present."""
    lib = pkg._lib.lib()
    assert lib.vqw_ar_wide_prefill_layer(None, 0, None, 8, 0, 8, 0, 1, None) != 0
    assert lib.vqw_last_error().decode() == 'vqw_ar_wide_prefill_layer: null handle'
    assert lib.vqw_ar_wide_prefill_finish(None, 8, None, None, None) != 0
    assert lib.vqw_last_error().decode() == 'vqw_ar_wide_prefill_finish: null handle'


def test_header_and_docstrings_name_the_wide_prefill(pkg):
    """The header no longer denies a prefill.  The classes keep the name `prefill` for the one-to-eight-row generators (older
    tests pin that a wide generator has no such attribute) and say which method prefills a wide handle."""
    hdr = open(HDR).read()
    assert 'There is no prefill' not in hdr
    for cls, peer, name in ((pkg.generator.WideGenerator, 'FastGenerator.prefill', 'prefill_prompt'),
                            (pkg.generator.WidePriorGenerator, 'PriorGenerator.prefill', 'prefill_codes')):
        assert 'There is no prefill' not in cls.__doc__ and peer in cls.__doc__ and name + '()' in cls.__doc__
        assert callable(getattr(cls, name)) and not hasattr(cls, 'prefill')


# ------------------------------------------------------------------ the Python methods' checks
class FakeModel:
    Cc, Q, pre_k = 4, 32, 3


def test_wide_prefill_refuses_bad_arguments_before_the_device(pkg):
    """The checks are FastGenerator.prefill's and PriorGenerator.prefill's own (shared code): same messages, no GPU touched."""
    g = pkg.generator
    wide, fast = g.WideGenerator.__new__(g.WideGenerator), g.FastGenerator.__new__(g.FastGenerator)
    for gen in (wide, fast):
        gen.B, gen.model, gen._h, gen._hs = 2, FakeModel(), None, []
    enc = torch.zeros(2, 4, 3)
    cases = [(torch.zeros(3, 10), enc), (torch.zeros(2, 10, dtype=torch.float64), enc), (torch.zeros(10), enc), ([0.0] * 10, enc),
             (torch.zeros(2, 10), torch.zeros(2, 5, 3)), (torch.zeros(2, 10), torch.zeros(1, 4, 3)), (torch.zeros(2, 193), enc)]
    for prompt, e in cases:
        with pytest.raises(ValueError) as want:
            fast.prefill(prompt, e)
        with pytest.raises(ValueError) as got:
            wide.prefill_prompt(prompt, e)
        assert str(got.value) == str(want.value)
    with pytest.raises(ValueError, match='longer than the encoding'):
        wide.prefill_prompt(torch.zeros(2, 49), enc, ratio=16)
    with pytest.raises(ValueError, match='contiguous tensors on the GPU'):
        wide.prefill_prompt(torch.zeros(2, 48), enc, ratio=16)
    widep = g.WidePriorGenerator.__new__(g.WidePriorGenerator)
    widep.B, widep.model, widep._h, widep._t = 2, FakeModel(), None, 0
    with pytest.raises(ValueError, match=r'codes must be an int32 \[2\]\[T\] tensor on the GPU'):
        widep.prefill_codes(torch.zeros(2, 5, dtype=torch.int32), torch.zeros(2, dtype=torch.int64))
    assert widep._t == 0


def test_prefill_tail(pkg):
    tail = pkg.generator._prefill_tail
    x = torch.arange(20, dtype=torch.float32).reshape(2, 10)
    assert torch.equal(tail(x, 10, 3), x[:, 7:10]) and torch.equal(tail(x, 5, 3), x[:, 2:5])
    assert torch.equal(tail(x, 2, 3), torch.tensor([[0., 0., 1.], [0., 10., 11.]]))
    assert tail(x.int(), 1, 4).dtype == torch.int32 and torch.equal(tail(x.int(), 1, 4), torch.tensor([[0, 0, 0, 0], [0, 0, 0, 10]], dtype=torch.int32))


# ------------------------------------------------------------------ the plan's sweep
def test_plan_check_sweeps_the_prefill_arithmetic(tmp_path):
    """tools/ar_wide_plan_check.cpp, built as its head says (a stand-alone host program under the address and undefined
    behaviour sanitizers) and run: it replays the scatter's tiles over bounds-checked buffers."""
    cxx = shutil.which('g++') or shutil.which('c++')
    assert cxx, 'no host C++ compiler'
    src = os.path.join(ROOT, 'tools', 'ar_wide_plan_check.cpp')
    exe = str(tmp_path / 'ar_wide_plan_check')
    out = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', src, '-o', exe],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith('ok: '), (out.stdout[-500:], out.stderr[-2000:])
    m = re.search(r'(\d+) prefilled values', out.stdout)
    assert m and int(m.group(1)) > 10 ** 6, out.stdout
