"""What the ISA tools share (epilogue_isa.py, wgrad_loop_isa.py, isa_identity.py): compile a source of the library to gfx950
assembly with build.py's FLAGS, cut a listing into kernels, demangle."""
import importlib.util
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join('vq-vae-wavenet_amd', 'csrc')


def compile_asm(name, root=ROOT):
    """The device assembly of <root>/vq-vae-wavenet_amd/csrc/<name>.hip (compiler and flags: this tree's build.py)."""
    spec = importlib.util.spec_from_file_location('vqw_build', os.path.join(ROOT, 'vq-vae-wavenet_amd', 'build.py'))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    cmd = [b._hipcc()] + b.FLAGS + ['--cuda-device-only', '-S', '-o', '-', os.path.join(root, CSRC, name + '.hip')]
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def split_kernels(text):
    """{symbol: (body, descriptor, meta)} in text order: the stripped lines from behind the kernel's label to its descriptor, those
    of its .amdhsa_kernel block, and {'NumVgprs' | 'NumAgprs' | 'ScratchSize': n} of the comments that follow it."""
    syms = set(re.findall(r'^\s*\.amdhsa_kernel\s+(\S+)', text, re.M))
    kernels, cur, part = {}, None, None          # part: 'body', 'gap' (body to descriptor), 'desc', 'meta'
    for line in text.splitlines():
        s = line.strip()
        m = re.match(r'^(\w+):', s)
        if m and m.group(1) in syms:
            cur, part = ([], [], {}), 'body'
            kernels[m.group(1)] = cur
            continue
        if cur is None:
            continue
        if part in ('body', 'gap') and s.startswith('.amdhsa_kernel'):
            part = 'desc'
        elif part == 'body' and s.startswith('.section'):
            part = 'gap'
        if part == 'body':
            cur[0].append(s)
        elif part == 'desc':
            cur[1].append(s)
            if s.startswith('.end_amdhsa_kernel'):
                part = 'meta'
        elif part == 'meta':
            m = re.match(r'^; (NumVgprs|NumAgprs|ScratchSize): (\d+)', s)
            if m:
                cur[2][m.group(1)] = int(m.group(2))
    return kernels


def demangle(names):
    if not names:
        return {}
    try:
        r = subprocess.run(['c++filt'] + list(names), capture_output=True, text=True, check=True)
        return dict(zip(names, r.stdout.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def short(demangled):
    return re.sub(r'\(anonymous namespace\)::|void |\(.*\)$', '', demangled)
