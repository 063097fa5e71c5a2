"""Does a change of the sources leave the generated code of every kernel as it was?  ("Weight gradients")

    python tools/isa_identity.py --base REV UNIT [UNIT ...] > profiles/<tag>_isa_identity.txt      (UNIT: f16x3_wgrad, ...)

Exports vq-vae-wavenet_amd/csrc and include/ of REV (git archive) into a temporary directory, compiles csrc/UNIT.hip of that tree and
of the working tree to gfx950 assembly with build.py's FLAGS and cuts both listings into kernels.  A kernel's text is normalised --
comments and blank lines dropped, the ordinals of the .LBB<n>_ labels and the kernel's own symbol replaced -- and hashed together
with its .amdhsa_kernel descriptor block.  Kernels are matched by hash, not by name: a renamed kernel needs no mapping.  One line
per kernel of REV:

    SAME | DIFF   hash   name in REV -> name in the working tree   instructions

Exit status 1 if a kernel of REV has no match or the numbers of kernels differ.  No instruction is looked for."""
import argparse
import hashlib
import io
import os
import re
import subprocess
import sys
import tarfile
import tempfile
from concurrent.futures import ThreadPoolExecutor

from isa_listing import CSRC, ROOT, compile_asm, demangle, short, split_kernels


def normalised(sym, body, desc):
    """(hash, instructions) of a kernel."""
    def norm(lines):
        lines = (re.sub(r'\s+', ' ', s.split(';')[0]).strip() for s in lines)
        return [re.sub(r'\.LBB\d+_', '.LBB_', s).replace(sym, 'KERNEL') for s in lines if s]
    text = norm(body)
    n = sum(1 for s in text if not s.startswith('.') and not s.endswith(':'))
    return hashlib.sha256('\n'.join(text + norm(desc)).encode()).hexdigest()[:16], n


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--base', required=True, help='the revision to compare the working tree with')
    ap.add_argument('units', nargs='+', help='sources of csrc/, without .hip')
    a = ap.parse_args()
    rev = subprocess.run(['git', 'rev-parse', '--short', a.base], cwd=ROOT, check=True, capture_output=True, text=True).stdout.strip()
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.run(['git', 'archive', a.base, CSRC, 'include'], cwd=ROOT, check=True, capture_output=True).stdout
        tarfile.open(fileobj=io.BytesIO(tar)).extractall(tmp)
        jobs = [(u, r) for u in a.units for r in (tmp, ROOT)]
        with ThreadPoolExecutor(len(jobs)) as ex:
            asm = dict(zip(jobs, ex.map(lambda j: compile_asm(*j), jobs)))
    print('# tools/isa_identity.py --base %s %s: kernels of %s against the working tree, by hash of the normalised text' % (a.base, ' '.join(a.units), rev))
    for u in a.units:
        old, new = split_kernels(asm[u, tmp]), split_kernels(asm[u, ROOT])
        dm = demangle(list(old) + [n for n in new if n not in old])
        left = {}                                   # hash -> names in the working tree not matched yet
        for n, (body, desc, _) in new.items():
            left.setdefault(normalised(n, body, desc)[0], []).append(n)
        same = 0
        print('\n%s.hip: %d kernels in %s, %d in the working tree' % (u, len(old), rev, len(new)))
        for n, (body, desc, _) in old.items():
            h, count = normalised(n, body, desc)
            if left.get(h):
                same += 1
                print('SAME  %s  %s -> %s  %d' % (h, short(dm[n]), short(dm[left[h].pop(0)]), count))
            else:
                print('DIFF  %s  %s -> (no kernel with this hash)  %d' % (h, short(dm[n]), count))
        for h, names in left.items():
            for n in names:
                print('NEW   %s  %s  %d' % (h, short(dm[n]), normalised(n, *new[n][:2])[1]))
        print('%d of %d SAME' % (same, len(old)))
        bad += same != len(old) or len(new) != len(old)
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
