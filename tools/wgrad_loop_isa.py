"""What does the main loop of the planes-both weight-gradient kernels issue?  ("Weight gradients")

    python tools/wgrad_loop_isa.py [--asm FILE.s] > profiles/wgrad_split_isa.txt

Compiles vq-vae-wavenet_amd/csrc/f16x3_wgrad.hip to gfx950 assembly with build.py's FLAGS (or reads a listing made earlier) and
prints, for the wgrad_f16x3_dma_kernel instantiations (both operands as planes), every vector-memory, LDS, wait, barrier
and branch instruction from the first s_barrier to the last `s_waitcnt vmcnt(0)` in front of the slab stores, in text order:

    D  an LDS-DMA request (buffer_load ... lds)    L  another load          S  a store         A  an atomic
    R  an LDS read (T: ds_read_b64_tr_b16)          W  an LDS write          M*n  n MFMAs
    w(n) / l(n)  s_waitcnt vmcnt(n) / lgkmcnt(n)    BAR  s_barrier           B  a branch        <label>:  a branch target

Runs are folded (T*4).  Between the loop's barriers there should be no w(0) and no W."""
import argparse
import re
import sys

from isa_listing import compile_asm, demangle, short, split_kernels


def token(s):
    op = s.split()[0]
    if re.match(r'^(global|buffer|flat)_load_', op):
        return 'D' if re.search(r'\blds\b', s) else 'L'
    if re.match(r'^(global|buffer|flat)_store_', op):
        return 'S'
    if re.match(r'^(global|buffer|flat)_atomic_', op):
        return 'A'
    if op.startswith('ds_read_b64_tr'):
        return 'T'
    if op.startswith('ds_read') or op.startswith('ds_load'):
        return 'R'
    if op.startswith('ds_write'):
        return 'W'
    if op.startswith('v_mfma'):
        return 'M'
    if op == 's_barrier':
        return 'BAR'
    if op.startswith('s_cbranch') or op == 's_branch':
        return 'B'
    if op == 's_waitcnt':
        out = []
        m = re.search(r'vmcnt\((\d+)\)', s)
        if m:
            out.append('w(%s)' % m.group(1))
        m = re.search(r'lgkmcnt\((\d+)\)', s)
        if m:
            out.append('l(%s)' % m.group(1))
        return ' '.join(out) or None
    if re.match(r'^\.LBB\w+:', s):
        return '\n  %s' % s
    return None


def fold(toks):
    out, i = [], 0
    while i < len(toks):
        j = i
        while j < len(toks) and toks[j] == toks[i] and not toks[i].startswith('\n'):
            j += 1
        j = max(j, i + 1)
        out.append(toks[i] if j - i == 1 else '%s*%d' % (toks[i], j - i))
        i = j
    return ' '.join(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--asm', help='read this assembly file instead of compiling')
    a = ap.parse_args()
    kernels = split_kernels(open(a.asm).read() if a.asm else compile_asm('f16x3_wgrad'))
    dm = demangle([n for n in kernels if 'wgrad_f16x3_dma_kernel' in n])
    names = sorted(dm, key=dm.get)          # <false> (fp16x3) before <true> (bf16), whatever the order in the listing
    print('# tools/wgrad_loop_isa.py: the planes-both weight-gradient loop, first barrier to the wait before the slab stores (see the tool for the legend)')
    for n in names:
        # instructions and branch targets
        b = [s for s in kernels[n][0] if s and not s.startswith(';') and (not s.startswith('.') or re.match(r'^\.LBB\w+:', s))]
        bars = [i for i, l in enumerate(b) if l.split()[0] == 's_barrier']
        mt = kernels[n][2]
        print('\n%s' % short(dm[n]))
        print('  NumVgprs %s  NumAgprs %s  ScratchSize %s' % (mt.get('NumVgprs', '?'), mt.get('NumAgprs', '?'), mt.get('ScratchSize', '?')))
        if not bars:
            print('  (no s_barrier)')
            continue
        end = next((i for i in range(bars[-1], len(b)) if re.search(r'vmcnt\(0\)', b[i])), len(b) - 1)
        toks = [t for t in (token(l) for l in b[bars[0]:end + 1]) if t]
        inner = [t for l in b[bars[0]:bars[-1]] for t in [token(l)] if t]
        print('  between the barriers: %d DMA requests, %d transposed reads, %d other LDS reads, %d LDS writes, %d vmcnt(0), %d branches' % (
            inner.count('D'), inner.count('T'), inner.count('R'), inner.count('W'), sum('w(0)' in t for t in inner), inner.count('B')))
        print('  ' + fold(toks).replace('BAR', '\n  BAR'))


if __name__ == '__main__':
    sys.exit(main())
