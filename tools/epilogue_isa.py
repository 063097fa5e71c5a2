"""How many memory requests do the epilogues of the fp16x3 conv kernels keep in flight?  ("Epilogue request depth")

    python tools/epilogue_isa.py [--asm FILE.s] [--keep FILE.s] > profiles/epilogue_isa_<tag>.txt

Compiles the sources of the fp16x3 engine that hold *_f16x3_kernel instantiations (vq-vae-wavenet_amd/csrc/f16x3_*.hip, SRCS) to
gfx950 assembly with build.py's FLAGS, side by side (under a minute), into ONE listing (--keep keeps it; --asm reads a listing made
earlier instead) and prints, for every *_f16x3_kernel instantiation, the vector-memory instructions
behind its last v_mfma in text order:

    L  a load (global / buffer / flat)         S  a 4-byte store         P  a wider store (plane entries)
    A  an atomic                               w(n)  s_waitcnt vmcnt(n)  B  a branch          | a new group of loads

Runs are written L*12, equal consecutive groups once with a repeat count.  On gfx950 loads and stores share vmcnt and
retire in issue order, so the counter is modelled as a FIFO: w(n) drops the oldest entries until n remain.  Three
counts per instantiation:

    loads->w(0)   loads whose next memory event is vmcnt(0): one exposed round trip each
    depth@store   the largest / smallest number of loads still in the FIFO when a store is issued, and how many
                  stores are issued with none (nothing of a later group has been requested; the stores of the
                  last groups always are)
    branches      conditional and unconditional branches behind the last MFMA

Text order is execution order inside a straight-line epilogue; where a kernel holds several epilogue bodies under a
block-uniform branch they follow one another (the FIFO is emptied at s_endpgm and at unconditional branches).
Only loads, stores and wait counts are looked at."""
import argparse
from concurrent.futures import ThreadPoolExecutor
import re
import sys

from isa_listing import compile_asm, demangle, short, split_kernels

SRCS = ['f16x3_%s' % n for n in ('conv', 'gate_bwd', 'sconv', 'wgrad')]


LOAD = re.compile(r'^(global|buffer|flat)_load_')
STORE = re.compile(r'^(global|buffer|flat)_store_(\w+)')
ATOM = re.compile(r'^(global|buffer|flat)_atomic_')
VMCNT = re.compile(r'vmcnt\((\d+)\)')


def events(body):
    """[(kind, n)] behind the last MFMA of a kernel body (a list of instruction lines)."""
    last = max((i for i, l in enumerate(body) if l.startswith('v_mfma')), default=-1)
    ev = []
    for l in body[last + 1:]:
        op = l.split()[0]
        if LOAD.match(op):
            ev.append(('L', 0))
        elif STORE.match(op):
            ev.append(('S' if STORE.match(op).group(2) in ('dword', 'byte', 'short', 'b32') else 'P', 0))
        elif ATOM.match(op):
            ev.append(('A', 0))
        elif op == 's_waitcnt':
            m = VMCNT.search(l)
            if m:
                ev.append(('w', int(m.group(1))))
        elif op.startswith('s_cbranch') or op == 's_branch':
            ev.append(('B', 1 if op == 's_branch' else 0))
        elif op == 's_endpgm':
            ev.append(('E', 0))
    return ev


def counts(ev):
    fifo, exposed, dmax, dmin, br, nst, nbare = [], 0, 0, None, 0, 0, 0
    for i, (k, n) in enumerate(ev):
        if k == 'L':
            fifo.append('L')
            if i + 1 < len(ev) and ev[i + 1] == ('w', 0):
                exposed += 1
        elif k in 'SPA':
            if k != 'A':
                d = fifo.count('L')
                dmax, dmin = max(dmax, d), d if dmin is None else min(dmin, d)
                nst, nbare = nst + 1, nbare + (d == 0)
            fifo.append(k)
        elif k == 'w':
            del fifo[:max(0, len(fifo) - n)]
        elif k == 'B':
            br += 1
            if n:
                fifo = []
        elif k == 'E':
            fifo = []
    return exposed, dmax, dmin or 0, br, nst, nbare


def compact(ev):
    """Groups start at the first load behind something that is not a load; runs and repeated groups are folded."""
    groups, cur, prev = [], [], None
    for k, n in ev:
        if k == 'E':
            continue
        if k == 'L' and prev not in (None, 'L') and any(t[0] in 'SP' for t in cur):
            groups.append(cur)
            cur = []
        cur.append((k, n))
        prev = k

    if cur:
        groups.append(cur)

    def fold(g):
        out, i = [], 0
        while i < len(g):
            j = i
            while j < len(g) and g[j] == g[i]:
                j += 1
            k, n = g[i]
            tok = 'w(%d)' % n if k == 'w' else k
            out.append(tok if j - i == 1 else '%s*%d' % (tok, j - i))
            i = j
        return ' '.join(out)
    texts = [fold(g) for g in groups]
    lines, i = [], 0
    while i < len(texts):
        j = i
        while j < len(texts) and texts[j] == texts[i]:
            j += 1
        lines.append('  | %s%s' % (texts[i], '' if j - i == 1 else '      x %d groups' % (j - i)))
        i = j
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--asm', help='read this assembly file instead of compiling')
    ap.add_argument('--keep', help='keep the compiled assembly here')
    a = ap.parse_args()
    if a.asm:
        text = open(a.asm).read()
    else:
        with ThreadPoolExecutor(len(SRCS)) as ex:
            text = ''.join(ex.map(compile_asm, SRCS))
        if a.keep:
            with open(a.keep, 'w') as f:
                f.write(text)
    kernels = split_kernels(text)
    names = [n for n in kernels if re.search(r'(gate|out|head|gate_bwd)_f16x3_kernel', n)]
    dm = demangle(names)
    print('# tools/epilogue_isa.py: vector-memory instructions behind the last MFMA (see the tool for the legend)')
    for n in names:
        ev = events([s for s in kernels[n][0] if s and not s.startswith((';', '.')) and not s.endswith(':')])
        exposed, dmax, dmin, br, nst, nbare = counts(ev)
        mt = kernels[n][2]
        print('\n%s' % short(dm[n]))
        print('  NumVgprs %s  NumAgprs %s  ScratchSize %s' % (mt.get('NumVgprs', '?'), mt.get('NumAgprs', '?'), mt.get('ScratchSize', '?')))
        print('  loads->w(0) %d   depth@store max %d min %d, %d of %d stores with no load in flight   branches %d' % (exposed, dmax, dmin, nbare, nst, br))
        for l in compact(ev):
            print(l)


if __name__ == '__main__':
    sys.exit(main())
