"""Writes tests/golden/x3_loop_digests.json: a SHA-256 per case and output of tests/x3_loop_cases.py.

    python tests/golden/make_x3_loop_digests.py [OUT.json]

Run on the GPU against a library built from the commit whose results are to be pinned (the parent of a change to the conv
main loop that must leave every output bit for bit what it was).  tests/test_x3_loop_gpu.py compares against the file."""
import importlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import x3_loop_cases as X  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, 'x3_loop_digests.json')
    K = importlib.import_module('vq-vae-wavenet_amd').kernels
    d = X.all_digests(K)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
        json.dump(d, f, indent=0, sort_keys=True)
        f.write('\n')
    print('%d cases, %d digests -> %s' % (len(d), sum(len(v) for v in d.values()), out))


if __name__ == '__main__':
    main()
