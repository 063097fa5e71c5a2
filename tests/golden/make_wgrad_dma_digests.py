"""Writes tests/golden/wgrad_dma_digests.json: a SHA-256 per case and dW of tests/wgrad_dma_cases.py.

    python tests/golden/make_wgrad_dma_digests.py [OUT.json]

Run on the GPU against a library built from the commit whose results are to be pinned (the parent of a change to the
planes-both weight-gradient loop that must leave every dW bit for bit what it was).  tests/test_wgrad_dma_gpu.py compares
against the file."""
import importlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import wgrad_dma_cases as W  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, 'wgrad_dma_digests.json')
    K = importlib.import_module('vq-vae-wavenet_amd').kernels
    d = W.all_digests(K)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
        json.dump(d, f, indent=0, sort_keys=True)
        f.write('\n')
    print('%d cases, %d digests -> %s' % (len(d), sum(len(v) for v in d.values()), out))


if __name__ == '__main__':
    main()
