"""Writes tests/golden/generator_digests.json: a SHA-256 per case and output of tests/generator_cases.py.

    python tests/golden/make_generator_digests.py [OUT.json]

Run on the GPU against the commit whose results are to be pinned (the parent of a change that must leave every output bit
for bit what it was); it calls public methods only.  tests/test_generator_digests_gpu.py compares against the file."""
import importlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import generator_cases as C  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, 'generator_digests.json')
    pkg = importlib.import_module('vq-vae-wavenet_amd')
    models = C.make_models(pkg)
    d = {}
    for backend in C.BACKENDS:
        for k, v in C.environment(backend).items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
        d.update(C.run_backend(pkg, models, backend))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
        json.dump(d, f, indent=0, sort_keys=True)
        f.write('\n')
    print('%d cases, %d digests -> %s' % (len(d), sum(len(v) for v in d.values()), out))


if __name__ == '__main__':
    main()
