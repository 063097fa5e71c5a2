"""The generators' host code is stated once (generator.py's shared helpers, csrc/ar_host.h) and the default row's sampling
once (ar_sampling.h): every tensor every case of tests/generator_cases.py returns is bit for bit what
tests/golden/generator_digests.json recorded at the commit before (a differing digest of a launch-per-phase or wide case
means the sampling's operation order moved; of every case of a backend, that the host path hands the kernels other
arguments)."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import generator_cases as C  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'generator_digests.json')


@pytest.fixture(scope='module')
def models(pkg):
    made = C.make_models(pkg)
    yield made
    made.clear()


@pytest.fixture(scope='module')
def want():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.gpu
@pytest.mark.parametrize('backend', list(C.BACKENDS))
def test_every_digest_matches_the_parent(pkg, models, want, monkeypatch, backend):
    for k, v in C.environment(backend).items():
        monkeypatch.delenv(k, raising=False)
        if v is not None:
            monkeypatch.setenv(k, v)
    got = C.run_backend(pkg, models, backend)
    assert len(got) == (2 if backend.startswith('flat/') else 3)
    for name in got:
        assert name in want, 'case %s is absent from the golden file' % name
        n_out = 4 if C.BACKENDS[backend][1] == 'prior' else 6
        assert len(got[name]) == n_out and sorted(got[name]) == sorted(want[name])
    bad = [(n, k) for n in got for k in got[n] if got[n][k] != want[n][k]]
    assert not bad, '%d outputs differ from the parent commit: %s' % (len(bad), bad)


def test_the_golden_file_holds_these_cases_only(want):
    names = ['%s/%s' % (b, d) for b in C.BACKENDS for d in C.DRAWS if not (b.startswith('flat/') and d == 'mixed')]
    assert sorted(want) == sorted(names) and len(names) == 6 * 3 + 3 * 2
