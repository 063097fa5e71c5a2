"""The epilogues of the fp16x3 conv kernels only reorder their memory instructions: every output of every case of
tests/epilogue_cases.py is bit for bit what tests/golden/epilogue_digests.json recorded at the commit before the epilogues were
software-pipelined (a differing digest means an arithmetic expression was regrouped, e.g. by fma contraction: restore it).
The table runs once per session; the other tests read its digests."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epilogue_cases as E  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'epilogue_digests.json')


@pytest.fixture(scope='module')
def got(K):
    return E.all_digests(K)


def test_every_digest_matches_the_parent(got):
    with open(GOLDEN) as f:
        want = json.load(f)
    assert len(got) > 150
    missing = [n for n in got if n not in want]
    assert not missing, 'cases absent from the golden file: %s' % missing[:5]
    bad = [(n, k) for n in got for k in set(got[n]) | set(want[n]) if got[n].get(k) != want[n].get(k)]
    assert not bad, '%d outputs differ from the parent commit, e.g. %s' % (len(bad), bad[:8])


def _same(got, a, b, keys=None):
    """The outputs two cases share (or `keys`) are bitwise equal."""
    keys = keys if keys is not None else sorted(set(got[a]) & set(got[b]))
    assert keys
    for k in keys:
        assert got[a][k] == got[b][k], '%s differs between %s and %s' % (k, a, b)


def test_in_place_equals_out_of_place(got):
    n = 0
    for mn, _ in E.MODES:
        for planes in (0, 1):
            _same(got, 'res/%s/alias=0/planes=%d' % (mn, planes), 'res/%s/alias=1/planes=%d' % (mn, planes),
                  ['skip', 'net_out'] + (['planes', 'amax', 'flag'] if planes else []))
            n += 1
        for dil in (3, 300):
            _same(got, 'dgrad/%s/d=%d/net_in=distinct' % (mn, dil), 'dgrad/%s/d=%d/net_in=alias' % (mn, dil), ['net_out', 'planes', 'amax', 'flag'])
            n += 1
        for cond in (0, 1):
            for relu in (0, 1):
                for alias in ('net_in', 'aux0'):
                    _same(got, 'head/%s/alias=none/cond=%d/relu=%d' % (mn, cond, relu), 'head/%s/alias=%s/cond=%d/relu=%d' % (mn, alias, cond, relu),
                          ['net_out', 'planes', 'amax', 'flag'])
                    n += 1
    assert n == 2 * (2 + 2 + 8)


def test_removing_an_optional_output_leaves_the_others(got):
    n = 0
    for mn, _ in E.MODES:
        # residual 1x1 + skip without the planes and guard slots
        for alias in (0, 1):
            _same(got, 'res/%s/alias=%d/planes=1' % (mn, alias), 'res/%s/alias=%d/planes=0' % (mn, alias), ['skip', 'net_out'])
        # gate backward without fp32 dpre
        for aux in ('tanh', 'gated', 'planes'):
            _same(got, 'bwd/%s/aux0=%s/fp32=1' % (mn, aux), 'bwd/%s/aux0=%s/fp32=0' % (mn, aux), ['planes', 'amax', 'flag'])
        # gate conv: every subset against all four outputs
        for geo in ('R=256/ks=3/d=1/bias=1/cond=1', 'R=128/ks=2/d=300/bias=0/cond=1'):
            full = 'gate/%s/%s/%s' % (mn, geo, '+'.join(E.GATE_OUTPUTS))
            assert sorted(got[full]) == sorted(E.GATE_OUTPUTS)
            for sub in E.GATE_SUBSETS:
                name = 'gate/%s/%s/%s' % (mn, geo, '+'.join(sub))
                assert sorted(got[name]) == sorted(sub)
                _same(got, full, name, list(sub))
                n += 1
    assert n == 2 * 2 * len(E.GATE_SUBSETS) and len(E.GATE_SUBSETS) == 10
