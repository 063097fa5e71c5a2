"""The main loop of the fp16x3 conv kernels only changes HOW operands travel to LDS: every output of every case of
tests/x3_loop_cases.py is bit for bit what tests/golden/x3_loop_digests.json recorded at the commit before the loop staged its
operands by LDS-DMA (a differing digest means a stage reached the MFMAs with other bytes than the register ring gave it: a
padding row that did not read zero, a stage read before it had landed, a ring slot refilled too early).
The table runs once per session; the tests read its digests."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import x3_loop_cases as X  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'x3_loop_digests.json')


@pytest.fixture(scope='module')
def got(K):
    return X.all_digests(K)


@pytest.fixture(scope='module')
def want():
    with open(GOLDEN) as f:
        return json.load(f)


def _differing(got, want, prefix):
    names = [n for n in got if n.startswith(prefix)]
    assert names and all(n in want for n in names), 'cases absent from the golden file'
    return [(n, k) for n in names for k in sorted(set(got[n]) | set(want[n])) if got[n].get(k) != want[n].get(k)]


def test_table_is_the_recorded_one(got, want):
    assert sorted(got) == sorted(want) and len(got) == 2 * (2 * 4 + 1) + 3 + 2 * (2 * 4 + 1) + 3


@pytest.mark.parametrize('kernel', ['gate', 'dgrad'])
def test_dilated_taps_match_the_parent(got, want, kernel):
    """d = 1, 2, 256, 512 at T = 512: rows before / behind their batch row read zero in every column tile."""
    bad = _differing(got, want, kernel + '/')
    assert not bad, '%d outputs differ from the parent commit: %s' % (len(bad), bad[:8])
    for mn in ('m0', 'half'):
        for d in X.DILATIONS:
            assert '%s/%s/d=%d' % (kernel, mn, d) in got
    assert '%s/bf16/d=256' % kernel in got


def test_long_contraction_matches_the_parent(got, want):
    """48 K steps: the ring wraps 12 to 16 times."""
    bad = _differing(got, want, 'head/')
    assert not bad, '%d outputs differ from the parent commit: %s' % (len(bad), bad[:8])


@pytest.mark.parametrize('direction', ['fwd', 'dgrad'])
def test_strided_convs_match_the_parent(got, want, direction):
    """Every block shape, unsplit and split-K, forward and input gradient (whose two parities run the loop twice per block)."""
    bad = _differing(got, want, 'sconv/%s/' % direction)
    assert not bad, '%d outputs differ from the parent commit: %s' % (len(bad), bad[:8])
    for Cin in (64, 128):
        for shape in X.SCONV_SHAPES:
            assert 'sconv/%s/T=256/Cin=%d/shape=%d' % (direction, Cin, shape) in got
    assert sum(n.startswith('sconv/%s/T=64/' % direction) for n in got) >= 2
    for n in got:
        if 'split' in n:      # (the ticket counters are back at zero: the digest of 1024 zero words)
            assert got[n]['counters'] == want[n]['counters']
