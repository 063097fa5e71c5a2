"""The planted sampling cases (sampling_cases.py) on the CPU: every case is clean (sampling_ref.planted_clean: nothing may be
excused), the float32 restatement of the kernel's rule keeps what the float64 restatement keeps, every wrong evaluation of
sampling_ref.WRONG is told apart by at least one case of every Q it applies to, and sampling_ref.fp32_edge -- the predicate
of the continuous-logits tests -- would have excused the tie cases, which is the gap the planted cases close."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampling_cases as C  # noqa: E402
import sampling_ref as S  # noqa: E402

T_CPU = 16          # positions per row here (the GPU tests plant more, and assert Planted.faults == [] themselves)


def cases(Q):
    for i in range(C.N_STAIRCASES):
        st = C.staircase(Q, i)
        for row in C.settings(st):
            yield st, row


def test_staircases_are_as_described():
    for Q in C.QS + C.CODE_QS:
        kinds = set()
        for i in range(C.N_STAIRCASES):
            st = C.staircase(Q, i)
            z = C.logits(st, 3)
            assert sum(st.counts) == Q and 2 <= len(st.counts) <= 5 and z.dtype == np.float32 and np.isfinite(z).all()
            assert sorted(z.tolist()) == sorted(C.canonical(st).tolist())
            assert all(float(np.float32(v)) == v and v * 4 == int(v * 4) for v in st.values)
            for t in C.TEMPERATURES:
                lv = (np.asarray(st.values) - st.values[0]) / t
                body = lv[:-1] if st.under else lv
                assert (np.diff(body) <= -0.75).all() and body[-1] >= -40 and (not st.under or lv[-1] <= -120)
            ks = C.top_ks(st)
            above, count = C.plateau(st)
            assert count >= 2 and {0, 1, above + count} <= set(ks) and any(above < k < above + count for k in ks)
            if st.under:
                assert any(Q - st.counts[-1] < k < Q for k in ks)                 # more than the non-zero classes
                assert float(np.exp(np.float32(lv[-1]))) == 0.0 and np.exp(lv[-1] * 2) > 0
            kinds.add((st.counts[0] == 1, st.under))
            rows = C.settings(st)
            assert {r[0] for r in rows} == set(C.TEMPERATURES) and any(r[2] == 1.0 for r in rows) and any(r[2] < 1.0 for r in rows)
        assert len(kinds) >= 2


@pytest.mark.parametrize('Q', C.QS + C.CODE_QS)
def test_every_case_is_clean_and_fp32_keeps_the_same_set(Q):
    closest = 1.0
    n_rows = 0
    for i in range(C.N_STAIRCASES):
        st = C.staircase(Q, i)
        rows = C.settings(st)
        n_rows += len(rows)
        planted = C.plant(st, rows, T_CPU)
        assert planted.faults == []
        assert (planted.u[:, 0] == 0.0).all() and (planted.u[:, 1] == 2.0).all() and (planted.u[:, 2] == 1.0).any()
        for b, row in enumerate(rows):
            for t in (0, 1, 2):
                z = planted.z[b, :, t]
                k32 = S.kept_set_fp32(z, *row)
                assert np.array_equal(k32, planted.keep[b, t]), (Q, i, row, t)
                assert S.planted_clean(z, *row, planted.u[b, t:t + 1])
            # the whole draw list on one shuffle: every kept class with q >= 1e-4 is drawn exactly once, nothing else is
            z = planted.z[b, :, 0]
            p, keep, q, _ = S.restate(z, *row)
            us = C.draw_list(q, keep)
            assert S.planted_clean(z, *row, us), S.planted_faults(z, *row, us)
            mid = us[3 if us[2] == 1.0 else 2:]
            want = S.draws(q, keep, mid.astype(np.float64))
            assert np.array_equal(want, np.nonzero(keep & (q >= 1e-4))[0])
            assert np.array_equal(S.restate_fp32(z, *row, us=mid)[3], want)
            first, last = np.nonzero(keep)[0][[0, -1]]
            assert [S.draw(q, keep, 0.0), S.draw(q, keep, 2.0)] == [first, last]
            if row[2] < 1.0:
                nk = row[1] if 0 < row[1] < Q else Q
                ps = p[S.order_of(p)][:nk]
                closest = min(closest, np.abs(np.cumsum(ps / ps.sum()) - row[2]).min())
    print('Q %d: %d rows, a prefix mass comes no closer to top_p than %.3g' % (Q, n_rows, closest))
    assert closest >= 5e-5


@pytest.mark.parametrize('Q', C.QS)
def test_wrong_evaluations_are_told_apart(Q):
    """Each wrong evaluation gives another kept set or another index than the right one on at least one case of this Q (on
    positions 0..2: u = 0, 2, 1 / the first midpoint; shuffles 0..2), and the right one is the float64 restatement."""
    told = {}
    for st, row in cases(Q):
        planted = C.plant(st, [row], 3)
        for t in range(3):
            z, u = planted.z[0, :, t], planted.u[0, t:t + 1]
            _, keep, _, idx = S.restate_fp32(z, *row, us=u)
            assert np.array_equal(keep, planted.keep[0, t]) and idx[0] == planted.idx[0, t]
            for wrong in S.WRONG:
                if wrong in told:
                    continue
                _, wkeep, _, widx = S.restate_fp32(z, *row, us=u, wrong=wrong)
                if not np.array_equal(wkeep, keep) or widx[0] != idx[0]:
                    told[wrong] = 'staircase %d %s, settings %s, shuffle %d, u %g' % (st.index, st.counts, row, t, u[0])
    print('\n'.join('Q %d  %-22s %s' % (Q, w, told[w]) for w in S.WRONG if w in told))
    applies = [w for w in S.WRONG if w != 'lane_tail_dropped' or Q % 64]
    assert [w for w in applies if w not in told] == []
    assert ('lane_tail_dropped' in told) == bool(Q % 64)


@pytest.mark.parametrize('Q', C.QS)
def test_fp32_edge_would_have_excused_the_tie_cases(Q):
    """The continuous-logits tests excuse a decision when fp32_edge flags it, and it flags every tie at a cut: these are the
    cases no test held the kernels to.  (planted_clean and fp32_edge are different predicates on purpose.)"""
    excused = ties = 0
    for st, row in cases(Q):
        z = C.logits(st, 0)
        p, keep, q, _ = S.restate(z, *row)
        ps = p[S.order_of(p)]
        n = int(keep.sum())
        if n < Q and ps[n - 1] == ps[n]:                     # the cut goes through a plateau
            ties += 1
            assert S.planted_clean(z, *row, [0.0, 2.0])
            excused += S.fp32_edge(p, keep, q, row[1], row[2], -1.0)
    print('Q %d: %d tie cases, fp32_edge flags %d of them' % (Q, ties, excused))
    assert ties >= 3 and excused >= 1
