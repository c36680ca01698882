"""gorse_nbr_recommend's walk at its edges (csrc/nbr_recommend.hip: 256 hop-1 entries staged at a time, one list fetched ahead, 64 or
256 threads per query): hop-1 rows that end at and next to the staging chunks with order-sensitive lists on either side of a
boundary, hop-2 lists of every length around the thread counts, empty lists and repeated sources where the prefetch looks, a seen
row pointer that does not start at 0, tables filled to their last slot at the real class limits.  tests/nbr_cases.py builds the
inputs, tests/test_nbr_cases_cpu.py shows what they reach; everything is held against tests/nbr_ref.py bit for bit."""
import numpy as np
import pytest

import nbr_cases as C
import nbr_ref as R
from gorse_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _hooks_at_default():
    yield
    capi.set_nbr(0, 0)


@pytest.mark.parametrize("form", C.FORMS)
def test_staging_boundaries(form):
    C.run_case("staging", form)


@pytest.mark.parametrize("form", C.FORMS)
def test_list_lengths_at_the_thread_count_edges(form):
    got = C.run_case("list_lengths", form)  # its recommend_stats: as built 28 LDS tables, 23 of them one wave's (the CPU test), else 0
    n = len(C.LIST_LENGTHS)
    assert got[256][2][:n].tolist() == [min(length, 256) for length in C.LIST_LENGTHS]


@pytest.mark.parametrize("form", C.FORMS)
def test_awkward_neighbours(form):
    got = C.run_case("neighbours", form)
    cnt = got[256][2]
    assert cnt[8] == 0 and cnt[9] == 0 and cnt[10] == 3 and (cnt[:8] > 0).all()  # rows of empty lists only; item 9 of list 4 is seen


@pytest.mark.parametrize("form", C.FORMS)
def test_seen_pointer_that_starts_past_zero(form):
    """seen_indptr[0] = 5 with five items before it that would hide the best candidates if they were read"""
    case = C.case("neighbours")
    n_items, seen, hook = C.in_form(case, form)
    want = C.reference("neighbours", 5)
    junk = [int(j) for j in want[0][0]]
    assert len(junk) == 5 and min(junk) >= 0
    sp, si = R.seen_csr(seen)
    assert sp[0] == 0 and sp[-1] == si.size > 0
    capi.set_nbr(hook, 0)
    h = capi.NbrRecommender(n_items)
    case.hop1.set_on(h, R.HOP1)
    case.hop2.set_on(h, R.HOP2)
    zero_based = h.recommend(case.rows, 5, sp, si)
    offset = h.recommend(case.rows, 5, sp + 5, np.concatenate([np.array(junk, np.int32), si]))
    R.assert_same(offset, want, ("offset", form))
    R.assert_same(offset, zero_based, ("offset against zero-based", form))


def test_full_tables_at_the_class_limits():
    """bound + 1 == slots at 512, 4096 and 13056 slots and one entry more: as built (five LDS tables, one global), and each pair
    again with the hook at the limit, where the larger of the two goes to global scratch"""
    case = C.case("full_tables")
    sp, si = R.seen_csr(case.seen)
    h = capi.NbrRecommender(case.n_items)
    case.hop1.set_on(h, R.HOP1)
    case.hop2.set_on(h, R.HOP2)
    for k in case.ks:
        want = C.reference("full_tables", k)
        R.assert_same(h.recommend(case.rows, k, sp, si), want, ("as built", k))
        assert h.recommend_stats()[:2] == (5, 1)
        assert (want[2] == k).all() and all(np.array_equal(want[0][t], want[0][0]) for t in range(6))  # the seen rows hide nothing
    want = C.reference("full_tables", 256)
    for i, limit in enumerate((C.WAVE_SLOTS, C.MID_SLOTS, C.MAX_SLOTS)):
        capi.set_nbr(limit, 0)
        pair = slice(2 * i, 2 * i + 2)
        psp, psi = R.seen_csr(case.seen[pair])
        R.assert_same(h.recommend(case.rows[pair], 256, psp, psi), tuple(a[pair] for a in want), ("limit", limit))
        assert h.recommend_stats()[:2] == (1, 1), limit
