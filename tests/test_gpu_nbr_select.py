"""gorse_nbr_recommend's selection at its edges (csrc/nbr_recommend.hip: a radix select over 96-bit keys, sum key | ~item): a stop at
every byte of the key, plateaus of equal sums beyond the survivor buffer, sums of +inf, -inf, NaN and zero, candidate counts around
k, items next to 2^31 - 1.  tests/nbr_cases.py builds the inputs, tests/test_nbr_cases_cpu.py shows what they reach; every case runs
as one wave per query, as a 256-thread workgroup over an LDS table and over a table in global scratch, and is held against
tests/nbr_ref.py in items, counts, padding and every sum's bits."""
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
@pytest.mark.parametrize("name", C.DEPTH_CASES)
def test_select_stops_at_every_byte(name, form):
    C.run_case(name, form)


@pytest.mark.parametrize("form", C.FORMS)
@pytest.mark.parametrize("name", ["plateau_300", "tie_straddle", "unweighted"])
def test_plateaus(name, form):
    got = C.run_case(name, form)
    if name == "plateau_300":  # 256 of 300 equal sums: the smallest items in ascending order
        items, sums, cnt = got[256]
        assert cnt[0] == 256 and items[0].tolist() == (7 + 13 * np.arange(256)).tolist() and (sums[0] == 1.0).all()


@pytest.mark.parametrize("form", C.FORMS)
def test_nonfinite_sums(form):
    got = C.run_case("nonfinite", form)
    items, sums, cnt = got[40]
    assert cnt.tolist() == [32, 25, 6]
    assert [C.sum_class(s) for s in sums[0, :32]] == [c for c in C.NONFINITE_CLASSES for _ in range(C.case("nonfinite").notes["counts"][c])]
    assert not np.signbit(sums[0, 11:17]).any()  # the zero sums are +0.0
    assert np.isnan(got[28][1][0, 26:]).all() and np.isneginf(got[26][1][0, 25]) and np.isposinf(got[3][1][0]).all()


@pytest.mark.parametrize("form", C.FORMS)
@pytest.mark.parametrize("c", sorted(C.COUNT_CASES))
def test_candidate_counts_around_k(c, form):
    got = C.run_case("count_%d" % c, form)
    for k, (items, sums, cnt) in got.items():
        n = min(k, c)
        assert cnt[0] == n and (items[0, :n] >= 0).all() and (items[0, n:] == -1).all() and not sums[0, n:].view(np.uint64).any()
        assert (np.diff(sums[0, :n]) < 0).all()  # distinct sums, descending


@pytest.mark.parametrize("form", C.FORMS)
def test_item_extremes(form):
    got = C.run_case("item_extremes", form)
    top = C.MAX_ITEMS - 1
    items, sums, cnt = got[256]
    assert items[0, :4].tolist() == [0, 512, 1023, 1 << 30 | 512] and top in items[0] and sums[0, list(items[0]).index(top)] == 1.0
    assert top not in items[1] and 0 not in items[1] and top in items[3] and top not in items[5]
    assert got[1][0][:, 0].tolist() == [0, 512, 0, 7, 0, 7]
