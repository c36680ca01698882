"""The inputs of tests/test_gpu_nbr_select.py and tests/test_gpu_nbr_walk.py can fail a wrong kernel (no GPU): with tests/nbr_ref.py
alone, every builder of tests/nbr_cases.py gives the property its GPU test relies on -- the byte at which the radix select stops, the
classes of non-finite sums and where k cuts them, the candidate counts around k, sums whose bits change when the two lists on either
side of a staging boundary change places, and the kernel form that the header's bound gives every query in every form of a case."""
import math
import struct

import numpy as np
import pytest

import nbr_cases as C
import nbr_ref as R

ALL_CASES = C.SELECT_CASES + C.WALK_CASES + ("full_tables",)
NEG_ZERO = struct.unpack("<Q", struct.pack("<d", -0.0))[0]


def ranked(case, t):
    return sorted(case.candidates(t), key=lambda e: R.order_key(*e))


def test_stop_depth_is_where_the_kth_and_the_next_key_part():
    """the model against its definition: in descending order of the 96-bit keys, the highest byte in which the k-th key and the
    (k + 1)-th differ"""
    rng = np.random.default_rng(1)
    special = [0.0, -0.0, math.inf, -math.inf, math.nan, 1.0, -1.0, 1.0 + 2.0 ** -52, 2.0 ** -1074]
    for trial in range(60):
        n = int(rng.integers(2, 40))
        items = rng.choice([300, 70000, C.MAX_ITEMS][trial % 3], n, replace=False)
        pool = special + list(rng.integers(-3, 4, 5).astype(float)) + list(rng.standard_normal(4))
        cands = [(int(j), float(pool[int(rng.integers(len(pool)))])) for j in items]
        order = sorted(cands, key=lambda e: R.order_key(*e))
        keys = [C.key96(*e) for e in order]
        assert keys == sorted(keys, reverse=True) and len(set(keys)) == n  # the integer keys restate the call's total order
        for k in range(1, n + 2):
            want = None if k >= n else max(d for d in range(12) if (keys[k - 1] ^ keys[k]) >> 8 * d & 255)
            assert C.stop_depth(cands, k) == want, (cands, k)
    assert C.sum_key(-0.0) == C.sum_key(0.0) == 1 << 63 and C.sum_key(math.nan) == 0 < C.sum_key(-math.inf)


def test_every_stop_depth_is_reached():
    reached = {}
    for name in C.DEPTH_CASES:
        case = C.case(name)
        assert len(case.candidates(0)) == C.DEPTH_ITEMS
        depths = case.depths()
        assert set(depths.values()) == {case.notes["depth"]}, (name, depths)
        reached[name] = case.notes["depth"]
    assert set(reached.values()) == set(range(12)), reached
    assert max(int(r.max()) for r in C.case("item_byte_3").hop2.rows) == 671088640 and C.case("item_byte_3").n_items == 2 ** 31 - 1
    for b in range(6):  # the two addends of a sum are exact, and so is the sum
        s = R.sums(C.case("sum_byte_%d" % b).hop1, C.case("sum_byte_%d" % b).hop2, 0)
        assert all(s[i].hex() == (1.0 + (i + 1) * 2.0 ** (8 * b - 52)).hex() and 1.0 < s[i] < 2.0 for i in range(C.DEPTH_ITEMS))


def test_plateaus():
    case = C.case("plateau_300")
    cand = case.candidates(0)
    assert len(cand) == 300 > 256 and len(set(s for _, s in cand)) == 1
    assert case.depths() == {(0, 256): 1, (0, 1): 0, (0, 255): 0}  # all eight sum bytes are walked
    assert min(j for j, _ in cand) < 256 < max(j for j, _ in cand) < 65536  # the items span two bytes
    case = C.case("tie_straddle")
    order = ranked(case, 0)
    assert [s for _, s in order] == [2.0] * 10 + [1.0] * 30 + [0.5] * 20
    tie = [j for j, s in order if s == 1.0]
    assert tie == sorted(tie) and tie[0] < 256 and tie[-1] >= 1024  # the group spans two item bytes
    assert case.depths() == {(0, 25): 0, (0, 26): 1, (0, 10): 11, (0, 40): 10}
    case = C.case("unweighted")
    assert case.hop1.weights is None and case.hop2.weights is None
    assert any(len(set(r.tolist())) < len(r) for r in case.hop2.rows) and any(len(set(r.tolist())) < len(r) for r in case.hop1.rows)
    deep = 0
    for t in range(len(case.rows)):
        cand = case.candidates(t)
        assert all(s == int(s) and 1 <= s <= 60 for _, s in cand)
        order = ranked(case, t)
        deep += len(order) > 10 and order[9][1] == order[10][1]
    assert deep >= 5 and min(d for (t, k), d in case.depths().items() if k == 10) <= 3  # ties straddle the cut: item bytes decide


def test_nonfinite_classes_and_cuts():
    case = C.case("nonfinite")
    counts = case.notes["counts"]
    order = ranked(case, 0)
    cls = [C.sum_class(s) for _, s in order]
    assert cls == [c for c in C.NONFINITE_CLASSES for _ in range(counts[c])]  # the classes in the call's order, NaN last
    numbers = len(cls) - counts["nan"]
    assert {k: (cls[k - 1], cls[k]) for k in case.ks[:3]} == {3: ("+inf", "+inf"), numbers: ("-inf", "nan"), numbers + 2: ("nan", "nan")}
    for group in C.NONFINITE_CLASSES:  # equal sums and NaN sums by ascending item, and in no class do the items ascend with the rank
        part = [e for e in order if C.sum_class(e[1]) == group]
        if group in ("+inf", "zero", "-inf", "nan"):
            assert [j for j, _ in part] == sorted(j for j, _ in part)
    assert [j for j, _ in order] != sorted(j for j, _ in order)
    # both ways to a NaN, and both signs of a zero product
    s = R.sums(case.hop1, case.hop2, 0)
    assert all(math.isnan(s[j]) for j in case.hop2.rows[2]) and all(math.isnan(s[j]) for j in case.hop2.rows[3])
    assert list(case.hop1.rows[0]).count(3) == 2 and float(case.hop1.weights[0][2]) == 0.0
    # query 1: the seen row takes some of every class and leaves some; query 2: NaN sums only, cut by k = 4
    hidden = set(case.seen[1])
    for group in C.NONFINITE_CLASSES:
        part = [j for j, sm in order if C.sum_class(sm) == group]
        assert set(part) & hidden and set(part) - hidden, group
    only_nan = ranked(case, 2)
    assert len(only_nan) == 6 and all(math.isnan(sm) for _, sm in only_nan) and case.depths()[2, 4] <= 3
    # -0 == +0 cannot be reached from 0.0 + v: no sum of any case has the bits of -0.0
    for name in ALL_CASES:
        c = C.case(name)
        for t in range(len(c.rows)):
            assert all(struct.unpack("<Q", struct.pack("<d", sm))[0] != NEG_ZERO for _, sm in c.candidates(t)), (name, t)
    for k in case.ks:  # the reference's rows are this ranking
        items, sums, cnt = C.reference("nonfinite", k)
        assert items[0, :cnt[0]].tolist() == [j for j, _ in order[:k]]


@pytest.mark.parametrize("c", sorted(C.COUNT_CASES))
def test_candidate_counts_around_k(c):
    case = C.case("count_%d" % c)
    cand = case.candidates(0)
    assert len(cand) == c and len(set(s for _, s in cand)) == c
    assert len(R.sums(case.hop1, case.hop2, 0)) == c + 3  # three reached items are hidden
    want = {1: (1, 2), 2: (1, 2, 3), 255: (254, 255, 256), 256: (255, 256), 257: (256,)}[c]
    assert case.ks == want == tuple(k for k in (c - 1, c, c + 1) if 1 <= k <= 256)
    for k in case.ks:
        items, sums, cnt = C.reference(case.name, k)
        assert cnt[0] == min(k, c) and (items[0, cnt[0]:] == -1).all() and not sums[0, cnt[0]:].view(np.uint64).any()
        assert (C.stop_depth(cand, k) is not None) == (c > k)


def test_item_extremes():
    case = C.case("item_extremes")
    top = 2 ** 31 - 2
    assert case.n_items == 2 ** 31 - 1 and case.notes["top"] == top
    cands = [dict(case.candidates(t)) for t in range(len(case.rows))]
    assert top in cands[0] and 0 in cands[0] and cands[0][top] == cands[0][0]  # the two ends tie
    assert top not in cands[1] and 0 not in cands[1] and top in case.seen[1]
    assert top in cands[3] and 0 not in cands[3] and top not in cands[5] and 0 in cands[5]
    reached = set(R.sums(case.hop1, case.hop2, case.rows[2]))
    assert set(cands[2]) == reached and not set(case.seen[2]) & reached  # a seen row of unreached items only ...
    assert {x % 512 for x in case.seen[2]} == {j % 512 for j in reached}  # ... on the reached items' residues
    assert {x % 4096 for x in case.seen[2]} == {j % 4096 for j in reached}
    assert ~np.int32(top) == np.iinfo(np.int32).min + 1  # the blocked key beside the free slot's


def test_staging_markers_are_order_sensitive():
    """exchanging the lists at positions c - 1 and c changes the bits of at least a quarter of the sums of the items they share, at
    every planted boundary; every boundary is planted in every row that reaches past it"""
    case = C.case("staging")
    assert tuple(len(r) for r in case.hop1.rows) == C.STAGE_LENGTHS == (255, 256, 257, 512, 513, 769)
    planted = case.notes["planted"]
    assert sorted(planted) == sorted((i, c) for i, n in enumerate(C.STAGE_LENGTHS) for c in C.STAGE_BOUNDARIES if n > c)
    assert {c for _, c in planted} == {256, 512, 768}
    for row, c in planted:
        x, y = case.notes["marker"][c]
        assert {int(case.hop1.rows[row][c - 1]), int(case.hop1.rows[row][c])} == {x, y}
        shared = sorted(set(case.hop2.rows[x].tolist()) & set(case.hop2.rows[y].tolist()))
        assert len(shared) >= 100
        here = R.sums(case.hop1, case.hop2, row)
        there = R.sums(C.exchanged(case.hop1, row, c - 1, c), case.hop2, row)
        changed = sum(here[j].hex() != there[j].hex() for j in shared)
        assert changed >= len(shared) / 4, (row, c, changed, len(shared))
        assert all(abs(here[j]) < 2.0 ** 20 for j in here)  # every 2^40 is taken back: the sums are of the plain lists' order


def test_list_lengths_run_in_their_forms():
    case = C.case("list_lengths")
    n = len(C.LIST_LENGTHS)
    assert C.LIST_LENGTHS == (0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513)
    for i, length in enumerate(C.LIST_LENGTHS):
        assert case.hop1.rows[i].tolist() == [i] and len(case.hop2.rows[i]) == length
        a, mid, b = case.hop1.rows[n + i].tolist()
        assert mid == i and (len(case.hop2.rows[a]), len(case.hop2.rows[b])) == C.FLANKS
        both = set(case.hop2.rows[a].tolist()) | set(case.hop2.rows[b].tolist())
        assert length < 63 or both & set(case.hop2.rows[i].tolist())
    as_built = C.classes(case, "wave")
    assert as_built == ["wave" if C.lengths_wave(length, False) else "mid" for length in C.LIST_LENGTHS] + \
        ["wave" if C.lengths_wave(length, True) else "mid" for length in C.LIST_LENGTHS]
    assert as_built[:n].count("wave") == 12 and as_built[n:].count("wave") == 11  # 512 and 513 alone, 511 too between two lists
    assert C.classes(case, "lds256") == ["mid"] * (2 * n) and C.classes(case, "global") == ["global"] * (2 * n)


def test_neighbours():
    case = C.case("neighbours")
    rows1, rows2 = case.hop1.rows, case.hop2.rows
    empty = {s for s, r in enumerate(rows2) if len(r) == 0}
    assert empty == {0, 5} and case.hop2.weights is None and case.hop1.weights is not None
    assert rows1[0][0] in empty and rows1[1][1] in empty and rows1[2][-1] in empty
    assert all(len(rows1[t]) == 300 for t in (3, 4, 5, 7))
    assert rows1[3][255] in empty and rows1[3][254] not in empty and rows1[3][256] not in empty
    assert rows1[4][256] in empty and rows1[4][255] not in empty
    assert rows1[5][255] in empty and rows1[5][256] in empty
    assert rows1[6][1] == rows1[6][2] and case.hop1.weights[6][1] != case.hop1.weights[6][2]
    assert rows1[7][255] == rows1[7][256] and rows1[7][255] not in empty
    assert set(rows1[8].tolist()) <= empty and set(rows1[9].tolist()) <= empty and len(rows1[9]) == 257
    assert case.candidates(8) == [] and case.candidates(9) == []
    assert rows2[4].tolist().count(7) == 200 and len(rows2[4]) == 203 and rows1[10].tolist() == [4] and 4 in rows1[11].tolist()
    assert len(C.NEIGHBOUR_ROWS) == len(rows1) and C.NEIGHBOUR_ROWS[10] == "one item 200 times"


@pytest.mark.parametrize("name", C.SELECT_CASES + C.WALK_CASES)
def test_forms_put_every_query_in_the_intended_class(name):
    """as built every select case is walked by one wave; 600 unreached seen items make it the 256-thread LDS form, the hook the
    global one; the padding is never reached, so one expectation serves the three forms"""
    case = C.case(name)
    live = [r >= 0 for r in case.rows]
    assert all(live)
    if name != "list_lengths":
        assert C.classes(case, "wave") == ["wave"] * len(live), C.classes(case, "wave")
    assert C.classes(case, "lds256") == ["mid"] * len(live), C.classes(case, "lds256")
    assert C.classes(case, "global") == ["global"] * len(live)
    named = set(int(j) for r in case.hop2.rows for j in r)
    for form in ("lds256", "global"):
        n_items, seen, _ = C.in_form(case, form)
        pad = C.pad_items(case, C.PAD[form])
        assert len(set(pad)) == C.PAD[form] and not set(pad) & named and max(pad) < n_items <= C.MAX_ITEMS
        assert all(s[-len(pad):] == pad and s[:-len(pad)] == case.seen_of(t) for t, s in enumerate(seen))
        assert max(np.bincount(np.array(pad) % 512)) <= 4  # no long chain of congruent seen items


def test_table_class_is_the_planners():
    assert [C.table_class(b) for b in (0, 511, 512, 4095, 4096, 13055, 13056)] == ["wave", "wave", "mid", "mid", "max", "max", "global"]
    assert [C.table_class(b, 1) for b in (0, 1, 2, 600)] == ["wave", "wave", "global", "global"]
    assert [C.table_class(b, 4096) for b in (511, 512, 4095, 4096)] == ["wave", "mid", "mid", "global"]
    assert [C.table_class(b, 512) for b in (511, 512)] == ["wave", "global"]


def test_full_tables_sit_on_the_class_limits():
    case = C.case("full_tables")
    assert C.bounds(case, case.n_items, case.seen) == case.notes["bounds"] == [511, 512, 4095, 4096, 13055, 13056]
    assert C.classes(case, "wave") == case.notes["classes"] == ["wave", "mid", "mid", "max", "max", "global"]
    reached = set(R.sums(case.hop1, case.hop2, 0))
    assert len(reached) == C.FULL_REACHED
    for s in case.seen:  # distinct, never reached, spread over the residues of every table size
        assert len(set(s)) == len(s) and not set(s) & reached
        for slots in (512, 4096, 13056):
            assert max(np.bincount(np.array(s) % slots)) <= 200
    assert len(case.candidates(0)) == C.FULL_REACHED > max(case.ks)


@pytest.mark.parametrize("name", ALL_CASES)
def test_weighted_hop2_rows_have_distinct_indices(name):
    case = C.case(name)
    if case.hop2.weights is not None:
        assert all(len(set(r.tolist())) == len(r) for r in case.hop2.rows)
    hi = max((int(r.max()) for r in case.hop2.rows if len(r)), default=0)
    assert 0 <= hi < case.n_items and all(0 <= x < case.n_items for s in (case.seen or []) for x in s)
    assert all(int(r.max()) < len(case.hop2.rows) for r in case.hop1.rows if len(r))
    for w in (case.hop1.weights or []) + (case.hop2.weights or []):
        assert np.isfinite(w).all()  # set_table takes finite raw weights only
