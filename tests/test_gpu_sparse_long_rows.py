"""GPU parity: the sparse exact top-k at REAL lengths -- the paths that the thresholds' test hooks cannot shrink (csrc/sparse.hip,
csrc/sparse_kernels.hpp): stored rows of more than 1024 entries under a heavy query (the whole-wave walk of sparse_rows_kernel, both
summation forms of a 64-entry step), calls of several launch rounds (run_queries), a directory scan with two chunk sums per thread
(sparse_scan_top_kernel), and the thresholds in force without any hook (split 2048, heavy 16384, the front chosen at creation).
Everything bit for bit against the oracle's merge-order sparse dot (sparse_cases.check_against_oracle) or between two configurations of
the library (_same); Sparse.path_stats() shows that a test ran the path it is named after.  The collections L, B and W are built in
tests/sparse_cases.py; tests/test_sparse_long_cases_cpu.py shows that they can fail a wrong kernel.

Wall time of each test on an MI355X (pytest --durations, seconds; the whole module 1.9):
    test_heavy_searches_meet_long_rows                           0.37 (the first test also loads the library), 0.06
    test_all_pairs_with_long_rows_as_front_and_heavy_queries     0.10, 0.10
    test_production_thresholds_without_any_hook                  0.16, 0.16
    test_production_thresholds_search_with_a_mask                0.04
    test_index_construction_over_a_wide_directory                0.18 + 0.08 for W's handle, which the next two share
    test_all_pairs_in_several_launch_rounds                      0.15
    test_search_in_several_launch_rounds                         0.08
"""
import numpy as np
import pytest

import sparse_cases as SC
from gorse_amd import capi
from sparse_cases import check_against_oracle as check, rows_of, rows_with_lengths

pytestmark = pytest.mark.gpu


@pytest.fixture
def hooks():
    L = capi.lib()
    yield L
    L.gorse_hip_test_set_sparse_sym(-1, 0, 0, 0)
    L.gorse_hip_test_set_sparse_front(1)
    L.gorse_hip_test_set_sparse_slots(0)
    L.gorse_hip_test_set_sparse_head(-1)
    L.gorse_hip_test_set_sparse_tile(0)
    L.gorse_hip_test_set_sparse_split(2048)
    L.gorse_hip_test_set_sparse_heavy(16384)
    L.gorse_hip_test_set_sparse_atomic(-1)


def _bits(x):
    return x.view(np.uint32) if x.dtype == np.float32 else x


def _same(x, y):
    for a, b in zip(x, y):
        assert np.array_equal(_bits(a), _bits(b))


def _both(hooks, s, k):
    """(unsymmetric, symmetric) results of all_pairs(k) and the path statistics of each"""
    hooks.gorse_hip_test_set_sparse_sym(0, 0, 0, 0)
    plain = s.all_pairs(k)
    assert s.sym_stats()[0] == 0
    st_plain = s.path_stats()
    hooks.gorse_hip_test_set_sparse_sym(-1, 0, 0, 0)
    sym = s.all_pairs(k)
    assert s.sym_stats()[0] == 1
    return plain, sym, st_plain, s.path_stats()


# ---- (a) heavy searches meet long rows ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("long_row_last", [False, True])
def test_heavy_searches_meet_long_rows(oracle, hooks, long_row_last):
    """Queries of 30 .. 4096 entries over L's 4096 dims and the hand-built one (16 / 17 / 64 / 0 / ... / 1 matches per step of the
    1089-entry row) with split = heavy = 40: every query but the first is scored row by row against its dense copy, and the eleven rows
    past 1024 entries are walked by the whole wave -- about 5 matches per step (one readlane per match), about 31 (all 64 lanes added,
    -0 where a lane has no match), about 16 (both forms within a row).  k = 1024 >= N compares the bits of every non-zero row.  Plain,
    masked, with exclusions that name long rows; on the copy of L that ends with a long row (the look-ahead of its last step reads at
    the arrays' end); and the same queries as split items through the list walk (heavy = 0)."""
    ptr, idx, val, long_rows = SC.long_rows_case(long_row_last=long_row_last)
    qp, qi, qv = SC.long_rows_queries(ptr, idx, val, long_rows)
    nq = qp.size - 1
    queries = rows_of(qp, qi, qv, range(nq))
    n_heavy = int((np.diff(qp) > SC.L_THRESHOLD).sum())
    assert n_heavy == nq - 1 == 6
    rng = np.random.default_rng(40)
    mask = (rng.random(ptr.size - 1) < 0.8).astype(np.uint8)
    mask[long_rows] = 1
    mask[[long_rows[1], long_rows[4], long_rows[9]]] = 0  # 1025, 1088 and 4096 entries
    excl = np.array([long_rows[(3 * t) % 12] for t in range(nq)], np.int64)  # 1024, 1087, 1500, 4096, ... entries
    excl[2] = -1
    hooks.gorse_hip_test_set_sparse_split(SC.L_THRESHOLD)
    hooks.gorse_hip_test_set_sparse_heavy(SC.L_THRESHOLD)
    s = capi.Sparse(ptr, idx, val)
    for k in (1024, 5):
        hooks.gorse_hip_test_set_sparse_heavy(SC.L_THRESHOLD)
        got = s.search(qp, qi, qv, k)
        print("path_stats (rounds, heavy queries, row ranges, directory cells), k = %d:" % k, s.path_stats())
        assert s.path_stats()[:2] == (1, n_heavy)
        check(oracle, ptr, idx, val, k, got, queries, [-1] * nq)
        with_excl = s.search(qp, qi, qv, k, exclude=excl)
        check(oracle, ptr, idx, val, k, with_excl, queries, list(excl))
        s.set_mask(mask)
        masked = s.search(qp, qi, qv, k, exclude=excl)
        assert s.path_stats()[:2] == (1, n_heavy)
        check(oracle, ptr, idx, val, k, masked, queries, list(excl), mask)
        s.set_mask(None)
        one = s.search(qp[-2:] - qp[-2], qi[qp[-2]:], qv[qp[-2]:], k)  # a single heavy query in a call of its own
        assert s.path_stats()[:2] == (1, 1)
        _same([x[-1:] for x in got], one)
        hooks.gorse_hip_test_set_sparse_heavy(0)  # split items through the list walk
        _same(got, s.search(qp, qi, qv, k))
        assert s.path_stats()[:2] == (1, 0)
        _same(with_excl, s.search(qp, qi, qv, k, exclude=excl))
    s.close()


# ---- (b) all pairs over L in both forms -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 100])
def test_all_pairs_with_long_rows_as_front_and_heavy_queries(oracle, hooks, k):
    """Rows of 256 per group, front = split = heavy = 1000: L's twelve long rows are the front and every one is a heavy query (more than
    the kernel's eight queues, not a multiple of eight), each walking the other eleven with the whole wave.  k = 3: the front delivers
    (2 * 12 >= 5 * 3) and sparse_rows_kernel writes the front's score matrix from long rows; k = 100: it does not.  Unsymmetric,
    symmetric and the oracle over all 600 rows; a query range that cuts through the long rows."""
    ptr, idx, val, long_rows = SC.long_rows_case()
    N = ptr.size - 1
    hooks.gorse_hip_test_set_sparse_tile(256)
    hooks.gorse_hip_test_set_sparse_front(1000)
    hooks.gorse_hip_test_set_sparse_split(1000)
    hooks.gorse_hip_test_set_sparse_heavy(1000)
    s = capi.Sparse(ptr, idx, val)
    plain, sym, st_plain, st_sym = _both(hooks, s, k)
    print("path_stats (rounds, heavy queries, row ranges, directory cells): unsymmetric", st_plain, "symmetric", st_sym)
    assert st_plain[:2] == (1, 12) and st_sym[:2] == (1, 12)
    _same(plain, sym)
    check(oracle, ptr, idx, val, k, sym, rows_of(ptr, idx, val, range(N)), list(range(N)))
    by_row = sorted(long_rows)
    q0, q1 = by_row[3], by_row[8] + 1  # six long rows inside (both ends are long rows), six outside
    got = s.all_pairs(k, q0, q1)
    assert s.path_stats()[:2] == (1, 6) and s.sym_stats()[0] == 0
    check(oracle, ptr, idx, val, k, got, rows_of(ptr, idx, val, range(q0, q1)), list(range(q0, q1)))
    s.close()


# ---- (c) no hook at all ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def production_case():
    ptr, idx, val = SC.production_thresholds_case()
    lens = np.diff(ptr)
    sample = sorted(set(np.nonzero(lens > 1024)[0].tolist()) | set(range(0, lens.size, 60)))
    return ptr, idx, val, sample


@pytest.mark.parametrize("k", [10, 100])
def test_production_thresholds_without_any_hook(oracle, hooks, production_case, k):
    """B under the thresholds in force without a hook: eleven rows past 16384 entries are heavy queries, 44 rows past 2048 the front chosen
    at creation and the split queries of both forms (k = 10: the front delivers, 2 * 44 >= 5 * 10; k = 100: it does not); more row ranges
    than row groups, so the partial rankings are strided by ranges.  Symmetric against unsymmetric, the oracle on every row past 1024
    entries and every 60th row."""
    ptr, idx, val, sample = production_case
    s = capi.Sparse(ptr, idx, val)
    sym = s.all_pairs(k)
    rounds, heavy, n_ranges, cells = s.path_stats()
    print("path_stats (rounds, heavy queries, row ranges, directory cells):", s.path_stats())
    assert s.sym_stats()[0] == 1 and (rounds, heavy) == (1, 11)
    groups = cells // SC.B_DIMS
    assert cells == groups * SC.B_DIMS and groups == 3 and n_ranges > groups  # (2149 rows + the phantom ids behind the front, 2048 per group)
    hooks.gorse_hip_test_set_sparse_sym(0, 0, 0, 0)
    plain = s.all_pairs(k)
    assert s.sym_stats()[0] == 0 and s.path_stats()[:2] == (1, 11)
    _same(plain, sym)
    check(oracle, ptr, idx, val, k, [x[sample] for x in sym], rows_of(ptr, idx, val, sample), sample)
    s.close()


def test_production_thresholds_search_with_a_mask(oracle, hooks, production_case):
    """five queries of 10, 3000, 16384, 16385 and 20000 entries over B, no hook: one whole-query item, two split queries (16384 is not past
    the heavy threshold), two heavy ones; a mask that hides some of the longest rows"""
    ptr, idx, val, _ = production_case
    rng = np.random.default_rng(20000)
    qp, qi, qv = rows_with_lengths(rng, SC.B_DIMS, [10, 3000, 16384, 16385, 20000])
    mask = (rng.random(ptr.size - 1) < 0.7).astype(np.uint8)
    longest = np.argsort(-np.diff(ptr), kind="stable")[:12]
    mask[longest] = 1
    mask[longest[[0, 3, 7]]] = 0
    s = capi.Sparse(ptr, idx, val)
    s.set_mask(mask)
    for k in (7, 300):
        got = s.search(qp, qi, qv, k)
        print("path_stats (rounds, heavy queries, row ranges, directory cells):", s.path_stats())
        assert s.path_stats()[:2] == (1, 2)
        check(oracle, ptr, idx, val, k, got, rows_of(qp, qi, qv, range(5)), [-1] * 5, mask)
    s.close()


# ---- (d), (e) a wide directory, several launch rounds -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide():
    """W under rows of 256 per group and every other switch at its default: the handle, its all_pairs(100) as ONE launch round, and a
    sample of rows -- every 200th, and by length rank (rows are numbered longest first: the row groups, and the launch rounds of the
    long queries, follow that order) the first, a middle and the last row group / the first, a middle and the last round, short rows"""
    ptr, idx, val, shared = SC.wide_directory_case()
    lens = np.diff(ptr)
    distinct = np.unique(idx)
    n_long = int((lens > SC.W_LONG).sum())
    L = capi.lib()
    L.gorse_hip_test_set_sparse_tile(256)
    try:
        s = capi.Sparse(ptr, idx, val)
    finally:
        L.gorse_hip_test_set_sparse_tile(0)
    one_round = s.all_pairs(100)
    stats = s.path_stats()
    # long queries per round of a call with k <= 128: at most the dense copies' bound; the handle's row ranges may lower it
    bound = SC.launch_round_bound(distinct.size, 47, stats[2], 100)
    assert bound <= SC.dense_copy_bound(distinct.size)
    by_len = np.argsort(-lens, kind="stable")
    ranks = [0, 1, 255, 256, bound - 1, bound, 3 * bound + 5, 6000, n_long - 1, n_long, SC.W_ROWS - 256, SC.W_ROWS - 1]
    sample = sorted(set(range(0, SC.W_ROWS, 200)) | set(int(by_len[r]) for r in ranks))
    case = dict(ptr=ptr, idx=idx, val=val, shared=shared, distinct=distinct, bound=bound, n_long=n_long, sample=sample, s=s,
                one_round=one_round, one_round_stats=stats, one_round_sym=s.sym_stats()[0])
    yield case
    s.close()


def test_index_construction_over_a_wide_directory(oracle, hooks, wide):
    """more than 1024 x 8192 directory cells: sparse_scan_top_kernel adds two chunk sums per thread.  A wrong directory offset anywhere
    moves postings between lists, which the bits of the sampled rows (first, middle and last row group) and of the searches show."""
    ptr, idx, val, s = wide["ptr"], wide["idx"], wide["val"], wide["s"]
    rounds, heavy, n_ranges, cells = wide["one_round_stats"]
    print("path_stats (rounds, heavy queries, row ranges, directory cells):", wide["one_round_stats"])
    assert cells > 8388608 and cells == wide["distinct"].size * 47
    assert (rounds, heavy) == (1, 0) and wide["one_round_sym"] == 1
    sample = wide["sample"]
    check(oracle, ptr, idx, val, 100, [x[sample] for x in wide["one_round"]], rows_of(ptr, idx, val, sample), sample)
    rng = np.random.default_rng(47)
    private = np.setdiff1d(wide["distinct"], wide["shared"])
    nobody = np.setdiff1d(np.arange(SC.W_SPACE, dtype=np.uint32), wide["distinct"])
    rows = []
    for t in range(40):  # private indices from all over the directory (its first and last cells among them), shared ones, unknown ones
        own = rng.choice(private, int(rng.integers(5, 30)), replace=False)
        if t < 4:
            own = np.union1d(own, [private[0], private[-1], wide["distinct"][0], wide["distinct"][-1]])
        rows.append(np.unique(np.concatenate([own, rng.choice(wide["shared"], int(rng.integers(0, 6)), replace=False),
                                              rng.choice(nobody, int(rng.integers(0, 3)), replace=False)])).astype(np.uint32))
    qp = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int64)
    qi = np.concatenate(rows)
    qv = ((rng.random(qi.size) + 0.05) * rng.choice(np.array([-1.0, 1.0]), qi.size)).astype(np.float32)
    got = s.search(qp, qi, qv, 50)
    assert s.path_stats()[:2] == (1, 0)
    check(oracle, ptr, idx, val, 50, got, rows_of(qp, qi, qv, range(40)), [-1] * 40)


def test_all_pairs_in_several_launch_rounds(oracle, hooks, wide):
    """split 20: more long queries than a launch round holds partial rankings and dense copies for (sparse_cases.launch_round_bound):
    the rounds' partial rankings use round-local slots, the short queries go into round 0 only, no plan is kept.  Same bits as the
    one-round call."""
    ptr, idx, val, s = wide["ptr"], wide["idx"], wide["val"], wide["s"]
    want_rounds = -(-wide["n_long"] // wide["bound"])
    assert want_rounds >= 3 and wide["n_long"] % wide["bound"] != 0
    hooks.gorse_hip_test_set_sparse_split(SC.W_LONG)
    hooks.gorse_hip_test_set_sparse_heavy(0)
    hooks.gorse_hip_test_set_sparse_sym(0, 0, 0, 0)
    plain = s.all_pairs(100)
    print("long queries %d, per round %d; path_stats (rounds, heavy queries, row ranges, directory cells):" % (wide["n_long"], wide["bound"]),
          s.path_stats())
    assert s.sym_stats()[0] == 0 and s.path_stats()[:2] == (want_rounds, 0)
    _same(wide["one_round"], plain)
    _same(plain, s.all_pairs(100))  # the same call again: its plan was not kept
    assert s.path_stats()[0] == want_rounds
    hooks.gorse_hip_test_set_sparse_sym(-1, 0, 0, 0)
    sym = s.all_pairs(100)
    print("symmetric: path_stats", s.path_stats())
    assert s.sym_stats()[0] == 1 and s.path_stats()[0] >= 2
    _same(wide["one_round"], sym)
    sample = wide["sample"]
    check(oracle, ptr, idx, val, 100, [x[sample] for x in plain], rows_of(ptr, idx, val, sample), sample)


def test_search_in_several_launch_rounds(oracle, hooks, wide):
    """700 queries of 25 entries, which are long queries (split 20) that are not stored rows: two rounds, split_t of the second one
    uploaded from behind the first one's queries"""
    ptr, idx, val, s = wide["ptr"], wide["idx"], wide["val"], wide["s"]
    bound = wide["bound"]
    assert bound < 700 < 2 * bound
    rng = np.random.default_rng(700)
    private = np.setdiff1d(wide["distinct"], wide["shared"])
    rows = [np.sort(np.concatenate([rng.choice(private, 21, replace=False), rng.choice(wide["shared"], 4, replace=False)]))
            for _ in range(700)]
    qp = np.arange(701, dtype=np.int64) * 25
    qi = np.concatenate(rows).astype(np.uint32)
    qv = ((rng.random(qi.size) + 0.05) * rng.choice(np.array([-1.0, 1.0]), qi.size)).astype(np.float32)
    excl = rng.integers(-1, SC.W_ROWS, 700).astype(np.int64)
    hooks.gorse_hip_test_set_sparse_split(SC.W_LONG)
    hooks.gorse_hip_test_set_sparse_heavy(0)
    got = s.search(qp, qi, qv, 10, exclude=excl)
    print("path_stats (rounds, heavy queries, row ranges, directory cells):", s.path_stats())
    assert s.path_stats()[:2] == (2, 0)
    hooks.gorse_hip_test_set_sparse_split(0)
    _same(got, s.search(qp, qi, qv, 10, exclude=excl))  # whole-query items, one round
    assert s.path_stats()[:2] == (1, 0)
    sample = sorted(set(range(0, 700, 25)) | {bound - 1, bound, bound + 1, 699})
    check(oracle, ptr, idx, val, 10, [x[sample] for x in got], rows_of(qp, qi, qv, sample), [int(excl[t]) for t in sample])
