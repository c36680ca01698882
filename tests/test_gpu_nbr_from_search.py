"""gorse_nbr_set_table_from_topk / _from_sparse (csrc/nbr_build.hip): neighbour tables built on the device from a similarity
search's device-resident results.

The yardstick is the host route through public calls only (tests/nbr_build_ref.py): the search to the host, the list rule in Python,
gorse_nbr_set_table on a second handle.  Every case compares the two tables' arrays bit for bit (gorse_nbr_get_table), the lists
gorse_nbr_recommend forms through both handles, and -- with the LDS capacity cut so that the queries split -- the planner's counts,
which rest on the bounds a device-built hop-1 table computes on the device."""
import ctypes as C

import numpy as np
import pytest

import nbr_build_ref as B
import nbr_ref as R
import sparse_cases as SC
from gorse_amd import capi

pytestmark = pytest.mark.gpu

NEG_DOT, EUCLIDEAN, COSINE = capi.METRIC_NEG_DOT, capi.METRIC_EUCLIDEAN, capi.METRIC_COSINE
AUTO, SCAN, MFMA = 0, 1, 2  # gorse_hip_test_set_topk_path; AUTO: fewer than 768 sources scan, and the scan hands its tie queries to the MFMA replay


@pytest.fixture(autouse=True)
def _hooks_at_default():
    yield
    capi.set_nbr(0, 0)
    capi.lib().gorse_hip_test_set_topk_path(0)
    capi.lib().gorse_hip_test_set_scan_block(0)


def bf16(x):
    """float32 -> the bf16 bit patterns of the truncated values"""
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) >> 16).astype(np.uint16)


def other_table(rng, which, n_rows_built, index_n, n_items):
    """the table of the other slot, unweighted: hop 1 over the built hop-2 table's rows, or hop 2 under the built hop-1 table"""
    if which == R.HOP2:
        rows = [rng.integers(0, n_rows_built, int(m)) for m in rng.choice([0, 1, 3, 9, 40], 24)] if n_rows_built else [[]] * 4
        return R.HOP1, R.Table(rows)
    return R.HOP2, R.Table([rng.integers(0, n_items, int(m)) for m in rng.choice([0, 2, 7, 30], index_n)])


def same_tables(dev, host, which, what):
    gp, gi, gw = dev.get_table(which)
    wp, wi, ww = host.get_table(which)
    assert dev.table_info(which) == host.table_info(which) == (wp.size - 1, wi.size, True), what
    assert np.array_equal(gp, wp), (what, "indptr")
    assert np.array_equal(gi, wi), (what, "indices")
    assert np.array_equal(gw.view(np.uint32), ww.view(np.uint32)), (what, "weights")
    return wp, wi, ww


def same_answers(dev, host, n_queries, what, k=10):
    rng = np.random.default_rng(3)
    rows = np.concatenate([np.arange(n_queries), [-1]]).astype(np.int32)
    seen = [rng.integers(0, dev.n_items, int(m)) for m in rng.choice([0, 0, 4], rows.size)]
    sp, si = R.seen_csr(seen)
    for slots in (0, 48):  # 48: the queries split between LDS tables and global ones
        capi.set_nbr(slots, 0)
        R.assert_same(dev.recommend(rows, k, sp, si), host.recommend(rows, k, sp, si), (what, slots))
        assert dev.recommend_stats()[:2] == host.recommend_stats()[:2], (what, slots, dev.recommend_stats(), host.recommend_stats())
    capi.set_nbr(0, 0)


def both_routes(build, lists, sources, index_n, n, positive_only, transform, scale, which, what, n_items=None):
    """build(handle) fills the slot on the device; lists = the host route's searches.  Returns the host route's CSR."""
    n_items = n_items or max(index_n, 50)
    ptr, ix, w = B.table_from_lists(sources, lists, n, positive_only)
    dev, host = capi.NbrRecommender(n_items), capi.NbrRecommender(n_items)
    try:
        build(dev)
        host.set_table(which, ptr, ix, w, transform, scale)
        same_tables(dev, host, which, what)
        slot, tab = other_table(np.random.default_rng(11), which, len(sources), index_n, n_items)
        tab.set_on(dev, slot)
        tab.set_on(host, slot)
        same_answers(dev, host, len(sources) if which == R.HOP1 else len(tab.rows), what)
    finally:
        dev.close()
        host.close()
    return ptr, ix, w


def last_call_scanned(index):
    """did the index's last call run blocks of the scan (gorse_hip_test_topk_scan_flags refuses when it did not)"""
    return capi.lib().gorse_hip_test_topk_scan_flags(index.h, np.zeros(1, np.int32).ctypes.data_as(C.POINTER(C.c_int32)), 0) == capi.OK


def dense_case(X, metric, dtype, path, n, sources=None, positive_only=False, transform=R.RAW, scale=1.0, which=R.HOP2, mask=None,
               scan_block=0, what="", swept_only=False):
    """swept_only: the rows leave the MFMA sweep nothing to hand back to the scan, so the forced path is seen to be the one taken"""
    Xs = bf16(X) if dtype == capi.DTYPE_BF16 else np.ascontiguousarray(X, np.float32)
    index = capi.TopK(Xs, metric, dtype)
    try:
        if mask is not None:
            index.set_mask(mask)
        capi.lib().gorse_hip_test_set_topk_path(path)
        capi.lib().gorse_hip_test_set_scan_block(scan_block)
        src = list(range(index.N)) if sources is None else list(sources)
        lists = B.dense_lists(index, Xs, src, n)

        def build(h):
            h.set_table_from_topk(which, index, n, sources, None, positive_only, transform, scale)
            if path in (AUTO, SCAN) and any(s >= 0 for s in src):  # (every case has fewer than 768 sources)
                assert last_call_scanned(index), what
            if path == MFMA and swept_only:
                assert not last_call_scanned(index), what
        return both_routes(build, lists, src, index.N, n, positive_only, transform, scale, which, (what, metric, dtype, path, n))
    finally:
        index.close()


def gauss(seed, N, d):
    return np.random.default_rng(seed).standard_normal((N, d)).astype(np.float32)


@pytest.mark.parametrize("path", [SCAN, MFMA])
@pytest.mark.parametrize("dtype", [capi.DTYPE_F32, capi.DTYPE_BF16])
@pytest.mark.parametrize("metric,positive_only,transform,scale", [(NEG_DOT, True, R.RAW, 0.5), (EUCLIDEAN, False, R.RECIP, 1.0),
                                                                  (COSINE, False, R.RECIP, 1.0)])
def test_dense_metrics_dtypes_paths(metric, positive_only, transform, scale, dtype, path):
    ptr, ix, w = dense_case(gauss(1, 333, 16), metric, dtype, path, 5, None, positive_only, transform, scale, swept_only=True)
    assert ptr[-1] > 333 and (metric != NEG_DOT or (w > 0).all())


@pytest.mark.parametrize("path", [SCAN, MFMA])
@pytest.mark.parametrize("n", [1, 100])
def test_dense_list_lengths(n, path):
    ptr, _, _ = dense_case(gauss(2, 257, 24), EUCLIDEAN, capi.DTYPE_F32, path, n, which=R.HOP1)
    assert (np.diff(ptr) == n).all()


def test_dense_more_than_one_scan_block_and_mfma_rows():
    X = gauss(3, 900, 8)
    a = dense_case(X, COSINE, capi.DTYPE_F32, SCAN, 5, scan_block=128, what="8 scan blocks")
    b = dense_case(X, COSINE, capi.DTYPE_F32, MFMA, 5, what="900 rows swept", swept_only=True)
    assert all(np.array_equal(x, y) for x, y in zip(a[:2], b[:2]))


@pytest.mark.parametrize("path", [SCAN, MFMA])
def test_dense_fewer_rows_than_n(path):
    ptr, _, _ = dense_case(gauss(4, 40, 8), EUCLIDEAN, capi.DTYPE_F32, path, 100)
    assert (np.diff(ptr) == 39).all()  # every other row, and the row itself dropped


@pytest.mark.parametrize("path", [SCAN, MFMA])
def test_dense_row_absent_from_its_own_list(path):
    """Dot with a few long vectors: a short row's n + 1 best are the long rows, it is not among them, and the cut at n is what
    shortens the list"""
    X = gauss(5, 120, 16)
    X[:8] = 50.0 * np.abs(X[:8])
    X[8:] = 0.1 * np.abs(X[8:])
    ptr, ix, _ = dense_case(X, NEG_DOT, capi.DTYPE_F32, path, 5, positive_only=True)
    assert (np.diff(ptr) == 5).all() and set(ix[ptr[100]:ptr[101]].tolist()) <= set(range(8))


@pytest.mark.parametrize("path", [AUTO, SCAN, MFMA])
def test_dense_duplicate_vectors(path):
    """rows 0..5 are one vector: row s's list starts with six entries at distance 0, and the one dropped is s itself"""
    X = gauss(6, 90, 8)
    X[1:6] = X[0]
    ptr, ix, w = dense_case(X, EUCLIDEAN, capi.DTYPE_F32, path, 7)
    for s in range(6):
        row = ix[ptr[s]:ptr[s + 1]].tolist()
        assert s not in row and set(row[:5]) == set(range(6)) - {s}


def test_dense_positive_only_with_zero_and_negative_products():
    """disjoint supports give inner products of +0 and -0, opposite signs negative ones: none of them survives positive_only"""
    rng = np.random.default_rng(7)
    X = np.zeros((64, 8), np.float32)
    for r in range(64):
        X[r, (r % 4) * 2:(r % 4) * 2 + 2] = rng.choice([-1.0, 1.0]) * (1.0 + rng.random(2))
    index = capi.TopK(X, NEG_DOT)
    _, dist, _ = index.search_vector(X[:8], 64)
    index.close()
    assert (dist == 0).any() and (dist > 0).any() and (dist < 0).any()
    for path in (AUTO, SCAN, MFMA):
        ptr, _, w = dense_case(X, NEG_DOT, capi.DTYPE_F32, path, 63, positive_only=True)
        assert (w > 0).all() and 0 < np.diff(ptr).max() < 63
        ptr, _, w = dense_case(X, NEG_DOT, capi.DTYPE_F32, path, 63, positive_only=False, scale=0.5)
        assert (np.diff(ptr) == 63).all() and (w == 0).any() and (w < 0).any()


@pytest.mark.parametrize("path", [SCAN, MFMA])
def test_dense_mask(path):
    X = gauss(8, 200, 16)
    mask = (np.random.default_rng(8).random(200) < 0.6).astype(np.uint8)
    mask[:3] = (0, 1, 0)  # masked sources among the rows
    ptr, ix, _ = dense_case(X, COSINE, capi.DTYPE_F32, path, 5, mask=mask, which=R.HOP1)
    assert mask[ix].all() and (np.diff(ptr) == 5).all()
    ptr, _, _ = dense_case(X, COSINE, capi.DTYPE_F32, path, 5, mask=np.zeros(200, np.uint8))
    assert ptr[-1] == 0


@pytest.mark.parametrize("path", [SCAN, MFMA])
def test_dense_sources(path):
    X = gauss(9, 150, 8)
    sources = [7, -1, 149, 7, 0, -1, -1, 33, 7]
    ptr, _, _ = dense_case(X, EUCLIDEAN, capi.DTYPE_BF16, path, 5, sources=sources)
    assert np.diff(ptr).tolist() == [5, 0, 5, 5, 5, 0, 0, 5, 5]
    ptr, _, _ = dense_case(X, EUCLIDEAN, capi.DTYPE_BF16, path, 5, sources=[-1, -1], which=R.HOP1)
    assert ptr.tolist() == [0, 0, 0]


# ---- sparse ---------------------------------------------------------------------------------------------------------------------

def sparse_world(rows=420, dims=300):
    """IDF-style positive rows as tests/sparse_cases.py builds them, and one last row whose only index no other row has"""
    ptr, idx, val = SC.random_csr(np.random.default_rng(21), rows, dims, 1, 12, zipf=True)
    ptr = np.concatenate([ptr, [ptr[-1] + 1]])
    return ptr, np.concatenate([idx, [dims + 5]]).astype(np.uint32), np.concatenate([val, [1.5]]).astype(np.float32)


def sparse_case(n, sources=None, which=R.HOP2, mask=None, positive_only=True, transform=R.RAW, scale=1.0):
    ptr, idx, val = sparse_world()
    index = capi.Sparse(ptr, idx, val)
    try:
        if mask is not None:
            index.set_mask(mask)
        src = list(range(index.N)) if sources is None else list(sources)
        lists = B.sparse_lists(index, ptr, idx, val, src, n)
        return both_routes(lambda h: h.set_table_from_sparse(which, index, n, sources, None, positive_only, transform, scale), lists,
                           src, index.N, n, positive_only, transform, scale, which, ("sparse", n, which))
    finally:
        index.close()


@pytest.mark.parametrize("n", [5, 127, 128, 255, 256])  # n + 1 on both sides of the search's ranking buffers of 128 and 256
def test_sparse_across_k_buckets(n):
    ptr, _, w = sparse_case(n)
    assert ptr[-1] - ptr[-2] == 0 and ptr[-1] > 0 and (w > 0).all()  # the last row shares no index: empty
    assert np.diff(ptr).max() == n if n < 200 else np.diff(ptr).max() > 128


def test_sparse_as_hop1_over_an_unweighted_hop2_and_sources():
    sparse_case(10, which=R.HOP1, transform=R.RECIP)
    ptr, _, _ = sparse_case(10, sources=[400, -1, 3, 3, 420, 17], which=R.HOP1)
    assert np.diff(ptr).tolist()[1] == 0 and np.diff(ptr).tolist()[4] == 0


def test_sparse_mask():
    mask = (np.random.default_rng(22).random(421) < 0.5).astype(np.uint8)
    ptr, ix, _ = sparse_case(20, mask=mask)
    assert mask[ix].all() and ptr[-1] > 0


# ---- errors and lifetime ----------------------------------------------------------------------------------------------------------

def snapshot(h, n_queries):
    return [a.copy() for a in h.get_table(R.HOP2)] + [a.copy() for a in h.recommend(n_queries, 7)]


def test_errors_leave_the_table_in_place():
    X = gauss(30, 60, 8)
    index, big = capi.TopK(X, EUCLIDEAN), capi.TopK(gauss(31, 90, 8), EUCLIDEAN)
    ptr, idx, val = sparse_world()
    sp = capi.Sparse(ptr, idx, val)
    h = capi.NbrRecommender(60)
    h.set_table_from_topk(R.HOP2, index, 5)
    R.Table([[1, 2, 3], [59]]).set_on(h, R.HOP1)
    before = snapshot(h, 2)
    L = capi.lib()
    i64 = lambda a: np.asarray(a, np.int64).ctypes.data_as(C.POINTER(C.c_int64))  # noqa: E731
    INV, RNG, NOMEM = capi.ERR_INVALID, capi.ERR_RANGE, capi.ERR_NOMEM
    nobody = np.full(100_000_000, -1, np.int64)  # 1e8 empty rows of 1023 pairs: 800 GB of staging
    cases = [
        ("NULL index", INV, lambda f, ix: f(h.h, R.HOP2, None, 60, None, 5, 0, R.RAW, 1.0)),
        ("NULL handle", INV, lambda f, ix: f(None, R.HOP2, ix.h, 60, None, 5, 0, R.RAW, 1.0)),
        ("which", INV, lambda f, ix: f(h.h, 2, ix.h, 60, None, 5, 0, R.RAW, 1.0)),
        ("n_rows < 0", INV, lambda f, ix: f(h.h, R.HOP2, ix.h, -1, None, 5, 0, R.RAW, 1.0)),
        ("n = 0", INV, lambda f, ix: f(h.h, R.HOP2, ix.h, 60, None, 0, 0, R.RAW, 1.0)),
        ("n + 1 beyond the search", INV, lambda f, ix: f(h.h, R.HOP2, ix.h, 60, None, 1024, 0, R.RAW, 1.0)),
        ("scale inf", INV, lambda f, ix: f(h.h, R.HOP2, ix.h, 60, None, 5, 0, R.RAW, float("inf"))),
        ("scale nan", INV, lambda f, ix: f(h.h, R.HOP2, ix.h, 60, None, 5, 0, R.RAW, float("nan"))),
        ("transform", INV, lambda f, ix: f(h.h, R.HOP2, ix.h, 60, None, 5, 0, 2, 1.0)),
        ("source beyond the index", RNG, lambda f, ix: f(h.h, R.HOP1, ix.h, 3, i64([0, ix.N, 1]), 5, 0, R.RAW, 1.0)),
        ("NULL sources, more rows than the index", RNG, lambda f, ix: f(h.h, R.HOP1, ix.h, ix.N + 1, None, 5, 0, R.RAW, 1.0)),
        ("staging", NOMEM, lambda f, ix: f(h.h, R.HOP1, ix.h, nobody.size, i64(nobody), 1023, 0, R.RAW, 1.0)),
    ]
    for fn, ix in ((L.gorse_nbr_set_table_from_topk, index), (L.gorse_nbr_set_table_from_sparse, sp)):
        for name, code, call in cases:
            assert call(fn, ix) == code, (fn.__name__, name)
    # hop 2 names items: an index of more rows than the handle has items
    assert L.gorse_nbr_set_table_from_topk(h.h, R.HOP2, big.h, 60, None, 5, 0, R.RAW, 1.0) == RNG
    assert L.gorse_nbr_set_table_from_sparse(h.h, R.HOP2, sp.h, 60, None, 5, 0, R.RAW, 1.0) == RNG
    # a NaN vector: the kept weight of its neighbours' entry for it is not finite
    Xn = X.copy()
    Xn[17] = np.nan
    nan_index = capi.TopK(Xn, EUCLIDEAN)
    lists = B.dense_lists(nan_index, Xn, range(60), 59)
    _, _, w = B.table_from_lists(range(60), lists, 59, False)
    assert not np.isfinite(w).all()
    assert L.gorse_nbr_set_table_from_topk(h.h, R.HOP2, nan_index.h, 60, None, 59, 0, R.RAW, 1.0) == INV
    if capi.device_count() > 1:
        far = capi.TopK(X, EUCLIDEAN, device=1)
        assert L.gorse_nbr_set_table_from_topk(h.h, R.HOP2, far.h, 60, None, 5, 0, R.RAW, 1.0) == INV
        far.close()
    # the read-back's own errors
    with pytest.raises(capi.GorseHipError) as e:
        capi.NbrRecommender(5).get_table(R.HOP1)
    assert e.value.code == INV
    one = np.zeros(8, np.float32)
    assert L.gorse_nbr_get_table(h.h, R.HOP1, None, None, one.ctypes.data_as(C.POINTER(C.c_float))) == INV  # unweighted
    assert L.gorse_nbr_table_info(h.h, 2, None, None, None) == INV
    after = snapshot(h, 2)
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(before, after))
    for x in (index, big, sp, nan_index, h):
        x.close()


def test_lifetime():
    X = gauss(40, 80, 8)
    index = capi.TopK(X, COSINE)
    lists = B.dense_lists(index, X, range(80), 6)
    ptr, ix, w = B.table_from_lists(range(80), lists, 6, False)
    h, ref = capi.NbrRecommender(80), capi.NbrRecommender(80)
    hop1 = R.Table([[3, 4, 79], [], [0, 0, 5]])
    for x in (h, ref):
        hop1.set_on(x, R.HOP1)
    ref.set_table(R.HOP2, ptr, ix, w, R.RECIP, 1.0)
    want = ref.recommend(3, 9)
    h.set_table_from_topk(R.HOP2, index, 6, transform=R.RECIP)
    R.assert_same(h.recommend(3, 9), want, "device-built")
    other = R.Table([[1], [2, 3]] + [[]] * 78, [[0.5], [0.25, 0.125]] + [[]] * 78)
    other.set_on(h, R.HOP2)  # replaced by a host-built table ...
    assert h.table_info(R.HOP2) == (80, 3, True)
    R.assert_same(h.recommend(3, 9), R.recommend(hop1, other, [0, 1, 2], 9), "host-built")
    h.set_table_from_topk(R.HOP2, index, 6, transform=R.RECIP)  # ... and back
    index.close()  # the table owns its memory
    R.assert_same(h.recommend(3, 9), want, "after the index is gone")
    same_tables(h, ref, R.HOP2, "after the index is gone")
    h.close()  # destroy with a device-built table
    ref.close()


# ---- the host twin: HipDatabase::SetNbrTableFromIndex ---------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["embedding", "tags", "auto"])
def test_handle_filled_from_the_resident_index_gives_the_bulk_twins_lists(kind):
    """300 vectors in ascending id order (the row numbering is then the twins' item numbering, ties included): the lists of
    ItemToItemRecommendBulk / UserToUserRecommendBulk, bit for bit, with and without categories"""
    import nbr_host_suite as S
    from gorse_amd import vectors as V
    db = V.Open("hip://")
    coll, ids, positives, excludes, feedback = S.world(db, kind, 23, n=300, n_users=24)

    def lists(h, rows, names, k, seen):
        items, sums, cnt = h.recommend(np.asarray(rows, np.int32), k, *R.seen_csr(seen))
        return [[(names[j], s) for j, s in zip(items[t, :cnt[t]], sums[t, :cnt[t]])] for t in range(len(rows))]

    for n, categories in ((10, None), (3, ["b"])):
        want = V.ItemToItemRecommendBulk(db, coll, kind, positives, excludes, categories, n)
        h = capi.NbrRecommender(300)
        names = V.SetNbrTableFromIndex(db, coll, kind, h, R.HOP2, categories, n)
        assert names == ids and h.table_info(R.HOP2)[0] == 300
        num = {i: r for r, i in enumerate(names)}
        R.Table([[num[p] for p in pos if p in num] for pos in positives]).set_on(h, R.HOP1)
        got = lists(h, range(len(positives)), names, n, [[num[e] for e in exc if e in num] for exc in excludes])
        assert any(len(w) == n for w in want)
        for t in range(len(positives)):
            S.same(want[t], got[t], ("item-to-item", kind, n, t))
        h.close()
    users = ids[:len(excludes)]
    items = sorted({i for row in feedback.values() for i in row})
    inum = {i: j for j, i in enumerate(items)}
    for n in (10, 40):
        want = V.UserToUserRecommendBulk(db, coll, kind, users, excludes, feedback, n)
        h = capi.NbrRecommender(len(items))
        names = V.SetNbrTableFromIndex(db, coll, kind, h, R.HOP1, None, n)
        R.Table([[inum[i] for i in feedback.get(u, [])] for u in names]).set_on(h, R.HOP2)
        num = {i: r for r, i in enumerate(names)}
        got = lists(h, [num[u] for u in users], items, n, [[inum[e] for e in exc if e in inum] for exc in excludes])
        assert any(len(w) == n for w in want)
        for t in range(len(users)):
            S.same(want[t], got[t], ("user-to-user", kind, n, t))
        h.close()
