"""The inputs of tests/test_gpu_topk_scan_select.py can fail a wrong selection kernel (no GPU): with the oracle alone, every builder
of tests/topk_cases.py gives the property its GPU test relies on -- one -0.0 in the signed-zero lists, the k + 1 best rows of the
concentrated cases in one thread's stride, k + 2 rows strictly better than the plateau, no equal pair among the k + 1 best wherever
the fast kernel is expected to answer, a NaN distance exactly where a query is expected to be flagged."""
import numpy as np
import pytest

import topk_cases as tc

NEG_ZERO = 0x80000000


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def all_distances(oracle, X, metric, q):
    """the oracle's list of ALL distances of a query (a stored row's id, itself left out, or a vector), ascending"""
    if np.ndim(q) == 0:
        return oracle.search_index(X, metric, int(q), X.shape[0])[1]
    return oracle.search_vector(X, metric, q, X.shape[0])[1]


@pytest.mark.parametrize("dtype", [tc.F32, tc.BF16], ids=["f32", "bf16"])
def test_signed_zero_lists_hold_one_negative_zero(oracle, dtype):
    (X6, qv, k6), (X40, qi, k40) = tc.signed_zero_cases()
    for X in (X6, X40):
        assert np.array_equal(tc.as_index(X, dtype)[1], X)  # every value is a bf16 value: one expectation for both dtypes
    ei, ed = oracle.search_vector(X6, tc.NEG_DOT, qv, k6)
    assert ei.tolist() == [4, 2, 1, 0, 3]
    assert ["%08x" % b for b in bits(ed)] == ["c0400000", "c0000000", "bf800000", "80000000", "3f800000"]
    assert tc.distinct_best(all_distances(oracle, X6, tc.NEG_DOT, qv), k6)
    assert np.array_equal(X40[qi], qv)
    ei, ed = oracle.search_index(X40, tc.NEG_DOT, qi, k40)
    assert ei.size == k40 and int((bits(ed) == NEG_ZERO).sum()) == 1 and not (bits(ed) == 0).any()
    assert tc.distinct_best(all_distances(oracle, X40, tc.NEG_DOT, qi), k40)
    assert oracle.search_index(X40, tc.NEG_DOT, qi, k40, True)[0].size == 2  # prune0 drops both zeros and what is below


@pytest.mark.parametrize("metric", tc.METRICS)
@pytest.mark.parametrize("k", tc.SEL_KS)
def test_concentrated_best_rows_share_one_stride(oracle, k, metric):
    X, planted = tc.concentrated_case(metric, k)
    assert X.shape == ((k + 8) * 1024 + 6, tc.SEL_D) and planted.size == k + 6
    assert (planted % tc.SEL_THREADS == tc.SEL_STRIDE_AT).all()
    assert k + 1 > tc.SEL_KEEP  # one thread cannot keep them
    for q in tc.sel_queries():
        ei, ed = oracle.search_vector(X, metric, q, k + 6)
        assert set(ei.tolist()) == set(planted.tolist())  # every planted row beats every background row
        assert (ei[:k + 1] % tc.SEL_THREADS == tc.SEL_STRIDE_AT).all() and np.unique(ed[:k + 1]).size == k + 1
        assert not np.array_equal(ei, np.sort(ei)) and not np.array_equal(ei, np.sort(ei)[::-1])  # ranks in no index order
        d = all_distances(oracle, X, metric, q)
        assert not np.isnan(d).any() and d[k + 6] > d[k + 5]  # the background starts strictly behind the planted rows


@pytest.mark.parametrize("metric", tc.METRICS)
@pytest.mark.parametrize("k", tc.SEL_KS)
@pytest.mark.parametrize("variant", ["A", "B"])
def test_plateau_lies_behind_k_plus_2_better_rows(oracle, variant, k, metric):
    X, planted = tc.plateau_case(metric, k, variant)
    others = np.delete(np.arange(X.shape[0]), planted)
    assert others.size > tc.SEL_CAP and (X[others] == tc.plateau_row(metric)).all()
    if variant == "A":
        assert (planted % tc.SEL_THREADS == tc.SEL_STRIDE_AT).all()
    else:
        assert planted.tolist() == list(range(k + 6))  # one per stride
    for q in tc.sel_queries():
        level = np.float32(oracle.distance(metric, q, tc.plateau_row(metric)))
        ei, ed = oracle.search_vector(X, metric, q, k + 2)
        assert np.isin(ei, planted).all() and (ed < level).all() and np.unique(ed).size == k + 2
        d = all_distances(oracle, X, metric, q)
        assert not np.isnan(d).any() and (d[k + 6:] == level).all()


@pytest.mark.parametrize("metric", tc.METRICS)
def test_stride_cases_have_the_stated_queries(oracle, metric):
    assert set(tc.STRIDE_NS) >= {1, 2, 1023, 1024, 1025, 2047, 2048, 2049, 4096, 4097}
    for N in tc.STRIDE_NS:
        X, qs, qv = tc.stride_case(N, metric)
        assert X.shape[0] == N and 0 in qs and N - 1 in qs and qs.size <= 12 and qv.shape[0] == 4
    assert tc.stride_case(4097, metric)[1].size >= 11


def kcap_seed_ok(oracle, metric, k, seed_try):
    X, qs, qv = tc.kcap_case(metric, k, seed_try)
    return all(tc.distinct_best(all_distances(oracle, X, metric, q), k) for q in list(qs) + list(qv))


@pytest.mark.parametrize("metric", tc.METRICS)
@pytest.mark.parametrize("k", tc.KCAP_KS)
def test_kcap_seed_table_is_the_first_tie_free_seed(oracle, k, metric):
    assert tc.KCAP_KS == (tc.SEL_CAP // 2 - 1, tc.SEL_CAP // 2, tc.KCAP_N + 3)
    used = tc.KCAP_SEED_TRY.get((metric, k), 0)
    assert kcap_seed_ok(oracle, metric, k, used)
    assert not any(kcap_seed_ok(oracle, metric, k, s) for s in range(used))


def test_masks_admit_the_stated_rows(oracle):
    X, qv, masks, hidden = tc.mask_case()
    k = tc.MASK_K
    assert set(masks) == set(tc.MASK_NAMES)
    count = {n: int(m.sum()) for n, m in masks.items()}
    assert count["one_stride"] == 8 < k and count["two_strides"] == 16 >= k + 1
    assert 2 * tc.SEL_KEEP < k + 1  # the two threads' kept keys never reach k + 1: the bound saturates
    for name in ("one_stride", "two_strides"):
        assert set(np.nonzero(masks[name])[0] % tc.SEL_THREADS) == ({3} if name == "one_stride" else {3, 4})
    assert [count[n] for n in ("k_minus_1", "k", "k_plus_1", "none")] == [k - 1, k, k + 1, 0]
    assert not any(m[hidden] for m in masks.values()) and count["random"] > tc.SEL_CAP
    for metric in tc.METRICS:  # the fast kernel is expected to answer every one of these queries
        for name, m in masks.items():
            rows = np.nonzero(m)[0]
            if rows.size == 0:
                continue
            sub = np.ascontiguousarray(X[rows])
            for q in list(qv) + [X[hidden]]:
                assert tc.distinct_best(all_distances(oracle, sub, metric, q), k), (metric, name)
            for pos in range(0, rows.size, max(1, rows.size // 5))[:5]:
                assert tc.distinct_best(all_distances(oracle, sub, metric, pos), k), (metric, name)


def test_nonfinite_queries_meet_a_nan_exactly_where_stated(oracle):
    X, qs, qv, masks = tc.nonfinite_case()
    k = tc.NONFINITE_K
    assert np.isnan(X[5, 3]) and X[77, 0] == np.inf and X[300, 1] == -np.inf and np.isfinite(np.delete(X, tc.NONFINITE_ROWS, 0)).all()
    assert not np.isin(qs, tc.NONFINITE_ROWS).any() and qs.size > np.unique(qs).size
    for metric in tc.METRICS:
        for q in list(qs) + list(qv):
            assert np.isnan(all_distances(oracle, X, metric, q)).any()  # every query meets the NaN row
        for name, m in masks.items():
            rows = np.nonzero(m)[0]
            sub = np.ascontiguousarray(X[rows])
            for q in [int(np.searchsorted(rows, t)) for t in qs] + list(qv):
                d = all_distances(oracle, sub, metric, q)
                if name == "nan_hidden" and metric == tc.COSINE:
                    assert np.isnan(d).any()  # inf / inf: the infinite rows give a NaN of their own
                else:
                    assert tc.distinct_best(d, k), (metric, name)
                    if name == "nan_hidden":  # overflowed distances are ordinary keys
                        assert np.isinf(d).sum() == 2
                        assert metric != tc.NEG_DOT or (d[0] == -np.inf and d[-1] == np.inf)


def test_reroute_and_block_cases(oracle):
    X, qs, mask = tc.reroute_case()
    assert X.shape == (300, 8) and qs.size < 768 and tc.REROUTE_K == 15
    for metric in (tc.NEG_DOT, tc.EUCLIDEAN):
        tied = [not tc.distinct_best(all_distances(oracle, X, metric, int(q)), tc.REROUTE_K) for q in qs]
        assert sum(tied) > qs.size // 2
        rows = np.nonzero(mask)[0]
        sub = np.ascontiguousarray(X[rows])
        assert sum(not tc.distinct_best(all_distances(oracle, sub, metric, p), tc.REROUTE_K) for p in range(40)) > 20
    n_blocks = -(-tc.BLOCK_N // tc.BLOCK_QUERIES)
    assert n_blocks == 43 and tc.BLOCK_N % tc.BLOCK_QUERIES == 6  # the last block is partial
    for dtype in (tc.F32, tc.BF16):
        X, Xe, qs, qv, qe = tc.block_case(dtype)
        assert qs.size == 100 and np.unique(qs).size < 100 and (np.diff(qs) < 0).any() and qv.shape[0] == 50
        assert qs.size % tc.BLOCK_QUERIES and qv.shape[0] % tc.BLOCK_QUERIES
