"""GPU parity of top-k path A (the scan of gorse_amd/csrc/topk.hip) at the row widths of real embeddings.

Every index too deep for the MFMA sweep -- bf16 d > 384, fp32 d > 128, so the reference's shipped embedding_dimensions = 1024 and the
common 1536 and 3072 -- is answered by dist_kernel / norm2_kernel, whose workgroups shrink as the rows grow: scan_groups(d) keeps
(1 + g) rows of d floats inside 144 KB of LDS with g = 16, 8, 4, 2 or 1 sixteen-lane groups, down to a 16-thread workgroup at
d = 16384.  Both sides of every edge of that rule, the 16-chunk + 8-tail + scalar-tail row shapes (d % 16 in 9..15) and the bfloats
summation order (euclid_bf16_lds, which finds its group's first lane inside a partial wave) against the oracle: indices, fp32
distance bits, counts and -1 padding of every call the handle has."""
import functools

import numpy as np
import pytest

import topk_cases as tc
from gorse_amd import capi
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

K = 10
FULL_CHECK_UP_TO, SAMPLE = 4096, 24  # every query's row up to this width, a sample of 24 queries above it


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(autouse=True)
def _reset(oracle):
    oracle.set_isa(orc.ISA_AVX512)
    capi.lib().gorse_hip_test_set_topk_path(0)
    yield


@functools.lru_cache(maxsize=4)
def wide_inputs(d, dtype):
    rng = np.random.default_rng(31000 + 2 * d + dtype)
    N = 300 if d < 1024 else 200  # the oracle scores a pair in d steps: fewer rows where they are long
    Xf = rng.standard_normal((N, d)).astype(np.float32)
    Xf *= rng.uniform(0.5, 2.0, (N, 1)).astype(np.float32)
    X, Xe = tc.as_index(Xf, dtype)
    qs = np.concatenate([rng.integers(0, N, 36), [5, 5, N - 1, 0]]).astype(np.int64)  # unordered, with repeats
    qv, qe = tc.as_index(rng.standard_normal((30, d)).astype(np.float32), dtype)
    mask = (rng.random(N) < 0.6).astype(np.uint8)
    return N, X, Xe, qs, qv, qe, mask


def sample(n, d):
    """positions of a call's n queries that are compared with the oracle"""
    return np.arange(n) if d <= FULL_CHECK_UP_TO or n <= SAMPLE else np.linspace(0, n - 1, SAMPLE).astype(np.int64)


def check_index(oracle, Xe, metric, qs, k, out, at, prune0=False, ids=None):
    idx, dist, cnt = out
    for r in at:
        ei, ed = oracle.search_index(Xe, metric, int(qs[r]), k, prune0)
        n = ei.size
        assert cnt is None or cnt[r] == n, (metric, r)
        assert np.array_equal(idx[r, :n], ei if ids is None else ids[ei]), (metric, r)
        assert np.array_equal(bits(dist[r, :n]), bits(ed)), (metric, r)
        assert (idx[r, n:] == -1).all() and np.isinf(dist[r, n:]).all(), (metric, r)


def check_vector(oracle, Xe, metric, qe, k, out, at, ids=None):
    idx, dist, cnt = out
    for r in at:
        ei, ed = oracle.search_vector(Xe, metric, qe[r], k)
        n = ei.size
        assert cnt[r] == n and np.array_equal(idx[r, :n], ei if ids is None else ids[ei]), (metric, r)
        assert np.array_equal(bits(dist[r, :n]), bits(ed)), (metric, r)
        assert (idx[r, n:] == -1).all(), (metric, r)


def scan_all_calls(oracle, d, dtype, metric):
    N, X, Xe, qs, qv, qe, mask = wide_inputs(d, dtype)
    t = capi.TopK(X, metric, dtype=dtype)
    t.set_profiling(True)
    idx, dist = t.all_pairs(K)
    check_index(oracle, Xe, metric, np.arange(N), K, (idx, dist, None), sample(N, d))
    assert (idx != np.arange(N)[:, None]).all()  # i != q (bruteforce.go:47)
    for prune0 in (False, True):  # prune0: distances <= 0 dropped after the selection
        check_index(oracle, Xe, metric, qs, K, t.search_index(qs, K, prune0), sample(qs.size, d), prune0)
    check_vector(oracle, Xe, metric, qe, K, t.search_vector(qv, K), sample(qv.shape[0], d))  # cosine: the norms of the queries
    few = np.array([0, N - 1, 17], np.int64)  # k > N - 1: every other row, then padding
    out = t.search_index(few, N + 7)
    assert (out[2] == N - 1).all()
    check_index(oracle, Xe, metric, few, N + 7, out, range(3))
    # a mask: ann.Bruteforce over the admissible rows alone, ids unchanged; a query row is one of them
    rows = np.nonzero(mask)[0]
    sub = np.ascontiguousarray(Xe[rows])
    t.set_mask(mask)
    check_vector(oracle, sub, metric, qe, K, t.search_vector(qv[:12], K), range(12), ids=rows)
    mq = rows[::max(1, rows.size // 12)]
    check_index(oracle, sub, metric, np.searchsorted(rows, mq), K, t.search_index(mq, K), range(mq.size), ids=rows)
    t.set_mask(None)
    again = t.all_pairs(K)
    assert np.array_equal(again[0], idx) and np.array_equal(bits(again[1]), bits(dist))
    assert t.get_profile(capi.PROF_TOPK_SCORE)[0] > 0 and t.get_profile(capi.PROF_TOPK_SWEEP)[0] == 0  # the scan answered


@pytest.mark.parametrize("metric", tc.METRICS)
@pytest.mark.parametrize("dtype", [tc.F32, tc.BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("d", tc.WIDE_WIDTHS)
def test_scan_at_every_group_count_and_tail(oracle, d, dtype, metric):
    scan_all_calls(oracle, d, dtype, metric)


@pytest.mark.parametrize("d", tc.WIDE_BF16_ORDER_WIDTHS)
def test_bfloats_order_in_whole_and_partial_waves(oracle, d):
    """bfloats.Euclidean's summation order with 16, 2 and 1 sixteen-lane groups in a workgroup"""
    assert [tc.scan_groups(w) for w in tc.WIDE_BF16_ORDER_WIDTHS] == [16, 2, 1]
    scan_all_calls(oracle, d, tc.BF16, capi.METRIC_EUCLIDEAN_BF16)


@pytest.mark.parametrize("metric", tc.METRICS)
@pytest.mark.parametrize("dtype", [tc.F32, tc.BF16], ids=["f32", "bf16"])
def test_ties_at_1024_take_the_literal_heaps(oracle, dtype, metric):
    """Two copies of one row: its query and the copies' queries have equal distances inside the k + 1 best, select_fast_kernel
    flags them, and no MFMA path exists at this width to take them -- the literal container/heap kernel decides them"""
    d = 1024
    rng = np.random.default_rng(1024 + 10 * metric + dtype)
    N = 300
    Xf = rng.standard_normal((N, d)).astype(np.float32) * rng.uniform(0.5, 2.0, (N, 1)).astype(np.float32)
    Xf[150] = Xf[7]
    Xf[280] = Xf[7]
    X, Xe = tc.as_index(Xf, dtype)
    t = capi.TopK(X, metric, dtype=dtype)
    idx, dist = t.all_pairs(K)
    check_index(oracle, Xe, metric, np.arange(N), K, (idx, dist, None), range(N))
    for q in (7, 150, 280):
        _, ed = oracle.search_index(Xe, metric, q, K + 1)
        assert ed[0] == ed[1]  # the two other copies, at one distance
    qv, qe = X[[7, 150, 3]], Xe[[7, 150, 3]]
    check_vector(oracle, Xe, metric, qe, K, t.search_vector(qv, K), range(3))  # by vector: three equal rows, none excluded
    for prune0 in (False, True):
        qs = np.array([280, 7, 7, 150, 0], np.int64)
        check_index(oracle, Xe, metric, qs, K, t.search_index(qs, K, prune0), range(qs.size), prune0)


def test_rows_wider_than_the_scan_stages_are_rejected(oracle):
    d = tc.TOPK_MAX_DIM + 1
    for dtype in (tc.F32, tc.BF16):
        with pytest.raises(capi.GorseHipError) as e:
            capi.TopK(np.zeros((4, d), np.uint16 if dtype == tc.BF16 else np.float32), capi.METRIC_NEG_DOT, dtype=dtype)
        assert e.value.code == capi.ERR_INVALID
    rng = np.random.default_rng(3)
    X = rng.standard_normal((50, 16)).astype(np.float32)  # the process still answers
    qs = np.arange(50, dtype=np.int64)
    check_index(oracle, X, capi.METRIC_NEG_DOT, qs, 5, capi.TopK(X, capi.METRIC_NEG_DOT).search_index(qs, 5), range(50))
