"""GPU parity of top-k path B (gorse_amd/csrc/topk_mfma.hip; its sweep: topk_sweep.hip) at every operand depth its sweep is instantiated for.

The sweep is a template over KP, the operand depth in k-steps of 16: kSupportedKP = {1, 2, 3, 4, 6, 8, 12, 16, 24}, with another tile
form, workgroup shape and column-block count per depth (launch_sweep; sweep_waves and sweep_dma of topk_plan.hpp).  tests/test_gpu_topk_mfma.py reaches
the depths its row widths happen to give; here every depth is reached in both dtypes, with an operand matrix that is the bf16 index
itself (d == 16 KP), that is full (fp32, 3 d == 16 KP) and that ends in whole k-steps of zeros (pad_bf16_kernel / split_f32_kernel),
through the main sweep and through the tie path's history sweep.  The bar is path A's: the indices and the fp32 distance bits of
ann.Bruteforce (common/ann/bruteforce.go:39-83), ties included; the oracle is the checker.

The inputs of test_every_depth_matches_oracle are tie free at every sampled query (no two equal distances among the k + 1 best;
checked with the oracle alone, for the seeds of topk_cases.depth_inputs, k = 25 and k = 100), so that the reference itself never
sends one of them to the scan."""
import numpy as np
import pytest

import topk_cases as tc
from gorse_amd import capi
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

V_TILE64, V_SLICES8 = capi.TOPK_TILE64, capi.TOPK_SLICES8


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def case_id(c):
    return "%s-d%d-kp%d" % ("bf16" if c[0] == tc.BF16 else "f32", c[1], tc.expected_kp(*c) or 0)


@pytest.fixture(autouse=True)
def _paths(oracle):
    oracle.set_isa(orc.ISA_AVX512)
    capi.lib().gorse_hip_test_set_topk_path(2)
    yield
    capi.lib().gorse_hip_test_set_topk_path(0)
    capi.lib().gorse_hip_test_set_topk_variant(0)


def test_the_table_names_every_depth_in_both_dtypes():
    """(tests/test_topk_depth_table_cpu.py holds SUPPORTED_KP against the kernels' source)"""
    for dtype in (tc.F32, tc.BF16):
        assert {tc.expected_kp(t, d) for t, d in tc.DEPTH_CASES if t == dtype} == set(tc.SUPPORTED_KP)
    assert {tc.expected_kp(*c) for c in tc.DEPTH_K100} == {12, 16, 24}
    assert {tc.expected_kp(*c) for c in tc.TIE_CASES} == {3, 6, 12, 16, 24} and {t for t, _ in tc.TIE_CASES} == {tc.F32, tc.BF16}


def check_index_rows(oracle, Xe, metric, qs, k, idx, dist, cnt=None, prune0=False):
    """rows of a search by stored id against the oracle: indices, distance bits, counts, -1 padding"""
    for r, q in enumerate(qs):
        ei, ed = oracle.search_index(Xe, metric, int(q), k, prune0)
        n = ei.size
        assert cnt is None or cnt[r] == n, (metric, q)
        assert np.array_equal(idx[r, :n], ei), (metric, q)
        assert np.array_equal(bits(dist[r, :n]), bits(ed)), (metric, q)
        assert (idx[r, n:] == -1).all(), (metric, q)


def check_vector_rows(oracle, Xe, metric, qe, rows, k, idx, dist, cnt):
    for r in rows:
        ei, ed = oracle.search_vector(Xe, metric, qe[r], k)
        n = ei.size
        assert cnt[r] == n and np.array_equal(idx[r, :n], ei) and np.array_equal(bits(dist[r, :n]), bits(ed)), (metric, r)
        assert (idx[r, n:] == -1).all(), (metric, r)


def sweep_all_calls(oracle, dtype, d, metric, k):
    """all_pairs, search_index over an unordered list with repeats and search_vector through path B, a sample of each against the
    oracle; the scan's rows for the first 600 queries; returns the fallback count of the all-pairs call"""
    N, step = tc.DEPTH_N, tc.DEPTH_SAMPLE
    X, Xe, qs, qv, qe = tc.depth_inputs(dtype, d, metric, k)
    t = capi.TopK(X, metric, dtype=dtype)
    assert tc.expected_kp(dtype, d) in tc.SUPPORTED_KP
    idx, dist = t.all_pairs(k)
    n_fb, n_tie = t.last_stats()
    print("KP %d %s d %d metric %d k %d: %d of %d queries to the scan (cap %d), %d to the replay"
          % (tc.expected_kp(dtype, d), "bf16" if dtype == tc.BF16 else "f32", d, metric, k, n_fb, N, N // 50, n_tie))
    assert n_fb <= N // 50, "path B handed %d of %d queries to the scan" % (n_fb, N)
    rows = np.arange(0, N, step)
    check_index_rows(oracle, Xe, metric, rows, k, idx[rows], dist[rows])
    assert (idx != np.arange(N)[:, None]).all()  # i != q (bruteforce.go:47)
    i2, d2, c2 = t.search_index(qs, k)
    assert (c2 == k).all() and (i2 != qs[:, None]).all()
    check_index_rows(oracle, Xe, metric, qs[::step], k, i2[::step], d2[::step], c2[::step])
    i3, d3, c3 = t.search_vector(qv, k)
    check_vector_rows(oracle, Xe, metric, qe, range(0, qv.shape[0], step), k, i3, d3, c3)
    capi.lib().gorse_hip_test_set_topk_path(1)  # the two paths agree on every row
    try:
        ia, da = t.all_pairs(k, 0, 600)
    finally:
        capi.lib().gorse_hip_test_set_topk_path(2)
    assert np.array_equal(ia, idx[:600]) and np.array_equal(bits(da), bits(dist[:600]))
    return n_fb


@pytest.mark.parametrize("metric", tc.METRICS)
@pytest.mark.parametrize("case", tc.DEPTH_CASES, ids=case_id)
def test_every_depth_matches_oracle(oracle, case, metric):
    sweep_all_calls(oracle, case[0], case[1], metric, tc.DEPTH_K)


@pytest.mark.parametrize("metric", tc.METRICS)
@pytest.mark.parametrize("case", tc.DEPTH_K100, ids=case_id)
def test_deep_operands_with_k_100(oracle, case, metric):
    sweep_all_calls(oracle, case[0], case[1], metric, 100)


@pytest.mark.parametrize("metric", tc.METRICS)
@pytest.mark.parametrize("case", tc.TILE64_CASES, ids=case_id)
def test_64_row_tiles_of_the_register_staged_sweep(oracle, case, metric):
    """TOPK_TILE64: KP 3 and KP 6 stage their tiles through registers; with 64-row tiles (RB = 2) the same rows"""
    capi.lib().gorse_hip_test_set_topk_variant(V_TILE64)
    sweep_all_calls(oracle, case[0], case[1], metric, tc.DEPTH_K)


TIE_PAIRS = ((3, 9000), (3, 23990), (40, 12000), (40, 12001), (700, 23000), (900, 100), (1023, 15000), (5, 6), (511, 23999))
TIE_RUN = (1000, 1016)


@pytest.mark.parametrize("metric", tc.METRICS)
@pytest.mark.parametrize("case", tc.TIE_CASES, ids=case_id)
def test_tie_path_at_every_history_sweep_shape(oracle, case, metric):
    """The history sweep of the tie path is another kernel shape per depth (sweep_waves): two-wave workgroups at KP 3 and 6, four
    waves at KP 12, eight register-staged waves at KP 16 and 24.  Pairs of equal rows early and late in the index and a run of sixteen
    equal rows: their queries have equal distances inside the k + 1 best, the replay (not the scan) answers them, in one row slice
    and in eight."""
    dtype, d = case
    rng = np.random.default_rng(5200 + 10 * d + metric)
    N, k, nq = 24000, 30, 1024
    Xf = rng.standard_normal((N, d)).astype(np.float32)
    if metric == capi.METRIC_COSINE:
        Xf /= np.sqrt((Xf * Xf).sum(1))[:, None]
    for src, dst in TIE_PAIRS:
        Xf[dst] = Xf[src]
    Xf[TIE_RUN[0]:TIE_RUN[1]] = Xf[TIE_RUN[0]]
    X, Xe = tc.as_index(Xf, dtype)
    planted = sorted({q for p in TIE_PAIRS for q in p if q < nq} | set(range(*TIE_RUN)))
    plain = [0, 1, 77, 123, 256, 300, 512, 640, 801, 950, 999, 1016]
    assert not set(plain) & set(planted) and len(plain) == 12
    expect = {q: oracle.search_index(Xe, metric, q, k) for q in planted + plain}
    for variant in (0, V_SLICES8):
        capi.lib().gorse_hip_test_set_topk_variant(variant)
        t = capi.TopK(X, metric, dtype=dtype)
        idx, dist, cnt = t.search_index(np.arange(nq), k)
        n_scan, n_replay = t.last_stats()
        print("KP %d metric %d variant %d: %d tie replays, %d to the scan" % (tc.expected_kp(dtype, d), metric, variant, n_replay, n_scan))
        assert n_replay > 0, (variant, n_scan, n_replay)
        for q, (ei, ed) in expect.items():
            assert cnt[q] == ei.size and np.array_equal(idx[q, :cnt[q]], ei), (variant, q)
            assert np.array_equal(bits(dist[q, :cnt[q]]), bits(ed)), (variant, q)
        del t


@pytest.mark.parametrize("metric", tc.METRICS)
@pytest.mark.parametrize("case", tc.TOO_DEEP_CASES, ids=case_id)
def test_one_column_past_the_deepest_operand_takes_the_scan(oracle, case, metric):
    """bf16 d = 385 and fp32 d = 129 need a 25th k-step: no path B operands are built, and with path B forced the scan answers --
    its score kernel launches, no sweep does -- with the oracle's rows"""
    dtype, d = case
    rng = np.random.default_rng(8800 + d + metric)
    N, k = 1200, 25
    Xf = rng.standard_normal((N, d)).astype(np.float32)
    Xf *= rng.uniform(0.2, 3.0, (N, 1)).astype(np.float32)
    X, Xe = tc.as_index(Xf, dtype)
    qv, qe = tc.as_index(rng.standard_normal((20, d)).astype(np.float32), dtype)
    t = capi.TopK(X, metric, dtype=dtype)
    t.set_profiling(True)
    idx, dist = t.all_pairs(k)
    qs = np.concatenate([rng.integers(0, N, 40), [5, 5, N - 1, 0]]).astype(np.int64)
    i2, d2, c2 = t.search_index(qs, k)
    i3, d3, c3 = t.search_vector(qv, k)
    assert t.get_profile(capi.PROF_TOPK_SCORE)[0] >= 3
    for cls in (capi.PROF_TOPK_SWEEP, capi.PROF_TOPK_SELECT, capi.PROF_TOPK_HIST, capi.PROF_TOPK_REPLAY):
        assert t.get_profile(cls)[0] == 0, cls
    rows = np.arange(0, N, tc.DEPTH_SAMPLE)
    check_index_rows(oracle, Xe, metric, rows, k, idx[rows], dist[rows])
    assert (idx != np.arange(N)[:, None]).all()
    check_index_rows(oracle, Xe, metric, qs, k, i2, d2, c2)
    check_vector_rows(oracle, Xe, metric, qe, range(qv.shape[0]), k, i3, d3, c3)
