"""GPU parity of the deep sweep form of top-k path B (gorse_topk_set_deep_sweep; gorse_amd/csrc/topk_deep.hip, rules in
topk_deep_plan.hpp): bf16 rows of 384 < d <= 4096 and fp32 rows of 128 < d <= 1536 on the matrix cores.  Path B is forced through the
test hook; every result is held to the oracle's search_index / search_vector in indices, distance bits, counts and -1 padding, and to
the same handle in mode 0 (the scan).

The cap of N // 50 queries handed to the scan is a condition on the inputs: the only queries a deep handle hands over are those
with equal distances among their k + 1 best (or a list that overflowed).  The inputs follow tc.depth_inputs' seed recipe (seed try 0
at every case).  They were NOT examined exhaustively with the oracle alone for k = 25 (a d = 4096 case costs it minutes); what is
known is the device's own count on an MI355X (last_stats): between 0 and 17 of 2500 queries per case and metric (cosine the most), against
the cap of 50.  A case whose inputs turn out to hold more ties than the cap needs another seed try, not a wider cap."""
import numpy as np
import pytest

import topk_cases as tc
from gorse_amd import capi
from gorse_amd import vectors as V
from oracle import oracle as orc
from test_gpu_topk_depths import TIE_PAIRS, TIE_RUN, bits, check_index_rows, check_vector_rows

pytestmark = pytest.mark.gpu

BF16, F32 = tc.BF16, tc.F32
# the first too-deep width, a ragged last K-slice (400 = 6 x 64 + 16), 768, 1536, the widest; fp32: first too-deep, 3 d = 1020 not a
# whole slice, the widest (operand 4608)
DEPTH_CASES = ((BF16, 385), (BF16, 400), (BF16, 768), (BF16, 1536), (BF16, 4096), (F32, 129), (F32, 340), (F32, 1536))
N, K, STEP = tc.DEPTH_N, tc.DEPTH_K, tc.DEPTH_SAMPLE


def case_id(c):
    return "%s-d%d" % ("bf16" if c[0] == BF16 else "f32", c[1])


@pytest.fixture(autouse=True)
def _paths(oracle):
    oracle.set_isa(orc.ISA_AVX512)
    capi.lib().gorse_hip_test_set_topk_path(2)
    yield
    capi.lib().gorse_hip_test_set_topk_path(0)
    capi.lib().gorse_hip_test_set_topk_variant(0)


def deep_index(X, metric, dtype):
    t = capi.TopK(X, metric, dtype=dtype)
    t.set_profiling(True)
    t.set_deep_sweep(1)
    return t


def assert_deep_ran(t):
    assert t.get_profile(capi.PROF_TOPK_DEEP)[0] > 0 and t.get_profile(capi.PROF_TOPK_SWEEP)[0] == 0
    assert t.get_deep_sweep() == (1, 1, 1)


@pytest.mark.parametrize("metric", tc.METRICS)
@pytest.mark.parametrize("case", DEPTH_CASES, ids=case_id)
def test_depth_edges_match_oracle(oracle, case, metric):
    """N = 2500: the last row tile mostly past N, a ragged last query block; an unordered id list with repeats; 300 query vectors"""
    dtype, d = case
    step = STEP if d < 1536 else 4 * STEP  # the oracle costs a wide row more: every 36th row there
    X, Xe, qs, _, _ = tc.depth_inputs(dtype, d, metric, K)
    qv, qe = tc.as_index(np.random.default_rng(31 * d + metric).standard_normal((300, d)).astype(np.float32), dtype)
    t = deep_index(X, metric, dtype)
    idx, dist = t.all_pairs(K)
    assert_deep_ran(t)
    assert t.last_stats()[0] <= N // 50
    rows = np.arange(0, N, step)
    check_index_rows(oracle, Xe, metric, rows, K, idx[rows], dist[rows])
    assert (idx != np.arange(N)[:, None]).all()
    i2, d2, c2 = t.search_index(qs, K)
    assert_deep_ran(t)
    check_index_rows(oracle, Xe, metric, qs[::step], K, i2[::step], d2[::step], c2[::step])
    i3, d3, c3 = t.search_vector(qv, K)
    assert_deep_ran(t)
    check_vector_rows(oracle, Xe, metric, qe, range(0, 300, step), K, i3, d3, c3)
    t.set_deep_sweep(0)  # the same handle in mode 0: the scan
    ia, da = t.all_pairs(K, 0, 600)
    assert t.get_deep_sweep() == (0, 0, 0)
    assert np.array_equal(ia, idx[:600]) and np.array_equal(bits(da), bits(dist[:600]))


@pytest.mark.parametrize("k", (100, 255, 256))
def test_k_edges(oracle, k):
    """kth = k + 1 = 256 is the path's limit; k = 256 takes the scan"""
    X, Xe, qs, _, _ = tc.depth_inputs(BF16, 768, capi.METRIC_COSINE, K)
    t = deep_index(X, capi.METRIC_COSINE, BF16)
    idx, dist, cnt = t.search_index(qs, k)
    if k == 256:
        assert t.get_profile(capi.PROF_TOPK_DEEP)[0] == 0 and t.get_deep_sweep() == (1, 1, 0)
    else:
        assert_deep_ran(t)
    check_index_rows(oracle, Xe, capi.METRIC_COSINE, qs[::STEP], k, idx[::STEP], dist[::STEP], cnt[::STEP])


@pytest.mark.parametrize("variant", (capi.TOPK_WARM_ALWAYS, capi.TOPK_WARM_ALWAYS | capi.TOPK_PILOT_KTH2), ids=("warm", "pilot_kth2"))
@pytest.mark.parametrize("case", ((BF16, 768), (F32, 340)), ids=case_id)
def test_warm_start_through_the_deep_kernel(oracle, case, variant):
    """WARM_ALWAYS: both pilots (strides 256 and 16) are the deep kernel; PILOT_KTH2: thresholds far too high, the verification fails
    and the scan answers with the oracle's rows"""
    dtype, d = case
    metric = capi.METRIC_EUCLIDEAN
    X, Xe, _, _, _ = tc.depth_inputs(dtype, d, metric, K)
    capi.lib().gorse_hip_test_set_topk_variant(variant)
    t = deep_index(X, metric, dtype)
    idx, dist = t.all_pairs(K)
    assert_deep_ran(t)
    assert t.get_profile(capi.PROF_TOPK_DEEP)[0] == 1  # one bracket around the pilots and the main sweep
    n_fb, _ = t.last_stats()
    assert (n_fb > 0) if variant & capi.TOPK_PILOT_KTH2 else (n_fb <= N // 50), n_fb
    rows = np.arange(0, N, STEP)
    check_index_rows(oracle, Xe, metric, rows, K, idx[rows], dist[rows])


@pytest.mark.parametrize("metric", tc.METRICS)
def test_ties_go_to_the_scan(oracle, metric):
    """pairs of equal rows early and late in the index and a run of sixteen: no tie path on a deep handle, the scan answers them"""
    dtype, d, n, k, nq = BF16, 400, 24000, 30, 1024
    rng = np.random.default_rng(5300 + metric)
    Xf = rng.standard_normal((n, d)).astype(np.float32)
    for src, dst in TIE_PAIRS:
        Xf[dst] = Xf[src]
    Xf[TIE_RUN[0]:TIE_RUN[1]] = Xf[TIE_RUN[0]]
    X, Xe = tc.as_index(Xf, dtype)
    planted = sorted({q for p in TIE_PAIRS for q in p if q < nq} | set(range(*TIE_RUN)))
    t = deep_index(X, metric, dtype)
    idx, dist, cnt = t.search_index(np.arange(nq), k)
    assert_deep_ran(t)
    n_fb, n_tie = t.last_stats()
    assert n_fb >= TIE_RUN[1] - TIE_RUN[0] and n_tie == 0  # a query of the run has fifteen equal distances among its k + 1 best
    check_index_rows(oracle, Xe, metric, planted + [0, 77, 512, 1016], k, idx[planted + [0, 77, 512, 1016]], dist[planted + [0, 77, 512, 1016]])


@pytest.mark.parametrize("mask_kind", ("scattered", "tile", "few"))
def test_masked_rows(oracle, mask_kind):
    """inadmissible rows scattered, a whole row tile (rows 128 .. 255) masked, fewer than k admissible rows"""
    metric, dtype, d = capi.METRIC_NEG_DOT, F32, 129
    X, Xe, _, _, _ = tc.depth_inputs(dtype, d, metric, K)
    rng = np.random.default_rng(17)
    ok = {"scattered": rng.random(N) < 0.6, "tile": ~((np.arange(N) >= 128) & (np.arange(N) < 256)), "few": np.arange(N) % 131 == 7}[mask_kind]
    qv, qe = tc.as_index(rng.standard_normal((40, d)).astype(np.float32), dtype)
    t = deep_index(X, metric, dtype)
    t.set_mask(ok.astype(np.uint8))
    idx, dist, cnt = t.search_vector(qv, K)
    assert_deep_ran(t)
    keep = np.nonzero(ok)[0]
    for r in range(40):
        ei, ed = oracle.search_vector(Xe[keep], metric, qe[r], K)
        assert cnt[r] == ei.size == min(K, keep.size) and np.array_equal(idx[r, :cnt[r]], keep[ei]), (mask_kind, r)
        assert np.array_equal(bits(dist[r, :cnt[r]]), bits(ed)) and (idx[r, cnt[r]:] == -1).all(), (mask_kind, r)


def test_sizes_below_one_tile(oracle):
    """N = 100 rows and one query, the path forced"""
    metric = capi.METRIC_EUCLIDEAN
    X, Xe, _, qv, qe = tc.depth_inputs(BF16, 385, metric, K, N=100)
    t = deep_index(X, metric, BF16)
    idx, dist, cnt = t.search_vector(qv[:1], K)
    assert_deep_ran(t)
    check_vector_rows(oracle, Xe, metric, qe, [0], K, idx, dist, cnt)
    i2, d2, c2 = t.search_index(np.array([99], np.int64), K)
    check_index_rows(oracle, Xe, metric, [99], K, i2, d2, c2)


def test_what_mode_1_does_not_touch(oracle):
    rng = np.random.default_rng(3)
    metric = capi.METRIC_COSINE

    def index(d, dtype, spoil=None):
        Xf = rng.standard_normal((300, d)).astype(np.float32)
        if spoil is not None:
            Xf[7] = spoil
        t = deep_index(tc.as_index(Xf, dtype)[0], metric, dtype)
        t.all_pairs(5)
        return t

    t = index(128, BF16)  # path B serves it already: the register-resident sweep
    assert t.get_deep_sweep() == (1, 0, 0) and t.get_profile(capi.PROF_TOPK_SWEEP)[0] > 0 and t.get_profile(capi.PROF_TOPK_DEEP)[0] == 0
    for d, dtype, spoil in ((4097, BF16, None), (1537, F32, None), (385, BF16, np.nan), (385, BF16, 0.0)):
        t = index(d, dtype, spoil)  # outside the ranges, a NaN row, a zero row under cosine: the scan
        assert t.get_deep_sweep() == (1, 0, 0), (d, dtype, spoil)
        assert t.get_profile(capi.PROF_TOPK_SCORE)[0] > 0 and t.get_profile(capi.PROF_TOPK_DEEP)[0] == 0
    t = index(385, BF16)
    assert_deep_ran(t)
    with pytest.raises(capi.GorseHipError) as e:
        t.set_deep_sweep(2)
    assert e.value.code == capi.ERR_INVALID and t.get_deep_sweep() == (1, 1, 1)
    t.set_deep_sweep(0)
    before = t.get_profile(capi.PROF_TOPK_DEEP)[0]
    t.all_pairs(5)
    assert t.get_profile(capi.PROF_TOPK_DEEP)[0] == before and t.get_deep_sweep() == (0, 0, 0)


def test_neighbour_table_from_a_deep_index():
    X, _, _, _, _ = tc.depth_inputs(BF16, 768, capi.METRIC_EUCLIDEAN, K)
    tables = []
    for mode in (1, 0):
        t = deep_index(X, capi.METRIC_EUCLIDEAN, BF16)
        t.set_deep_sweep(mode)
        h = capi.NbrRecommender(N)
        h.set_table_from_topk(capi.NBR_HOP2, t, 20, transform=capi.NBR_RECIP)
        assert (t.get_profile(capi.PROF_TOPK_DEEP)[0] > 0) == (mode == 1)
        tables.append(h.get_table(capi.NBR_HOP2))
    for a, b in zip(*tables):
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)


def test_hip_database_option():
    with pytest.raises(Exception, match="unknown option"):
        V.Open("hip://?deep_sweep=2")
    X = np.random.default_rng(8).standard_normal((900, 768)).astype(np.float32)
    answers = []
    for url in ("hip://", "hip://?deep_sweep=1", "hip://?quantization=sq&deep_sweep=1"):
        db = V.Open(url)
        db.AddCollection("c", 768, V.Euclidean)
        db.AddVectors("c", [V.Vector("v%03d" % r, X[r]) for r in range(900)])
        got = db.QueryVectorsBatch("c", X[:800], [], 7)
        answers.append([[(v.Id, np.float32(v.Score)) for v in row] for row in got])
    assert answers[0] == answers[1] == answers[2]
