"""GPU parity of the tie path of a deep top-k handle (gorse_topk_set_deep_tie_replay; csrc/topk_deep_hist.hip).  Path B is forced.
Every case holds ALL rows to the same handle with the setting off (the scan answers the ties: the answer before the setting existed)
in indices, distance bits and counts, and a handful of rows -- planted ties and a few plain ones -- to the oracle."""
import numpy as np
import pytest

import topk_cases as tc
from gorse_amd import capi
from gorse_amd import vectors as V
from test_gpu_topk_deep import _paths, deep_index  # noqa: F401  (the autouse fixture: path B forced, AVX512 oracle; a mode-1 handle)
from test_gpu_topk_depths import TIE_PAIRS, TIE_RUN, bits, check_index_rows, check_vector_rows

pytestmark = pytest.mark.gpu

BF16, F32, EUCLID = tc.BF16, tc.F32, capi.METRIC_EUCLIDEAN
# the first too-deep width, a ragged last K-slice, the widest (the sort kernel's fewest staging groups); fp32: first too-deep, operand 4608
EDGE_CASES = ((BF16, 385), (BF16, 400), (BF16, 4096), (F32, 129), (F32, 1536))
SLICE_FORMS = (capi.TOPK_SLICE1, capi.TOPK_SLICES8, capi.TOPK_SLICES8 | capi.TOPK_COLD_SLICES)
PLANTED = sorted({q for p in TIE_PAIRS for q in p if q < 1024} | set(range(*TIE_RUN)))


def planted_index(dtype, d, metric):
    """the recipe of test_gpu_topk_deep.test_ties_go_to_the_scan: pairs of equal rows early and late, a run of sixteen"""
    Xf = np.random.default_rng(5300 + metric).standard_normal((24000, d)).astype(np.float32)
    for src, dst in TIE_PAIRS:
        Xf[dst] = Xf[src]
    Xf[TIE_RUN[0]:TIE_RUN[1]] = Xf[TIE_RUN[0]]
    return tc.as_index(Xf, dtype)


def off_and_on(t, search):
    """the same search with the setting off, then on: every row equal; returns the rows and both (n_fallback, n_tie)"""
    t.set_deep_tie_replay(0)
    off, stats_off = search(), t.last_stats()
    assert t.get_deep_tie_replay() == (0, 0) and stats_off[1] == 0
    t.set_deep_tie_replay(1)
    on, stats_on = search(), t.last_stats()
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(off, on))
    print("setting off: %d to the scan; on: %d to the scan, %d to the replay" % (stats_off[0], stats_on[0], stats_on[1]))
    return on, stats_off, stats_on


@pytest.mark.parametrize("metric", tc.METRICS)
@pytest.mark.parametrize("case", EDGE_CASES, ids=lambda c: "%s-d%d" % ("bf16" if c[0] == BF16 else "f32", c[1]))
def test_planted_ties_at_the_shape_edges(oracle, case, metric):
    dtype, d = case
    k, nq = 30, 1024
    X, Xe = planted_index(dtype, d, metric)
    t = deep_index(X, metric, dtype)
    rows = {}
    for form in SLICE_FORMS:
        capi.lib().gorse_hip_test_set_topk_variant(form)
        before = t.get_profile(capi.PROF_TOPK_HIST)[0]
        rows[form], (fb_off, _), (fb_on, n_tie) = off_and_on(t, lambda: t.search_index(np.arange(nq), k))
        assert t.get_profile(capi.PROF_TOPK_HIST)[0] > before and t.get_deep_tie_replay() == (1, 1)
        assert t.get_deep_sweep() == (1, 1, 1) and t.get_profile(capi.PROF_TOPK_SWEEP)[0] == 0
        assert n_tie >= TIE_RUN[1] - TIE_RUN[0] and fb_on < fb_off, (form, n_tie, fb_on, fb_off)
    idx, dist, cnt = rows[SLICE_FORMS[1]]
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(rows[SLICE_FORMS[1]], rows[SLICE_FORMS[2]]))  # warm, cold
    qs = (PLANTED + [0, 77, 512, 1016]) if d < 4096 else [3, 40, 1000, 1015, 0, 77]  # (the oracle costs a 4096-wide row the most)
    check_index_rows(oracle, Xe, metric, qs, k, idx[qs], dist[qs], cnt[qs])


# -dot and Euclidean distances of small-integer rows are integers (or their roots): most queries tie by construction.  Cosine's
# quotient of roots does not repeat that way, and the cap below is a condition on the inputs: cosine is left out here.
@pytest.mark.parametrize("metric", (capi.METRIC_NEG_DOT, EUCLID))
@pytest.mark.parametrize("shape", ((24000, 400, 40), (9000, 385, 100), (9000, 385, 255)), ids=lambda s: "n%d-d%d-k%d" % s)
def test_ties_everywhere(oracle, shape, metric):
    """long histories, many compactions, a replay chunk of a few hundred queries"""
    n, d, k = shape
    rng = np.random.default_rng(97 * k + metric)
    X, Xe = tc.as_index(rng.integers(-4, 5, (n, d)).astype(np.float32), BF16)
    qv, qe = tc.as_index(rng.integers(-4, 5, (60, d)).astype(np.float32), BF16)
    qs = rng.integers(0, n, 300).astype(np.int64)
    capi.lib().gorse_hip_test_set_topk_variant(capi.TOPK_SLICES8)
    t = deep_index(X, metric, BF16)
    for prune0 in (False, True):
        (idx, dist, cnt), _, (_, n_tie) = off_and_on(t, lambda: t.search_index(qs, k, prune0))
        assert n_tie > qs.size // 2, (prune0, n_tie)
        check_index_rows(oracle, Xe, metric, qs[::60], k, idx[::60], dist[::60], cnt[::60], prune0)
    (idx, dist, cnt), _, (_, n_tie) = off_and_on(t, lambda: t.search_vector(qv, k))
    assert n_tie > 30, n_tie
    check_vector_rows(oracle, Xe, metric, qe, range(0, 60, 12), k, idx, dist, cnt)


@pytest.mark.parametrize("nq", (1, 129))
@pytest.mark.parametrize("n", (100, 2500))
def test_edges_of_the_slice_walk(oracle, n, nq):
    """N below one tile (seven of eight slices are empty) and a last tile mostly past N; one query and a ragged 128-query block"""
    Xf = np.random.default_rng(n + nq).standard_normal((n, 385)).astype(np.float32)
    Xf[[7, n - 1]] = Xf[0]  # queries 0 and 7 see two equal distances at the top
    X, Xe = tc.as_index(Xf, BF16)
    qs = np.arange(nq, dtype=np.int64) % n
    capi.lib().gorse_hip_test_set_topk_variant(capi.TOPK_SLICES8)
    t = deep_index(X, EUCLID, BF16)
    (idx, dist, cnt), _, (_, n_tie) = off_and_on(t, lambda: t.search_index(qs, tc.DEPTH_K))
    assert n_tie >= 1 and t.get_deep_tie_replay() == (1, 1)
    check_index_rows(oracle, Xe, EUCLID, qs, tc.DEPTH_K, idx, dist, cnt)


def test_what_still_goes_to_the_scan(oracle):
    """700 copies of one row (test_gpu_topk_mfma.test_duplicates_and_overflowing_lists at d = 385): lists and histories overflow.
    A mask: the replay counts the rows between two recorded ones, masked rows included, so every tie query takes the scan"""
    rng = np.random.default_rng(5)
    Xf = np.concatenate([np.tile(rng.standard_normal((1, 385)), (700, 1)), rng.standard_normal((300, 385))]).astype(np.float32)
    X, Xe = tc.as_index(Xf, BF16)
    t = deep_index(X, capi.METRIC_NEG_DOT, BF16)
    (idx, dist), _, (n_fb, _) = off_and_on(t, lambda: t.all_pairs(10))
    assert n_fb > 0
    qs = [0, 1, 699, 700, 850, 999]
    check_index_rows(oracle, Xe, capi.METRIC_NEG_DOT, qs, 10, idx[qs], dist[qs])
    k = tc.DEPTH_K
    X = tc.depth_inputs(F32, 129, EUCLID, k)[0].copy()
    X[[10, 20]] = X[30]
    ok = np.random.default_rng(17).random(X.shape[0]) < 0.6
    ok[[10, 20, 30]] = True
    keep = np.nonzero(ok)[0]
    t = deep_index(X, EUCLID, F32)
    t.set_deep_tie_replay(1)
    t.set_mask(ok.astype(np.uint8))
    idx, dist, cnt = t.search_vector(X[25:65].copy(), k)  # row 30's vector among them: rows 10, 20 and 30 tie at its top
    assert t.last_stats()[0] >= 1 and t.last_stats()[1] == 0 and t.get_deep_tie_replay() == (1, 0)
    for r in range(40):
        ei, ed = oracle.search_vector(X[keep], EUCLID, X[25 + r], k)
        assert cnt[r] == ei.size == k and np.array_equal(idx[r], keep[ei]) and np.array_equal(bits(dist[r]), bits(ed)), r


def test_small_calls_reroute_their_ties(oracle):
    """path hook 0, 64 queries: the scan answers, and hands its tie queries to path B only when the deep handle has a tie path"""
    capi.lib().gorse_hip_test_set_topk_path(0)
    X, Xe = planted_index(BF16, 400, capi.METRIC_NEG_DOT)
    qs = np.array((PLANTED + list(range(100, 164)))[:64], np.int64)
    t = deep_index(X, capi.METRIC_NEG_DOT, BF16)
    (idx, dist, cnt), (_, tie_off), (_, tie_on) = off_and_on(t, lambda: t.search_index(qs, 30))
    assert tie_off == 0 and tie_on > 0 and t.get_profile(capi.PROF_TOPK_SCORE)[0] > 0 and t.get_deep_tie_replay() == (1, 1)
    check_index_rows(oracle, Xe, capi.METRIC_NEG_DOT, qs[:30], 30, idx[:30], dist[:30], cnt[:30])


def test_interface(oracle):
    rng = np.random.default_rng(3)
    Xf = rng.standard_normal((1500, 128)).astype(np.float32)
    Xf[[9, 1400]] = Xf[2]
    X, Xe = tc.as_index(Xf, BF16)
    t = deep_index(X, EUCLID, BF16)  # path B serves it already: the setting is accepted and inert, the shallow tie path runs
    t.set_deep_tie_replay(1)
    idx, dist = t.all_pairs(5)
    assert t.get_deep_sweep() == (1, 0, 0) and t.get_deep_tie_replay() == (1, 0) and t.last_stats()[1] >= 3
    check_index_rows(oracle, Xe, EUCLID, [2, 9, 1400], 5, idx[[2, 9, 1400]], dist[[2, 9, 1400]])
    with pytest.raises(capi.GorseHipError) as e:
        t.set_deep_tie_replay(2)
    assert e.value.code == capi.ERR_INVALID and t.get_deep_tie_replay()[0] == 1
    with pytest.raises(Exception, match="deep_ties=1 needs deep_sweep=1"):
        V.Open("hip://?deep_ties=1")
    Xd = rng.standard_normal((900, 768)).astype(np.float32)
    Xd[[5, 800]] = Xd[3]
    answers = []
    for url in ("hip://", "hip://?deep_sweep=1&deep_ties=1"):
        db = V.Open(url)
        db.AddCollection("c", 768, V.Euclidean)
        db.AddVectors("c", [V.Vector("v%03d" % r, Xd[r]) for r in range(900)])
        answers.append([[(v.Id, np.float32(v.Score)) for v in row] for row in db.QueryVectorsBatch("c", Xd[:800], [], 7)])
    assert answers[0] == answers[1]
