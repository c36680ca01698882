"""gorse_sq, the scalar-quantised (int8) exact top-k index, held bit for bit to a numpy restatement of the semantics in
include/gorse_hip.h: int64 sums, fp32 operations in the stated order, np.lexsort for the order.  Every case fails without
csrc/sq.hip: the symbols do not exist."""
import numpy as np
import pytest

from gorse_amd import capi
from gorse_amd import vectors as V

pytestmark = pytest.mark.gpu
F = np.float32
DOT, EUC, COS = capi.METRIC_NEG_DOT, capi.METRIC_EUCLIDEAN, capi.METRIC_COSINE
STRIDE = 16  # csrc/sq_plan.hpp kBaseStride: the pilot's sample below 2^19 rows


def encode(X):
    """codes (int64), scale, sn, rn of the rows of X"""
    X = np.asarray(X, F)
    s = np.abs(X).max(1) / F(127)
    with np.errstate(all="ignore"):
        c = np.where(s[:, None] > 0, np.rint(X / s[:, None]), 0).astype(np.int64)
    sn = (s * s) * (c * c).sum(1).astype(F)
    return c, s, sn, np.sqrt(sn)


def scores(metric, q, x):
    (cq, sq, snq, rnq), (cx, sx, snx, rnx) = q, x
    p = ((cq @ cx.T).astype(F) * sx[None, :]) * sq[:, None]
    if metric == DOT:
        return p
    with np.errstate(all="ignore"):
        if metric == COS:
            den = rnq[:, None] * rnx[None, :]
            return np.where(den == 0, F(-1), p / den - F(1)).astype(F)
        return -np.sqrt(np.maximum((snq[:, None] + snx[None, :]) - (p + p), F(0)))


def lists(S, valid, k):
    nq = S.shape[0]
    idx, sc, cnt = np.full((nq, k), -1, np.int32), np.full((nq, k), -np.inf, F), np.zeros(nq, np.int32)
    for t in range(nq):
        rows = np.flatnonzero(valid[t])
        o = rows[np.lexsort((rows, -S[t, rows]))][:k]
        idx[t, :o.size], sc[t, :o.size], cnt[t] = o, S[t, o], o.size
    return idx, sc, cnt


def same(got, want):
    assert np.array_equal(got[2], want[2]), "counts"
    assert np.array_equal(got[0], want[0]), "rows"
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), "score bits"


def data(N, d, seed, distinct=None):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, d)).astype(F)
    if distinct:  # ties: few distinct rows, each many times
        X = X[rng.integers(0, min(distinct, N), N)]
    elif N > 8:
        X[N // 2], X[5] = X[1], 0  # one duplicated row, one zero row
    return X


@pytest.fixture(autouse=True)
def plan_after():
    yield
    capi.set_sq()


def run(metric, path, N, nq, k, d, form="vector", mask=None, X=None, cap=0, seed=3):
    X = data(N, d, seed) if X is None else X
    ex = encode(X)
    t = capi.SQIndex(X, metric)
    adm = np.ones(N, bool) if mask is None else mask
    t.set_mask(None if mask is None else mask.astype(np.uint8))
    capi.set_sq(path, cap)
    if form == "vector":
        Q = data(nq, d, seed + 1)
        Q[0] = X[0]
        eq, got = encode(Q), t.search_vector(Q, k)
        valid = np.broadcast_to(adm, (nq, N)).copy()
    else:
        lo = min(7, N - 1) if nq < N else 0
        hi = min(N, lo + nq)
        eq, got = tuple(a[lo:hi] for a in ex), t.search_rows(k, lo, hi, exclude_self=form == "rows_self")
        valid = np.broadcast_to(adm, (hi - lo, N)).copy()
        if form == "rows_self":
            valid[np.arange(hi - lo), np.arange(lo, hi)] = False
    S = scores(metric, eq, ex)
    same(got, lists(S, valid, k))
    return t, S, valid


@pytest.mark.parametrize("d", [1, 3, 31, 32, 33, 63, 64, 65, 200])
def test_codes_and_scales(d):
    X = data(12, d, d)
    X[0] = 0
    X[1], X[2] = np.roll(X[1], -np.argmax(np.abs(X[1]))), np.roll(X[2], d - 1 - np.argmax(np.abs(X[2])))  # maximum first / last
    X[3] = np.resize(np.array([127, 2.5, 3.5, -2.5], F), d)  # scale 1.0 from d = 1 on: quotients on halves
    X[4] = np.resize(np.array([-4, 1, 3], F), d)             # reaches -127
    c, s, _, _ = encode(X)
    got_c, got_s = capi.SQIndex(X, DOT).codes()
    assert np.array_equal(got_s.view(np.uint32), s.view(np.uint32)) and np.array_equal(got_c, c.astype(np.int8))
    assert got_c[4].min() == -127 and (d < 4 or list(got_c[3, :4]) == [127, 2, 4, -2])


CASES = [  # metric, N, nq, k, d
    (DOT, 1, 1, 1, 8), (COS, 31, 127, 10, 64), (EUC, 33, 129, 100, 96), (COS, 127, 300, 100, 128), (DOT, 129, 1, 256, 1024),
    (EUC, 513, 129, 257, 64), (COS, 4500, 127, 256, 8), (DOT, 513, 127, 10, 1056), (COS, 513, 129, 10, 1024),
    (DOT, 513, 300, 10, 96), (EUC, 513, 300, 1, 200),
    (EUC, 100000, 300, 10, 8),  # 391 tiles of 256 rows in 131 slices of three tiles
]


@pytest.mark.parametrize("path", [capi.SQ_PATH_PLAN, capi.SQ_PATH_SCAN, capi.SQ_PATH_SWEEP])
@pytest.mark.parametrize("metric,N,nq,k,d", CASES)
def test_lists(metric, N, nq, k, d, path):
    t, _, _ = run(metric, path, N, nq, k, d)
    sweep, scan, back = t.last_stats()
    assert sweep + scan == nq and back <= scan
    if path == capi.SQ_PATH_SCAN or d > 1024 or k > 256:
        assert sweep == 0


def test_saturated_codes_round_in_the_conversion():
    rng = np.random.default_rng(9)
    X = np.ones((40, 2048), F)
    for r in range(40):
        X[r, rng.integers(0, 2048, rng.integers(0, 30))] = -1
    _, S, _ = run(DOT, capi.SQ_PATH_PLAN, 40, 3, 10, 2048, form="rows", X=X)
    assert np.abs(S).max() * 127 * 127 > 2 ** 24  # |t| beyond fp32's integers


@pytest.mark.parametrize("path", [capi.SQ_PATH_SCAN, capi.SQ_PATH_SWEEP])
@pytest.mark.parametrize("metric", [DOT, EUC, COS])
def test_ties_in_ascending_row_order(metric, path):
    run(metric, path, 513, 129, 10, 64, X=data(513, 64, 4, distinct=5))


@pytest.mark.parametrize("path", [capi.SQ_PATH_SCAN, capi.SQ_PATH_SWEEP])
@pytest.mark.parametrize("form", ["rows", "rows_self"])
def test_search_rows(form, path):
    run(EUC, path, 513, 300, 10, 64, form=form)   # Euclidean: the own row scores -0
    run(COS, path, 513, 129, 10, 128, form=form, X=data(513, 128, 6, distinct=40))


@pytest.mark.parametrize("path", [capi.SQ_PATH_SCAN, capi.SQ_PATH_SWEEP])
@pytest.mark.parametrize("kind", ["best", "all", "starve"])
def test_mask(kind, path):
    N, nq = 513, 129
    mask = np.ones(N, bool)
    if kind == "best":
        mask[0] = mask[N // 2] = False  # query 0 is row 0; row N / 2 duplicates row 1
    elif kind == "all":
        mask[:] = False
    else:
        mask[::STRIDE] = False  # no admissible sampled row: every query is handed to the scan
    t, _, _ = run(COS, path, N, nq, 10, 64, mask=mask)
    if kind == "starve" and path == capi.SQ_PATH_SWEEP:
        assert t.last_stats() == (0, nq, nq)


@pytest.mark.parametrize("form", ["vector", "rows_self"])
def test_hand_back(form):
    N, nq, k, cap = 513, 129, 10, 150  # about kk * STRIDE rows reach a query's threshold: half of the lists overflow
    t, S, valid = run(DOT, capi.SQ_PATH_SWEEP, N, nq, k, 64, form=form, cap=cap)
    kk = k + (form == "rows_self")
    back = 0
    for q in range(S.shape[0]):  # tau = the kk-th best admissible sampled score; the list holds every row at or above it, the own row too
        samp = np.sort(S[q, ::STRIDE][valid[q, ::STRIDE]])[::-1]
        back += samp.size < kk or np.count_nonzero(S[q] >= samp[kk - 1]) > cap
    assert 0 < back < S.shape[0], "the case must hand some queries back and keep some"
    assert t.last_stats() == (S.shape[0] - back, back, back)


def test_errors():
    X = data(20, 16, 1)
    bad = X.copy()
    bad[3, 2] = np.nan
    for args, kw in (((bad, DOT), {}), ((X, DOT), {"bits": 4}), ((X, capi.METRIC_EUCLIDEAN_BF16), {}), ((np.zeros((2, 4097), F), DOT), {})):
        with pytest.raises(capi.GorseHipError) as e:
            capi.SQIndex(*args, **kw)
        assert e.value.code == capi.ERR_INVALID
    t = capi.SQIndex(X, DOT)
    with pytest.raises(capi.GorseHipError):
        t.search_vector(bad[:5], 3)  # a refused query leaves the index as it was
    same(t.search_rows(5), lists(scores(DOT, encode(X), encode(X)), np.ones((20, 20), bool), 5))


def test_host_mirror_opt_in():
    with pytest.raises(V.ErrNotSupported):
        V.Open("hip://").AddCollection("c", 16, V.Cosine, quantization="sq", bits=8)
    db = V.Open("hip://?quantization=sq")
    db.AddCollection("c", 16, V.Cosine, quantization="sq", bits=8)
    assert db.DescribeCollection("c")["Type"] == "sq" and db.DescribeCollection("c")["Bits"] == 8
    X = data(60, 16, 2)
    cats = [["a"] if r % 3 else ["a", "b"] for r in range(60)]
    db.AddVectors("c", [V.Vector("v%02d" % r, X[r], IsHidden=r == 3, Categories=cats[r]) for r in range(60)])
    assert db.GetVectors("c", ["v07"])[0].Values == [float(v) for v in X[7]]  # the floats, not the codes
    t = capi.SQIndex(X, COS)
    t.set_mask(np.array([r != 3 and "b" in cats[r] for r in range(60)], np.uint8))
    idx, sc, cnt = t.search_vector(X[3], 8)
    got = db.QueryVectors("c", V.Vector("q", X[3]), ["b"], 8)
    assert [v.Id for v in got] == ["v%02d" % r for r in idx[0, :cnt[0]]] and "v03" not in [v.Id for v in got]
    assert [F(v.Score) for v in got] == list(sc[0, :cnt[0]])
    batch = db.QueryVectorsBatch("c", X[:5], ["b"], 8)
    bi, _, bc = t.search_vector(X[:5], 8)
    assert [[v.Id for v in row] for row in batch] == [["v%02d" % r for r in bi[q, :bc[q]]] for q in range(5)]
