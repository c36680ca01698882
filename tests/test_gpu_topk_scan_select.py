"""GPU parity of the SELECTION of top-k path A (gorse_amd/csrc/topk.hip: select_fast_kernel, the literal select_kernel behind it,
the reroute of tie queries through path B, and the block loop of the three calls) against the oracle: ids, fp32 distance bits,
counts, -1 / +inf padding and both prune0 values, bit for bit -- there is no tolerance in this file.

select_fast_kernel: 1024 threads stride a query's row of the distance slab and keep their 4 smallest keys; the (k + 1)-th smallest
kept key bounds the true one from above; a second pass collects the rows up to that bound into 2048 LDS slots, sorts them and looks
for equal neighbours.  A NaN, k + 1 > 1024 or more than 2048 rows at the bound leave the query to the literal kernel.  After every
call the test reads which kernel answered (gorse_hip_test_topk_scan_flags) and asserts the path the case was built for; every
constructed case runs in the default state, with the literal-only switch (the same bits) and with path B switched off, so that the
literal kernel and not the reroute arbitrates.  tests/test_topk_scan_cases_cpu.py holds the inputs against the oracle alone."""
import functools

import numpy as np
import pytest

import topk_cases as tc
from gorse_amd import capi
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

FAST, LITERAL = 0, 1
MODES = ("default", "literal_only", "path_b_off")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def set_mode(mode="default"):
    L = capi.lib()
    L.gorse_hip_test_set_scan_literal(int(mode == "literal_only"))
    L.gorse_hip_test_set_topk_path(int(mode == "path_b_off"))


@pytest.fixture(autouse=True)
def _reset(oracle):
    oracle.set_isa(orc.ISA_AVX512)
    set_mode()
    capi.lib().gorse_hip_test_set_scan_block(0)
    yield
    set_mode()
    capi.lib().gorse_hip_test_set_scan_block(0)


def want_rows(oracle, Xe, metric, queries, k, prune0=False, ids=None):
    """the oracle's answer as the handle lays it out; a query is a stored row's position in Xe (itself left out) or a vector"""
    nq = len(queries)
    idx, dist, cnt = np.full((nq, k), -1, np.int32), np.full((nq, k), np.inf, np.float32), np.zeros(nq, np.int32)
    for r, q in enumerate(queries):
        if Xe.shape[0] == 0:  # an index without admissible rows answers nothing
            continue
        if np.ndim(q) == 0:
            ei, ed = oracle.search_index(Xe, metric, int(q), k, prune0)
        else:
            ei, ed = oracle.search_vector(Xe, metric, q, k, prune0)
        n = ei.size
        idx[r, :n], dist[r, :n], cnt[r] = (ei if ids is None else ids[ei]), ed, n
    return idx, dist, cnt


def assert_same(got, want, what, nan_bits=True):
    """ids, distance bits, counts, padding; nan_bits=False: where the oracle's distance is a NaN, a NaN of any sign and payload
    (test_nan_distances_carry_the_reference_sign compares those bits)"""
    assert np.array_equal(got[0], want[0]), what
    differ = bits(got[1]) != bits(want[1])
    if not nan_bits:
        differ &= ~(np.isnan(got[1]) & np.isnan(want[1]))
    bad = np.nonzero(differ)
    assert bad[0].size == 0, (what, bad, ["%08x != %08x" % (a, b) for a, b in zip(bits(got[1])[bad][:8], bits(want[1])[bad][:8])])
    if len(got) > 2 and got[2] is not None:
        assert np.array_equal(got[2], want[2]), what


def three_ways(t, call, want, path, what, modes=MODES, nan_bits=True):
    """call() in every mode against the oracle's rows; path = the expected flag of every query (FAST / LITERAL), or one for all"""
    nq = want[0].shape[0]
    path = np.broadcast_to(np.asarray(path, np.int32), (nq,))
    for mode in modes:
        set_mode(mode)
        got = call()
        flags = t.scan_flags(nq)
        assert_same(got, want, (what, mode), nan_bits)
        assert np.array_equal(flags, np.ones(nq, np.int32) if mode == "literal_only" else path), (what, mode, flags)
    set_mode()


# ---- signed zero ----

@pytest.mark.parametrize("dtype", [tc.F32, tc.BF16], ids=["f32", "bf16"])
def test_negative_zero_distance_keeps_its_sign(oracle, dtype):
    """-floats.Dot of an orthogonal pair is -0.0 (logics/cf.go:33): the fast kernel orders it as +0 and returns it as it is stored.
    Before the fix (select_fast_kernel wrote the distance rebuilt from its ordering key, which folds -0 onto +0) the first
    comparison here, the six-row search_vector in the default state, failed in both dtypes with 00000000 at rank 3 where the oracle
    has 80000000."""
    (X6, qv6, k6), (X40, qi, k40) = tc.signed_zero_cases()
    X, Xe = tc.as_index(X6, dtype)
    qv, qe = tc.as_index(qv6[None, :], dtype)
    t = capi.TopK(X, capi.METRIC_NEG_DOT, dtype=dtype)
    for prune0 in (False, True):
        want = want_rows(oracle, Xe, capi.METRIC_NEG_DOT, list(qe), k6, prune0)
        if not prune0:
            assert want[0][0].tolist() == [4, 2, 1, 0, 3] and bits(want[1])[0, 3] == 0x80000000
        three_ways(t, lambda: t.search_vector(qv, k6, prune0), want, FAST, ("six rows", prune0))
    X, Xe = tc.as_index(X40, dtype)
    t = capi.TopK(X, capi.METRIC_NEG_DOT, dtype=dtype)
    for prune0 in (False, True):
        want = want_rows(oracle, Xe, capi.METRIC_NEG_DOT, [qi], k40, prune0)
        assert prune0 or int((bits(want[1]) == 0x80000000).sum()) == 1
        three_ways(t, lambda: t.search_index([qi], k40, prune0), want, FAST, ("forty rows", prune0))
    want = want_rows(oracle, Xe, capi.METRIC_NEG_DOT, list(range(40)), k40)
    for mode in MODES:  # the other rows' queries may tie: whichever kernel answers them, the oracle's rows
        set_mode(mode)
        got = t.all_pairs(k40)
        assert_same(got, want, ("all pairs", mode))
        assert mode == "literal_only" or t.scan_flags(40)[qi] == FAST


# ---- the bound: concentrated strides, plateaus ----

@pytest.mark.parametrize("metric", tc.METRICS)
@pytest.mark.parametrize("k", tc.SEL_KS)
def test_best_rows_in_one_stride_are_fetched_by_the_second_pass(oracle, k, metric):
    """the k + 6 best rows in ONE thread's stride: it keeps 4, the bound comes from the others' background rows, the second pass
    collects planted rows that no thread kept"""
    X, planted = tc.concentrated_case(metric, k)
    qv = tc.sel_queries()
    t = capi.TopK(X, metric)
    for prune0 in (False, True):
        want = want_rows(oracle, X, metric, list(qv), k, prune0)
        assert prune0 or np.isin(want[0], planted).all()
        three_ways(t, lambda: t.search_vector(qv, k, prune0), want, FAST, (metric, k, prune0))


@pytest.mark.parametrize("metric", tc.METRICS)
@pytest.mark.parametrize("k", tc.SEL_KS)
@pytest.mark.parametrize("variant", ["A", "B"])
def test_plateau_at_the_bound(oracle, variant, k, metric):
    """every row but the planted ones is one row.  A: planted in one stride -- the bound lands on the plateau, more than 2048 rows
    lie at it, the query goes literal.  B: one planted row per stride -- the bound is exact and the fast kernel answers."""
    X, planted = tc.plateau_case(metric, k, variant)
    qv = tc.sel_queries()
    t = capi.TopK(X, metric)
    for prune0 in (False, True):
        want = want_rows(oracle, X, metric, list(qv), k, prune0)
        assert prune0 or np.isin(want[0], planted).all()
        three_ways(t, lambda: t.search_vector(qv, k, prune0), want, LITERAL if variant == "A" else FAST, (metric, k, variant, prune0))


# ---- the stride's edges ----

@pytest.mark.parametrize("metric", tc.METRICS)
@pytest.mark.parametrize("N", tc.STRIDE_NS)
def test_row_counts_around_the_1024_thread_stride(oracle, N, metric):
    X, qs, qv = tc.stride_case(N, metric)
    t = capi.TopK(X, metric)
    for k in tc.STRIDE_KS:
        for prune0 in (False, True):
            assert_same(t.search_index(qs, k, prune0), want_rows(oracle, X, metric, list(qs), k, prune0), (N, k, prune0, "index"))
            assert_same(t.search_vector(qv, k, prune0), want_rows(oracle, X, metric, list(qv), k, prune0), (N, k, prune0, "vector"))


# ---- k at the buffer rule ----

@pytest.mark.parametrize("metric", tc.METRICS)
@pytest.mark.parametrize("k", tc.KCAP_KS)
def test_k_at_the_buffer_rule(oracle, k, metric):
    """k + 1 == 1024 is half the buffer and the last k the fast kernel answers; from k = 1024 on, and with k = N + 3, every query is
    the literal kernel's (path B stops at k + 1 = 256, so nothing is rerouted)"""
    X, qs, qv = tc.kcap_case(metric, k)
    path = FAST if k + 1 <= tc.SEL_CAP // 2 else LITERAL
    t = capi.TopK(X, metric)
    for prune0 in (False, True):
        three_ways(t, lambda: t.search_index(qs, k, prune0), want_rows(oracle, X, metric, list(qs), k, prune0), path, (metric, k, prune0))
    three_ways(t, lambda: t.search_vector(qv, k), want_rows(oracle, X, metric, list(qv), k), path, (metric, k, "vector"))


# ---- skewed masks ----

@functools.lru_cache(maxsize=1)
def mask_inputs():
    return tc.mask_case()


@pytest.mark.parametrize("metric", tc.METRICS)
@pytest.mark.parametrize("name", tc.MASK_NAMES)
def test_skewed_masks(oracle, name, metric):
    """the admissible rows in one or two strides (fewer kept keys than k + 1: the bound saturates and everything is collected), exactly
    k - 1, k and k + 1 of them, none at all, and a query by index whose own row the mask hides: ann.Bruteforce over the admissible
    rows alone, ids unchanged"""
    X, qv, masks, hidden = mask_inputs()
    k, mask = tc.MASK_K, masks[name]
    rows = np.nonzero(mask)[0]
    sub = np.ascontiguousarray(X[rows])
    t = capi.TopK(X, metric)
    t.set_mask(mask)
    for prune0 in (False, True):
        want = want_rows(oracle, sub, metric, list(qv), k, prune0, ids=rows)
        assert prune0 or (want[2] == min(k, rows.size)).all()
        three_ways(t, lambda: t.search_vector(qv, k, prune0), want, FAST, (metric, name, prune0, "vector"))
    # by index: admissible rows (their positions in the sub-index), and a row the mask hides (then nothing is left out)
    mq = rows[::max(1, rows.size // 5)][:5]
    queries = [int(p) for p in np.searchsorted(rows, mq)] + [X[hidden]]
    qs = np.concatenate([mq, [hidden]]).astype(np.int64)
    assert not mask[hidden]
    want = want_rows(oracle, sub, metric, queries, k, ids=rows)
    three_ways(t, lambda: t.search_index(qs, k), want, FAST, (metric, name, "index"))


# ---- non-finite ----

def nonfinite_calls(oracle, t, metric, prune0s=(False, True)):
    """(call, the oracle's rows, expected path, label) of every call of the non-finite case; the handle's mask is set by the call"""
    X, qs, qv, masks = tc.nonfinite_case()
    k = tc.NONFINITE_K
    for name, mask in [("no mask", None)] + list(masks.items()):
        rows = np.arange(X.shape[0]) if mask is None else np.nonzero(mask)[0]
        sub = np.ascontiguousarray(X[rows])
        nan_left = mask is None or (name == "nan_hidden" and metric == capi.METRIC_COSINE)
        for prune0 in prune0s:
            def by_index(mask=mask, prune0=prune0):
                t.set_mask(mask)
                return t.search_index(qs, k, prune0)

            def by_vector(mask=mask, prune0=prune0):
                t.set_mask(mask)
                return t.search_vector(qv, k, prune0)

            want = want_rows(oracle, sub, metric, [int(p) for p in np.searchsorted(rows, qs)], k, prune0, ids=rows)
            yield by_index, want, LITERAL if nan_left else FAST, (metric, name, prune0, "index")
            want = want_rows(oracle, sub, metric, list(qv), k, prune0, ids=rows)
            yield by_vector, want, LITERAL if nan_left else FAST, (metric, name, prune0, "vector")


@pytest.mark.parametrize("metric", tc.METRICS)
def test_nan_rows_go_literal_and_hidden_ones_do_not(oracle, metric):
    """a NaN distance makes every comparison of the heap false: the query is the literal kernel's.  Behind a mask that hides the row
    the fast kernel answers, the overflowed +-inf distances being ordinary keys; the cosine distance to a row with an infinite
    entry is inf / inf, a NaN of its own.  The NaN row stays in every unmasked list: here its distance is a NaN where the oracle's
    is; its bits are the next test's."""
    t = capi.TopK(tc.nonfinite_case()[0], metric)
    seen_nan = 0
    for call, want, path, what in nonfinite_calls(oracle, t, metric):
        three_ways(t, call, want, path, what, nan_bits=False)
        seen_nan += int(np.isnan(want[1]).sum())
    assert seen_nan >= 9  # one per unmasked query without prune0


@pytest.mark.parametrize("metric", tc.METRICS)
def test_nan_distances_carry_the_reference_sign(oracle, metric):
    """The same calls with the NaN distances compared bit for bit.  Before ref_sub / cosine_distance (csrc/topk_internal.hpp) the
    Euclidean and the cosine distance to the NaN row came back as ffc00000 where the oracle (and the reference on x86) has 7fc00000,
    ids, counts and every other distance agreeing: v_sub_f32 applies its negation to a NaN in the second operand (measured on the
    device: 1.0f - NaN(7fc00000) = ffc00000; sqrtf, the product and the quotient keep the sign), x86's subss / vsubps return the NaN
    operand unchanged.  -floats.Dot has no subtraction and agreed all along (ffc00000 on both sides)."""
    t = capi.TopK(tc.nonfinite_case()[0], metric)
    for call, want, path, what in nonfinite_calls(oracle, t, metric, prune0s=(False,)):
        three_ways(t, call, want, path, what)


# ---- the reroute ----

@pytest.mark.parametrize("metric", [capi.METRIC_NEG_DOT, capi.METRIC_EUCLIDEAN])
def test_tie_queries_are_replayed_by_path_b_unless_masked(oracle, metric):
    """small-integer rows: the fast kernel flags the tie queries, and fewer than 768 queries without a mask send them through path
    B's history sweep and heap replay, not through the one-thread-per-query kernel; with a mask nothing is rerouted"""
    X, qs, mask = tc.reroute_case()
    k = tc.REROUTE_K
    t = capi.TopK(X, metric)
    for prune0 in (False, True):
        got = t.search_index(qs, k, prune0)
        flags, (n_fallback, n_tie) = t.scan_flags(qs.size), t.last_stats()
        assert_same(got, want_rows(oracle, X, metric, list(qs), k, prune0), (metric, prune0))
        print("metric %d prune0 %d: %d of %d queries flagged, %d replayed, %d left to the literal scan" %
              (metric, prune0, flags.sum(), qs.size, n_tie, n_fallback))
        assert flags.sum() > qs.size // 2 and set(flags.tolist()) <= {0, 1}
        assert n_tie > 0 and n_tie + n_fallback == flags.sum()
    rows = np.nonzero(mask)[0]
    sub = np.ascontiguousarray(X[rows])
    tm = capi.TopK(X, metric)  # a fresh handle: its counters have seen no replay
    tm.set_mask(mask)
    mq = rows[:40]
    got = tm.search_index(mq, k)
    assert_same(got, want_rows(oracle, sub, metric, list(range(40)), k, ids=rows), (metric, "masked"))
    assert tm.scan_flags(40).sum() > 20 and tm.last_stats() == (0, 0)


# ---- the block loop ----

@pytest.mark.parametrize("metric", tc.METRICS)
@pytest.mark.parametrize("dtype", [tc.F32, tc.BF16], ids=["f32", "bf16"])
def test_block_loop_of_the_three_calls(oracle, dtype, metric):
    """7 queries per block: all_pairs in 43 blocks with a partial last one, search_index over 100 unordered repeated ids, search_vector
    over 50 vectors (cosine: the query norms are recomputed per block; bf16: the vectors are expanded per block) -- the oracle's
    rows, and the bits of the same calls in one block"""
    X, Xe, qs, qv, qe = tc.block_case(dtype)
    k, N = tc.BLOCK_K, tc.BLOCK_N
    t = capi.TopK(X, metric, dtype=dtype)
    set_mode("path_b_off")
    L = capi.lib()
    out = {}
    for block in (tc.BLOCK_QUERIES, 0):
        L.gorse_hip_test_set_scan_block(block)
        out[block] = [t.all_pairs(k), t.search_index(qs, k), t.search_index(qs, k, True), t.search_vector(qv, k)]
        if block:  # the hook reports the LAST block: 50 = 7 * 7 + 1 vectors
            assert t.scan_flags(50 % block).size == 1
            with pytest.raises(capi.GorseHipError) as e:
                t.scan_flags(50 % block + 1)
            assert e.value.code == capi.ERR_INVALID
            t.all_pairs(k)
            assert t.scan_flags(N % block).size == N % block == 6
            with pytest.raises(capi.GorseHipError):
                t.scan_flags(block)
        else:
            assert t.scan_flags(50).size == 50
    want = [want_rows(oracle, Xe, metric, list(range(N)), k), want_rows(oracle, Xe, metric, list(qs), k),
            want_rows(oracle, Xe, metric, list(qs), k, True), want_rows(oracle, Xe, metric, list(qe), k)]
    for a, b, w, what in zip(out[tc.BLOCK_QUERIES], out[0], want, ("all_pairs", "index", "index prune0", "vector")):
        assert_same(a, w, (what, "blocks of 7"))
        assert_same(b, w, (what, "one block"))
        assert_same(a, b, (what, "7 against one"))


def test_two_blocks_at_the_grid_limit(oracle):
    """65535 + 40 query vectors without the hook: two blocks at the real constant, the second one's rows behind 65535 * k"""
    rng = np.random.default_rng(65535)
    N, d, k, nq = 64, 3, 5, tc.GRID_Y + 40
    X = rng.standard_normal((N, d)).astype(np.float32)
    qv = rng.standard_normal((nq, d)).astype(np.float32)
    t = capi.TopK(X, capi.METRIC_EUCLIDEAN)
    set_mode("path_b_off")  # this many queries would take the MFMA sweep
    got = t.search_vector(qv, k)
    assert t.scan_flags(40).size == 40
    with pytest.raises(capi.GorseHipError):
        t.scan_flags(41)  # the last block had 40 queries
    at = np.concatenate([np.arange(tc.GRID_Y - 40, tc.GRID_Y + 40), np.arange(nq - 10, nq)])
    assert at.size == 90 and at[-1] == nq - 1
    want = want_rows(oracle, X, capi.METRIC_EUCLIDEAN, list(qv[at]), k)
    assert_same(tuple(a[at] for a in got), want, "around the block boundary and at the end")
    assert (got[2] == k).all() and (got[0] >= 0).all() and (got[0] < N).all()


def test_scan_flags_refuses_a_call_that_did_not_scan():
    rng = np.random.default_rng(1)
    X = rng.standard_normal((900, 16)).astype(np.float32)
    t = capi.TopK(X, capi.METRIC_NEG_DOT)
    with pytest.raises(capi.GorseHipError) as e:
        t.scan_flags(1)  # no call yet
    assert e.value.code == capi.ERR_INVALID
    t.search_index(np.arange(5), 3)
    assert t.scan_flags(5).tolist() == [0] * 5
    capi.lib().gorse_hip_test_set_topk_path(2)  # the MFMA sweep answers, and Gaussian rows leave it nothing to hand back
    t.search_index(np.arange(5), 3)
    assert t.last_stats()[0] == 0
    with pytest.raises(capi.GorseHipError) as e:
        t.scan_flags(1)
    assert e.value.code == capi.ERR_INVALID
