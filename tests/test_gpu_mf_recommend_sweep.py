"""gorse_mf_recommend under the pilot schedule (gorse_mf_set_recommend_schedule(h, 1), csrc/recommend_sweep.hip): a threshold from a
strided sample, one matrix-core sweep, exclusion and ranking on the survivors only.

The expected rows are test_gpu_mf_recommend's: numpy candidate lists ranked and scored by the oracle.  Every case runs schedule 1,
holds items, counts, padding and score bits to them, and holds the threshold / literal split both to the tie rule and to schedule 0's
on the same handle."""
import numpy as np
import pytest

import test_gpu_mf_recommend as MR
from gorse_amd import capi
from test_gpu_mf_recommend import _hooks_at_default, expected, make_mf  # noqa: F401 (the fixture resets the hooks)

pytestmark = pytest.mark.gpu


def plan(n_items, k, n_users):
    """(stride, sample size, survivor capacity) the library plans for a call of this shape"""
    import ctypes as C
    s, n, c = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    capi.lib().gorse_hip_test_recommend_sweep_plan(n_items, k, n_users, C.byref(s), C.byref(n), C.byref(c))
    return s.value, n.value, c.value


def world(n_users, n_items, d, seed=0):
    rng = np.random.default_rng(1000 * d + n_items + seed)
    P = rng.standard_normal((n_users, d)).astype(np.float32)
    Q = rng.standard_normal((n_items, d)).astype(np.float32)
    rows = [rng.choice(n_items, int(rng.integers(0, max(1, n_items // 3))), replace=False).astype(np.int32) for _ in range(n_users)]
    return P, Q, rows, rng


def run(mf, P, Q, rows, users, k, ok=None, seen=None, used=1, literal=None):
    """one schedule-1 call against the oracle and against schedule 0's split; returns (handed back, survivors, tied)"""
    exp_i, exp_s, exp_c, tied = expected(P, Q, rows, users, k, ok, seen)
    sp, si = MR.csr(seen) if seen is not None else (None, None)
    mf.set_recommend_schedule(0)
    mf.recommend(users, k, ok, sp, si)
    split0 = mf.recommend_stats()[:2]
    assert mf.recommend_schedule() == (0, 0) and mf.recommend_sweep_stats() == (0, 0, 0)
    mf.set_recommend_schedule(1)
    got_i, got_s, got_c = mf.recommend(users, k, ok, sp, si)
    assert mf.recommend_schedule() == (1, used)
    assert np.array_equal(got_c, exp_c) and np.array_equal(got_i, exp_i), np.flatnonzero((got_i != exp_i).any(axis=1))[:10]
    assert np.array_equal(got_s.view(np.uint32), exp_s.view(np.uint32))
    assert mf.recommend_stats()[:2] == split0
    if k <= MR.FAST_CAP:
        want = int(tied.sum()) if literal is None else literal
        assert split0 == (len(users) - want, want)
    n_sweep, n_back, surv = mf.recommend_sweep_stats()
    assert n_sweep + n_back == (len(users) if used else 0)
    return n_back, surv, tied


@pytest.mark.parametrize("d,k,used", [(16, 10, 1), (128, 10, 1), (256, 10, 1), (48, 257, 0), (24, 10, 0)])
def test_widths_and_whole_call_fallbacks(d, k, used):
    P, Q, rows, _ = world(140, 1000, d)
    n_back, surv, tied = run(make_mf(P, Q, rows), P, Q, rows, np.arange(140, dtype=np.int32), k, used=used)
    assert not tied.any() and (n_back == 0 and surv >= 140 * (k + 1) if used else surv == 0)


@pytest.mark.parametrize("nq,n_items,k", [(1, 1000, 1), (127, 4099, 100), (129, 4099, 256), (257, 4099, 10), (129, 33, 1)])
def test_query_blocks_items_and_k(nq, n_items, k):
    """a users array with repeats and a -1 across the 128-query block and its ragged end; item counts that are no multiple of the
    tile or the stride; unsorted seen rows with repeats that overlap the training row; an item filter that drops every second item"""
    P, Q, rows, rng = world(60, n_items, 32)
    users = rng.integers(0, 60, nq).astype(np.int32)
    users[nq // 2] = -1 if nq > 1 else users[0]
    seen = []
    for u in users:
        s = rng.integers(0, n_items, min(40, n_items // 8)).astype(np.int32)
        seen.append(np.concatenate([s, s[:3], rows[u][:5]]).astype(np.int32) if u >= 0 else np.zeros(0, np.int32))
    ok = (np.arange(n_items) % 2 == 0).astype(np.uint8) if nq == 257 else np.ones(n_items, np.uint8)
    n_back, _, _ = run(make_mf(P, Q, rows), P, Q, rows, users, k, ok=ok, seen=seen)
    assert n_back < max(2, nq // 10)  # the sweep, not schedule 0, is what answered


def test_small_catalogue_hands_every_query_back():
    """no sample of 33 items holds 101 candidates"""
    P, Q, rows, _ = world(20, 33, 16)
    users = np.arange(20, dtype=np.int32)
    n_back, surv, _ = run(make_mf(P, Q, rows), P, Q, rows, users, 100, ok=np.ones(33, np.uint8))
    assert n_back == 20 and surv == 0


def test_exclusion_edges():
    """query 0: the seen row is exactly the sampled items (handed back); query 1: its best 3 k items are all seen; query 2: plain"""
    n_items, k = 4099, 10
    P, Q, _, _ = world(3, n_items, 64)
    rows = [np.zeros(0, np.int32)] * 3
    stride, n_sample, cap = plan(n_items, k, 3)
    assert stride > 1 and n_sample * stride >= n_items
    best = np.argsort(-(Q @ P[1]))[:3 * k].astype(np.int32)
    seen = [np.arange(0, n_items, stride, dtype=np.int32), best, np.zeros(0, np.int32)]
    mf = make_mf(P, Q, rows)
    n_back, surv, _ = run(mf, P, Q, rows, np.arange(3, dtype=np.int32), k, ok=np.ones(n_items, np.uint8), seen=seen)
    assert n_back == 1 and 2 * (k + 1) <= surv <= 2 * cap
    # the same rows at another stride: results never depend on it
    capi.lib().gorse_hip_test_set_recommend_sweep(5)
    try:
        assert plan(n_items, k, 3)[0] == 5
        assert run(mf, P, Q, rows, np.arange(3, dtype=np.int32), k, ok=np.ones(n_items, np.uint8), seen=seen)[0] == 0
    finally:
        capi.lib().gorse_hip_test_set_recommend_sweep(0)


def test_ties_nan_and_overflow_reach_the_literal_path():
    n_items, k = 4099, 3
    P, Q, _, _ = world(5, n_items, 16)
    rows = [np.array([u], np.int32) for u in range(5)]
    ones = np.ones(n_items, np.uint8)
    users = np.arange(5, dtype=np.int32)
    # user 0: a zero factor row: every score ties with tau = 0, the survivor list overflows, schedule 0 finds the tie
    P[0] = 0.0
    # user 1: two identical item rows among its best (off the sample's grid: the sweep itself must find the pair)
    stride, _, cap = plan(n_items, k, 5)
    assert cap < n_items and stride > 2
    Q[stride + 1] = Q[2 * stride + 1] = 4.0 * np.sign(P[1])
    mf = make_mf(P, Q, rows)
    n_back, _, tied = run(mf, P, Q, rows, users, k, ok=ones)
    assert tied[0] and tied[1] and n_back == 1
    # a NaN in an admissible item's row, off the grid (the sweep appends it, the finish flags it) and on it (the pilot hands back)
    for item, back in ((stride + 2, 1), (3 * stride, 5)):
        Qn = Q.copy()
        Qn[item, 3] = np.nan
        mf.set_factors(P, Qn)
        assert run(mf, P, Qn, rows, users, k, ok=ones, literal=5)[0] == back
    # in an excluded item's row it sends nobody anywhere
    ok = ones.copy()
    ok[3 * stride] = 0
    assert run(mf, P, Qn, rows, users, k, ok=ok)[0] == 1


def test_candidate_chain_follows_the_handle_and_bad_schedules_are_refused():
    P, Q, rows, _ = world(140, 1000, 48)
    mf = make_mf(P, Q, rows)
    users = np.arange(0, 140, 3, dtype=np.int32)
    got = []
    for schedule in (0, 1):
        mf.set_recommend_schedule(schedule)
        chain = capi.CandidateChain(1000)
        chain.begin(users.size, 20, *MR.csr([rows[u][:30] for u in users]))
        chain.add_mf(mf, users, 15)
        chain.finish()
        got.append(chain.get())
        assert mf.recommend_schedule() == (schedule, schedule)
        chain.close()
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(*got)) and got[0][0][-1] > 0
    for bad in (2, -1):
        with pytest.raises(capi.GorseHipError) as e:
            mf.set_recommend_schedule(bad)
        assert e.value.code == capi.ERR_INVALID and mf.recommend_schedule()[0] == 1
