"""Hot items with one replica row and with eight (csrc/hot_rows.hpp, csrc/bpr_fold.hpp HotRows): after ONE Hogwild update call -- in the
user-run schedule one update launch whose folders make the last pass, no fold kernel and no other launch behind it; in the per-sample
schedule the launch and its fold kernel -- Q holds every update of both items, whether it came as the positive or (user-run schedule)
as the negative, and every replica row reads zero.  The style of test_gpu_cf_parity.py::test_bpr_atomic_hot_rows_fold_exactly: reg = 0 and a
small step, so that the updates of distinct users add up to the sum of the per-sample deltas computed from the initial state."""
import ctypes as C

import numpy as np
import pytest

from gorse_amd import capi

pytestmark = pytest.mark.gpu

U, I, LEN, D = 2000, 4000, 40, 64
HOT8, HOT1 = 0, 1  # item 0 in every row (R = 8); items 1..80 in 70 rows each (R = 1 at the unit below)
UNIT = 0.002


def hooks():
    L = capi.lib()
    L.gorse_hip_test_set_bpr_replica_unit.restype, L.gorse_hip_test_set_bpr_replica_unit.argtypes = None, [C.c_double]
    L.gorse_hip_test_bpr_fold_stats.restype, L.gorse_hip_test_bpr_fold_stats.argtypes = C.c_int32, [C.c_void_p, C.c_void_p]
    L.gorse_hip_test_bpr_hot_state.restype = C.c_int32
    L.gorse_hip_test_bpr_hot_state.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def dataset():
    rng = np.random.default_rng(3)
    rows = [{HOT8} for _ in range(U)]
    for k in range(1, 81):
        for u in rng.choice(U, 70, replace=False):
            rows[u].add(k)
    for r in rows:
        while len(r) < LEN:
            r.add(int(rng.integers(81, I)))
    uidx = np.concatenate([np.sort(np.fromiter(r, np.int32)) for r in rows])
    uptr = np.zeros(U + 1, np.int64)
    uptr[1:] = np.cumsum([len(r) for r in rows])
    return uptr, uidx


@pytest.mark.parametrize("schedule", ["user_runs", "per_sample"])
def test_one_and_eight_replicas_fold_within_the_launch(schedule):
    L = hooks()
    uptr, uidx = dataset()
    L.gorse_hip_test_set_bpr_replica_unit(UNIT)
    try:
        mf = capi.MF(U, I, D, uptr, uidx)
    finally:
        L.gorse_hip_test_set_bpr_replica_unit(-1.0)
    L.gorse_hip_test_set_variant(128 if schedule == "user_runs" else 0)  # 2000 users: the per-sample schedule unless forced
    try:
        rng = np.random.default_rng(11)
        P = rng.normal(0, 0.3, (U, D)).astype(np.float32)
        Q = rng.normal(0, 0.3, (I, D)).astype(np.float32)
        mf.set_factors(P, Q)
        stats = np.zeros(3, np.int64)
        capi.check(L.gorse_hip_test_bpr_fold_stats(mf.h, stats.ctypes.data))
        n_hot, rows = int(stats[1]), int(stats[2])
        items, reps = np.zeros(n_hot, np.int32), np.zeros(n_hot, np.int32)
        capi.check(L.gorse_hip_test_bpr_hot_state(mf.h, items.ctypes.data, reps.ctypes.data, None))
        R = dict(zip(items.tolist(), reps.tolist()))
        assert n_hot == 81 and R[HOT8] == 8 and R[HOT1] == 1 and rows == reps.sum()
        # 40 samples with each hot item as the positive, 40 with each as the negative: 160 distinct users, cold partners
        users = rng.permutation(U)[:160].astype(np.int32)
        cold = (81 + rng.permutation(I - 81)[:160]).astype(np.int32)
        i = np.concatenate([np.full(40, HOT8), np.full(40, HOT1), cold[80:]]).astype(np.int32)
        j = np.concatenate([cold[:80], np.full(40, HOT8), np.full(40, HOT1)]).astype(np.int32)
        lr = 1e-3
        mf.bpr_apply_triplets(users, i, j, lr, 0.0, capi.BPR_HOGWILD_ATOMIC)
        rep = np.full(rows * D, np.nan, np.float32)
        capi.check(L.gorse_hip_test_bpr_hot_state(mf.h, None, None, rep.ctypes.data))
        capi.check(L.gorse_hip_test_bpr_fold_stats(mf.h, stats.ctypes.data))
        gQ = mf.get_factors()[1]
        diff = np.einsum("nd,nd->n", P[users].astype(np.float64), Q[i].astype(np.float64) - Q[j].astype(np.float64))
        grad = 1.0 / (1.0 + np.exp(diff))
        step = lr * grad[:, None] * P[users].astype(np.float64)
        for item in (HOT8, HOT1):
            expect = step[i == item].sum(axis=0) - step[j == item].sum(axis=0)
            moved = gQ[item].astype(np.float64) - Q[item].astype(np.float64)
            err = np.abs(moved - expect).max() / np.abs(expect).max()
            print("%s item %d (R = %d): max |moved - expected| / max |expected| = %.2e, folder passes %d"
                  % (schedule, item, R[item], err, stats[0]))
            # 80 deltas of random directions add up to ~9 x one of them: one lost update would show as ~10 % of the displacement; what
            # the small step leaves of the sequential dependence is O(lr) (the bound of the fold-exactly test)
            assert err < 1e-2
        if schedule == "user_runs":
            assert stats[0] >= 1  # the folders' last pass at least
        assert (rep == 0).all(), "replica rows not drained: %d non-zero of %d" % (int((rep != 0).sum()), rep.size)
    finally:
        L.gorse_hip_test_set_variant(0)
        mf.close()
