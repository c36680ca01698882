"""The accumulated tier of the Hogwild BPR schedules (csrc/hot_rows.hpp acc_rows_layout, csrc/bpr_fold.hpp run_folders / fold_acc_pass): on a
handle that takes the user-run schedule natively, has no cold item and whose item factors fit 4 MiB, every warm item's updates land in
one accumulator row behind the hot items' replica rows, and folder workgroups of the tier's own add those rows to Q inside the launch.
Checked at the smallest shape that reaches every edge (4096 users, 512 items, rows of 8), at nFactors 8 / 16 / 64 / 128, in both
Hogwild modes:
  * counts: with P = 2^-10, Q = 0, reg = 0 and lr = 2^-20 every sample moves its positive's row by exactly +2^-31 and its negative's
    by -2^-31 per element (x = 0 to fp32 precision, grad = 1/2; every sum is an integer multiple of 2^-31 far below 2^24 of them), so
    after two epochs enqueued back to back Q / 2^-31 is the signed count of the applied triplets, exactly, and every accumulator row
    reads zero;
  * one tier item as the positive of 40 samples and the negative of 40, in the user-run and in the per-sample schedule;
  * the switch: with the tier off a handle's classes are the hot codes and -1, and the hot codes are the same with it on;
  * gorse_mf_set_bpr_cold_window on a handle with the tier: no item turns cold, the classes stay;
  * 30 epochs of S-ml1m at nFactors 8, 16 and 64 stay finite and within 0.01 NDCG@10 of the sequential oracle.
"""
import numpy as np
import pytest

from gorse_amd import capi, synth
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

U, I, PER = 4096, 512, 8
VARIANT_PER_SAMPLE = 1 << 28
STEP = 2.0 ** -31


def _dataset():
    rng = np.random.default_rng(4096)
    rows = [np.sort(rng.choice(I, PER, replace=False)) for _ in range(U)]
    return np.arange(U + 1, dtype=np.int64) * PER, np.concatenate(rows).astype(np.int32)


@pytest.fixture(scope="module")
def data():
    return _dataset()


def _handle(d, uptr, uidx, tier=1):
    L = capi.lib()
    L.gorse_hip_test_set_bpr_acc_rows(tier)
    try:
        return capi.MF(U, I, d, uptr, uidx)
    finally:
        L.gorse_hip_test_set_bpr_acc_rows(-1)


def _classes(mf, items=I):
    slot, out2 = np.zeros(items, np.int32), np.zeros(2, np.int64)
    capi.check(capi.lib().gorse_hip_test_bpr_item_classes(mf.h, slot.ctypes.data, out2.ctypes.data))
    return slot, int(out2[0]), int(out2[1])


def _hot(mf):
    stats = np.zeros(3, np.int64)
    capi.check(capi.lib().gorse_hip_test_bpr_fold_stats(mf.h, stats.ctypes.data))
    n_hot, rows = int(stats[1]), int(stats[2])
    items, reps = np.zeros(n_hot, np.int32), np.zeros(n_hot, np.int32)
    capi.check(capi.lib().gorse_hip_test_bpr_hot_state(mf.h, items.ctypes.data, reps.ctypes.data, None))
    base = np.concatenate([[0], np.cumsum(reps)[:-1]]).astype(np.int64)
    codes = ((base << 4) | np.log2(reps).astype(np.int64)).astype(np.int32)
    return items, codes, rows


def _acc_state(mf, n_acc, d):
    items, rows = np.full(n_acc, -1, np.int32), np.full(n_acc * d, np.nan, np.float32)
    capi.check(capi.lib().gorse_hip_test_bpr_acc_state(mf.h, items.ctypes.data, rows.ctypes.data))
    return items, rows


def _check_layout(mf, d):
    """the handle's classes: the hot codes, and one row per other item behind the replica rows; returns (hot items, tier items)"""
    slot, n_acc, n_cold = _classes(mf)
    hot_items, hot_codes, hot_rows = _hot(mf)
    assert hot_items.size > 0 and n_cold == 0
    assert np.array_equal(slot[hot_items], hot_codes)
    warm = np.setdiff1d(np.arange(I), hot_items)
    assert n_acc == warm.size
    assert np.array_equal(slot[warm] >> 4, hot_rows + np.arange(warm.size)) and (slot[warm] & 15 == 0).all()
    items, rows = _acc_state(mf, n_acc, d)
    assert np.array_equal(items, warm) and (rows == 0).all()
    return hot_items, warm


def _signed_counts(trips):
    c = np.zeros(I, np.int64)
    for (u, i, j) in trips:
        ok = u >= 0
        c += np.bincount(i[ok], minlength=I) - np.bincount(j[ok], minlength=I)
    return c


N, SEED, BASE = 4 * U, 17, 1 << 33


@pytest.mark.parametrize("d", [8, 16, 64, 128])
@pytest.mark.parametrize("mode", [capi.BPR_HOGWILD_ATOMIC, capi.BPR_HOGWILD_STORES])
def test_counts_are_exact_and_the_rows_drained(data, d, mode):
    uptr, uidx = data
    mf = _handle(d, uptr, uidx)
    try:
        assert mf.bpr_user_runs()
        hot_items, warm = _check_layout(mf, d)
        trips = [mf.bpr_sample_triplets(N, SEED, ep, BASE) for ep in (1, 2)]
        mf.set_factors(np.full((U, d), 2.0 ** -10, np.float32), np.zeros((I, d), np.float32))
        for ep in (1, 2):  # back to back: both parities of the arrival stripes
            mf.bpr_epoch_enqueue(N, 2.0 ** -20, 0.0, SEED, ep, BASE, mode=mode)
        mf.synchronize()
        gQ = mf.get_factors()[1].astype(np.float64) / STEP
        expect = _signed_counts(trips)
        assert np.abs(expect[hot_items]).sum() > 0 and np.abs(expect[warm]).sum() > 0
        wrong = np.flatnonzero((gQ != expect[:, None].astype(np.float64)).any(axis=1))
        print("d %d mode %d: %d hot, %d tier items; rows off their count: %d" % (d, mode, hot_items.size, warm.size, wrong.size))
        assert wrong.size == 0, (wrong[:8], gQ[wrong[:8], 0], expect[wrong[:8]])
        _, rows = _acc_state(mf, warm.size, d)
        assert (rows == 0).all(), "accumulator rows not drained: %d non-zero of %d" % (int((rows != 0).sum()), rows.size)
        rep = np.full(_hot(mf)[2] * d, np.nan, np.float32)
        capi.check(capi.lib().gorse_hip_test_bpr_hot_state(mf.h, None, None, rep.ctypes.data))
        assert (rep == 0).all()
    finally:
        mf.close()


@pytest.mark.parametrize("d", [8, 16, 64, 128])
@pytest.mark.parametrize("schedule", ["user_runs", "per_sample"])
def test_a_tier_item_folds_exactly(data, d, schedule):
    """The style of test_gpu_bpr_hot_replicas.py: 40 samples with a tier item as the positive, 40 with it as the negative, 80 distinct
    users and partners, reg = 0 and a small step -- Q's row moves by the sum of the per-sample deltas computed from the initial state
    (80 deltas of random directions add up to ~9 x one of them: one lost update would show as ~10 % of the displacement).  In the
    per-sample schedule, driven on the same handle, Q is complete after the launch and its fold kernel."""
    L = capi.lib()
    uptr, uidx = data
    mf = _handle(d, uptr, uidx)
    L.gorse_hip_test_set_variant(VARIANT_PER_SAMPLE if schedule == "per_sample" else 0)
    try:
        assert mf.bpr_user_runs() == (schedule == "user_runs")
        hot_items, warm = _check_layout(mf, d)
        rng = np.random.default_rng(11 + d)
        P = rng.normal(0, 0.3, (U, d)).astype(np.float32)
        Q = rng.normal(0, 0.3, (I, d)).astype(np.float32)
        mf.set_factors(P, Q)
        x = int(warm[warm.size // 2])
        users = rng.permutation(U)[:80].astype(np.int32)
        partners = rng.permutation(np.setdiff1d(np.arange(I), [x]))[:80].astype(np.int32)
        i = np.concatenate([np.full(40, x), partners[40:]]).astype(np.int32)
        j = np.concatenate([partners[:40], np.full(40, x)]).astype(np.int32)
        lr = 1e-3
        mf.bpr_apply_triplets(users, i, j, lr, 0.0, capi.BPR_HOGWILD_ATOMIC)
        gQ = mf.get_factors()[1]
        diff = np.einsum("nd,nd->n", P[users].astype(np.float64), Q[i].astype(np.float64) - Q[j].astype(np.float64))
        step = lr / (1.0 + np.exp(diff))[:, None] * P[users].astype(np.float64)
        expect = step[i == x].sum(axis=0) - step[j == x].sum(axis=0)
        moved = gQ[x].astype(np.float64) - Q[x].astype(np.float64)
        err = np.abs(moved - expect).max() / np.abs(expect).max()
        print("%s d %d tier item %d: max |moved - expected| / max |expected| = %.2e" % (schedule, d, x, err))
        assert err < 1e-2
        touched = np.zeros(I, bool)
        touched[i] = touched[j] = True
        assert np.array_equal(gQ[~touched].view(np.uint32), Q[~touched].view(np.uint32))  # nothing else moved
        _, rows = _acc_state(mf, warm.size, d)
        assert (rows == 0).all(), "accumulator rows not drained: %d non-zero of %d" % (int((rows != 0).sum()), rows.size)
    finally:
        L.gorse_hip_test_set_variant(0)
        mf.close()


@pytest.mark.parametrize("d", [8, 64])
def test_switch_off_gives_the_classes_without_the_tier(data, d):
    uptr, uidx = data
    on, off = _handle(d, uptr, uidx, 1), _handle(d, uptr, uidx, 0)
    try:
        slot_on, n_on, _ = _classes(on)
        slot_off, n_off, n_cold = _classes(off)
        hot_items, hot_codes, _ = _hot(off)
        expect = np.full(I, -1, np.int32)
        expect[hot_items] = hot_codes
        assert n_off == 0 and n_cold == 0 and np.array_equal(slot_off, expect)
        assert n_on == I - hot_items.size and np.array_equal(slot_on[hot_items], hot_codes)  # the hot tier is the same either way
        h2 = _hot(on)
        assert np.array_equal(h2[0], hot_items) and np.array_equal(h2[1], hot_codes)
    finally:
        on.close()
        off.close()


def test_cold_window_leaves_the_tier_and_n_cold_consistent(data):
    """A window of 64 samples makes every item outside the hot set cold on a handle without the tier ((cnt / nnz + 1 / 512) x 64 < 1 for
    every share below 1.4 %); on a handle with the tier those items have a row, stay as they are, and no item is cold -- so the store
    route stays closed and the counts of an epoch in GORSE_BPR_HOGWILD_STORES are exact as before."""
    d = 16
    uptr, uidx = data
    on, off = _handle(d, uptr, uidx, 1), _handle(d, uptr, uidx, 0)
    try:
        before, n_acc, _ = _classes(on)
        n_hot = _hot(off)[0].size
        assert off.set_bpr_cold_window(64) == I - n_hot
        assert on.set_bpr_cold_window(64) == 0
        after, n_acc2, n_cold = _classes(on)
        assert np.array_equal(before, after) and n_acc2 == n_acc == I - n_hot and n_cold == 0
        trip = on.bpr_sample_triplets(N, SEED, 5, BASE)
        on.set_factors(np.full((U, d), 2.0 ** -10, np.float32), np.zeros((I, d), np.float32))
        on.bpr_epoch(N, 2.0 ** -20, 0.0, SEED, 5, BASE, mode=capi.BPR_HOGWILD_STORES)
        gQ = on.get_factors()[1].astype(np.float64) / STEP
        assert (gQ == _signed_counts([trip])[:, None].astype(np.float64)).all()
        assert (_acc_state(on, n_acc, d)[1] == 0).all()
    finally:
        on.close()
        off.close()


@pytest.mark.parametrize("d", [8, 16, 64])
def test_thirty_epochs_on_s_ml1m_with_the_tier(oracle, d):
    """The fixtures and the bound of test_gpu_bpr_positive_series.py::test_thirty_epochs_on_s_ml1m_stay_finite_and_on_the_oracle, with
    the tier on: three handles (sampler seeds), factors finite, three-seed-mean NDCG@10 within 0.01 of the sequential oracle on the
    same sampler streams."""
    oracle.set_exp(0)
    L = capi.lib()
    L.gorse_hip_test_set_exact_exp(0)
    data = synth.s_ml1m()
    lr, reg, epochs = 0.05, 0.01, 30
    P0, Q0 = synth.init_factors(data.U, data.I, d, 0.0, 0.001, 1)
    srt = orc.sort_rows(data.uptr, data.uidx)
    refs, gots = [], []
    for seed in (2024, 7, 99):
        L.gorse_hip_test_set_bpr_acc_rows(1)
        try:
            mf = capi.MF(data.U, data.I, d, data.uptr, data.uidx)
        finally:
            L.gorse_hip_test_set_bpr_acc_rows(-1)
        assert mf.bpr_user_runs()
        assert _classes(mf, data.I)[1] == 2780  # every item outside the hot set of 926
        mf.set_factors(P0, Q0)
        for ep in range(1, epochs + 1):
            mf.bpr_epoch(data.n_train, lr, reg, seed, ep, mode=capi.BPR_HOGWILD_STORES)
        gP, gQ = mf.get_factors()
        mf.close()
        assert np.isfinite(gP).all() and np.isfinite(gQ).all(), "non-finite factors, seed %d" % seed
        gots.append(float(oracle.evaluate(gP, gQ, data.test_ptr, data.test_idx, data.neg_ptr, data.neg_idx, 10)[0]))
        P, Q = P0.copy(), Q0.copy()
        for ep in range(1, epochs + 1):
            oracle.bpr_epoch_sampled(P, Q, data.uptr, data.uidx, srt, seed, ep, 0, data.n_train, lr, reg)
        refs.append(float(oracle.evaluate(P, Q, data.test_ptr, data.test_idx, data.neg_ptr, data.neg_idx, 10)[0]))
    print("d %d NDCG@10 oracle %s device %s" % (d, refs, gots))
    assert abs(float(np.mean(gots)) - float(np.mean(refs))) < 0.01
