"""The sole-writer fold of the BPR user-run launches (csrc/bpr_fold.hpp, above HotRows; csrc/hot_rows.hpp fold_share): on a handle with the
accumulated tier no worker writes Q, and the launch's folders fold with loads and stores -- Q <- base + the slot's rows, base = the
row as the launch found it -- instead of an exchange and an atomic add per pass.  The shape and the counting trick are those of
tests/test_gpu_bpr_acc_rows.py (4096 users, 512 items, rows of 8; P = 2^-10, reg = 0, lr = 2^-20: every sample moves its positive's row
by exactly +2^-31 per element and its negative's by -2^-31), here from a NON-ZERO start, Q0[i, :] = (i % 7 - 3) x 2^-28: a fold that
forgets base, or takes it after a fold, is then wrong by an exact multiple of 8 steps, which a start from zero cannot show.
The start's scale.  The trick needs x = p . (q_i - q_j) = 0 to fp32 precision, so that grad = exp(-x) / (1 + exp(-x)) is exactly 1/2:
exp(-x) rounds to 1 only for x < 2^-25.  A start of (i % 7 - 3) x 2^-20 gives x = nFactors x 2^-10 x (up to 6) x 2^-20 -- 1.5 x 2^-25
at nFactors 8, 1.5 x 2^-21 at 128 -- and the steps are then 2^-31 x (1 - up to 3.6e-7), no multiple of 2^-31, in either form of the
fold; at 2^-28 the start adds at most 1.5 x 2^-29 to x at nFactors 128, far below the counts' own drift that test_gpu_bpr_acc_rows.py
already runs with, and every sum is an exact multiple of 2^-31.
  1. many passes: fold period and the tier's cadence at 1 tick, two epochs back to back; each tier made >= 3 passes in the last launch;
  2. base is per launch: other exact factors set between two epochs;
  3. several launches per epoch (chunks of a quarter epoch);
  4. leftovers: a launch whose folders time out at once leaves updates in the rows, the next launch folds them in;
  5. the atomic fold is still what the other launches take: the per-sample kernel on the same handle, and a handle without the tier.
Every test restores the hooks it sets."""
import numpy as np
import pytest

from gorse_amd import capi

pytestmark = pytest.mark.gpu

U, I, PER = 4096, 512, 8
VARIANT_PER_SAMPLE = 1 << 28
STEP = 2.0 ** -31
N, SEED, BASE = 4 * U, 17, 1 << 33
LR = 2.0 ** -20
MODES = [capi.BPR_HOGWILD_ATOMIC, capi.BPR_HOGWILD_STORES]
WIDTHS = [8, 16, 64, 128]


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(4096)
    rows = [np.sort(rng.choice(I, PER, replace=False)) for _ in range(U)]
    return np.arange(U + 1, dtype=np.int64) * PER, np.concatenate(rows).astype(np.int32)


def _start(d, shift=0):
    """exact non-zero item factors: (i % 7 - 3) x 2^-28, every element of a row the same (`shift` moves the pattern along the items)"""
    k = ((np.arange(I) + shift) % 7 - 3).astype(np.float32) * np.float32(2.0 ** -28)
    return np.repeat(k[:, None], d, axis=1)


def _handle(d, uptr, uidx, tier=1):
    L = capi.lib()
    L.gorse_hip_test_set_bpr_acc_rows(tier)
    try:
        mf = capi.MF(U, I, d, uptr, uidx)
    finally:
        L.gorse_hip_test_set_bpr_acc_rows(-1)
    mf.set_factors(np.full((U, d), 2.0 ** -10, np.float32), _start(d))
    return mf


def _tier_stats(mf):
    """hot passes, tier passes, hot items, replica rows, tier rows, sole-writer form -- of the last update launch with folders"""
    out = np.zeros(6, np.int64)
    capi.check(capi.lib().gorse_hip_test_bpr_fold_tier_stats(mf.h, out.ctypes.data))
    return [int(x) for x in out]


def _signed_counts(trips):
    c = np.zeros(I, np.int64)
    for (u, i, j) in trips:
        ok = u >= 0
        c += np.bincount(i[ok], minlength=I) - np.bincount(j[ok], minlength=I)
    return c


def _check_exact(mf, d, Q0, trips, what):
    """Q / 2^-31 == Q0 / 2^-31 + signed counts for every element; every replica and accumulator row zero"""
    _, _, n_hot, hot_rows, n_acc, _ = _tier_stats(mf)
    got = mf.get_factors()[1].astype(np.float64) / STEP
    expect = Q0.astype(np.float64) / STEP + _signed_counts(trips)[:, None].astype(np.float64)
    wrong = np.flatnonzero((got != expect).any(axis=1))
    print("%s d %d: %d hot items, %d tier rows; rows off their count: %d" % (what, d, n_hot, n_acc, wrong.size))
    assert wrong.size == 0, (what, wrong[:8], got[wrong[:8], 0], expect[wrong[:8], 0])
    if n_acc:
        rows = np.full(n_acc * d, np.nan, np.float32)
        capi.check(capi.lib().gorse_hip_test_bpr_acc_state(mf.h, None, rows.ctypes.data))
        assert (rows == 0).all(), "accumulator rows not drained: %d non-zero of %d" % (int((rows != 0).sum()), rows.size)
    rep = np.full(hot_rows * d, np.nan, np.float32)
    capi.check(capi.lib().gorse_hip_test_bpr_hot_state(mf.h, None, None, rep.ctypes.data))
    assert (rep == 0).all(), "replica rows not drained"


@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("mode", MODES)
def test_many_passes(data, d, mode):
    L = capi.lib()
    mf = _handle(d, *data)
    L.gorse_hip_test_set_bpr_fold_period(1)
    L.gorse_hip_test_set_bpr_acc_fold_every(1)
    try:
        assert mf.bpr_user_runs() and _tier_stats(mf)[2] > 0 and _tier_stats(mf)[4] > 0
        trips = [mf.bpr_sample_triplets(N, SEED, ep, BASE) for ep in (1, 2)]
        for ep in (1, 2):
            mf.bpr_epoch_enqueue(N, LR, 0.0, SEED, ep, BASE, mode=mode)
        mf.synchronize()
        hot_passes, acc_passes, _, _, _, sole = _tier_stats(mf)
        print("d %d mode %d: passes of the last launch: hot tier %d, accumulated tier %d" % (d, mode, hot_passes, acc_passes))
        assert sole == 1
        assert hot_passes >= 3 and acc_passes >= 3
        _check_exact(mf, d, _start(d), trips, "many passes, mode %d" % mode)
    finally:
        L.gorse_hip_test_set_bpr_fold_period(0)
        L.gorse_hip_test_set_bpr_acc_fold_every(0)
        mf.close()


@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("mode", MODES)
def test_base_is_taken_per_launch(data, d, mode):
    mf = _handle(d, *data)
    try:
        mf.bpr_epoch(N, LR, 0.0, SEED, 1, BASE, mode=mode)
        Q1 = _start(d, shift=2)
        mf.set_factors(None, Q1)
        trip = mf.bpr_sample_triplets(N, SEED, 2, BASE)
        mf.bpr_epoch(N, LR, 0.0, SEED, 2, BASE, mode=mode)
        assert _tier_stats(mf)[5] == 1
        _check_exact(mf, d, Q1, [trip], "other factors between two epochs, mode %d" % mode)
    finally:
        mf.close()


@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("mode", MODES)
def test_several_launches_per_epoch(data, d, mode):
    L = capi.lib()
    L.gorse_hip_test_set_bpr_chunk(N // 4)  # (before the handle's first epoch sizes its chunk buffers)
    mf = None
    try:
        mf = _handle(d, *data)
        trips = [mf.bpr_sample_triplets(N, SEED, ep, BASE) for ep in (1, 2)]
        mf.set_profiling(True)
        mf.reset_profile()
        for ep in (1, 2):
            mf.bpr_epoch_enqueue(N, LR, 0.0, SEED, ep, BASE, mode=mode)
        mf.synchronize()
        launches = mf.get_profile(capi.PROF_BPR_UPDATE)[0]
        mf.set_profiling(False)
        assert launches >= 2 * 3, launches
        assert _tier_stats(mf)[5] == 1
        _check_exact(mf, d, _start(d), trips, "%d launches, mode %d" % (launches, mode))
    finally:
        L.gorse_hip_test_set_bpr_chunk(0)
        if mf is not None:
            mf.close()


@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("mode", MODES)
def test_leftovers_of_a_timed_out_fold_reach_q_in_the_next_launch(data, d, mode):
    L = capi.lib()
    mf = _handle(d, *data)
    try:
        trips = [mf.bpr_sample_triplets(N, SEED, ep, BASE) for ep in (1, 2)]
        L.gorse_hip_test_set_bpr_folder_timeout(1)  # the folders make their last pass at once and leave
        mf.bpr_epoch(N, LR, 0.0, SEED, 1, BASE, mode=mode)
        L.gorse_hip_test_set_bpr_folder_timeout(0)
        assert _tier_stats(mf)[:2] == [1, 1] and _tier_stats(mf)[5] == 1
        n_acc = _tier_stats(mf)[4]
        rows = np.zeros(n_acc * d, np.float32)
        capi.check(L.gorse_hip_test_bpr_acc_state(mf.h, None, rows.ctypes.data))
        print("d %d mode %d: non-zero accumulator elements left by the first launch: %d of %d" % (d, mode, int((rows != 0).sum()), rows.size))
        mf.bpr_epoch(N, LR, 0.0, SEED, 2, BASE, mode=mode)
        _check_exact(mf, d, _start(d), trips, "leftovers, mode %d" % mode)
    finally:
        L.gorse_hip_test_set_bpr_folder_timeout(0)
        mf.close()


@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("launch", ["per_sample_on_the_tier_handle", "user_runs_without_the_tier"])
def test_the_other_launches_keep_the_atomic_fold(data, d, launch):
    L = capi.lib()
    per_sample = launch == "per_sample_on_the_tier_handle"
    mf = _handle(d, *data, tier=1 if per_sample else 0)
    L.gorse_hip_test_set_variant(VARIANT_PER_SAMPLE if per_sample else 0)
    try:
        assert mf.bpr_user_runs() == (not per_sample)
        assert (_tier_stats(mf)[4] > 0) == per_sample and _tier_stats(mf)[2] > 0
        trips = [mf.bpr_sample_triplets(N, SEED, ep, BASE) for ep in (1, 2)]
        for ep in (1, 2):
            mf.bpr_epoch_enqueue(N, LR, 0.0, SEED, ep, BASE, mode=capi.BPR_HOGWILD_ATOMIC)
        mf.synchronize()
        assert _tier_stats(mf)[5] == 0
        _check_exact(mf, d, _start(d), trips, launch)
    finally:
        L.gorse_hip_test_set_variant(0)
        mf.close()
