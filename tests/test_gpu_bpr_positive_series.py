"""Positive series of the user-run schedule (csrc/bpr_prepare.hip: bpr_group_positives_kernel; csrc/bpr_update_users.hip: POSITIVE SERIES in bpr_update_user_kernel).

The preparation of a chunk puts the samples of a run that share their positive next to each other; the update kernel walks such a
stretch (a series) with the positive's row in registers and sends the summed change as one atomic row update.  Checked here:
  * the prepared chunk still holds exactly the sampled triplets, every positive of a run in ONE stretch, and as many series as
    there are distinct (user, positive) pairs -- the count of positive-side row updates the kernel issues;
  * no update of a series is lost or counted twice (tiny step: the displacement is the sum of the per-sample deltas), on hot and
    warm positives, in both Hogwild modes, at every kernel width, with negatives that meet the series' own positive;
  * a single user's series equals the sequential oracle (P bit for bit: every sample of the series computes from the row the
    sequential code would hold);
  * 30 epochs at the widths where a late hot-row update once diverged (kDefaultFoldPeriod's sweep) stay finite and on the oracle's NDCG.
"""
import numpy as np
import pytest

from gorse_amd import capi, synth
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

VARIANT_USER_RUNS, VARIANT_STABLE_RANK = 128, 1 << 29
GROUP_CAP = 1024  # csrc/bpr_prepare.hip kGroupCap: the longest run the grouping pass orders


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def rel_err(a, b):
    """tests/test_gpu_cf_parity.py rel_err: largest element error relative to max(|reference element|, rms of the reference)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    floor = max(float(np.sqrt(np.mean(b * b))), 1e-12)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), floor)))


def _sorted_triples(u, i, j):
    t = np.stack([u, i, j], axis=1)
    return t[np.lexsort((t[:, 2], t[:, 1], t[:, 0]))]


def _ragged():
    """the ragged set of test_prepared_chunk_holds_the_sampled_triplets: two users of three without feedback, one holding every item"""
    U, I = 60, 40
    lens = np.zeros(U, np.int64)
    lens[::3] = 5
    lens[3] = I
    uptr = np.zeros(U + 1, np.int64)
    np.cumsum(lens, out=uptr[1:])
    rng = np.random.default_rng(3)
    uidx = np.concatenate([rng.permutation(I)[:n] for n in lens if n > 0]).astype(np.int32)
    return U, I, uptr, uidx


def _check_chunk(mf, U, I, n, seed, epoch, base, label):
    off, si, sj = mf.bpr_prepare_chunk(n, seed, epoch, base)
    gu, gi, gj = mf.bpr_sample_triplets(n, seed, epoch, base)
    assert off[0] == 0 and off[U + 1] == n and (np.diff(off) >= 0).all()
    m = int(off[U])
    su = np.repeat(np.arange(U + 1, dtype=np.int32), np.diff(off))[:m]
    si, sj = si[:m], sj[:m]
    ok = sj >= 0
    failed = gu < 0
    assert int(failed.sum()) == int((~ok).sum()) + int(n - m)
    assert (si[~ok] == -1).all()
    assert np.array_equal(_sorted_triples(su[ok], si[ok], sj[ok]), _sorted_triples(gu[~failed], gi[~failed], gj[~failed]))
    # a series: a maximal stretch of consecutive valid samples of one run with the same positive
    first = ok.copy()
    first[1:] &= ~ok[:-1] | (su[1:] != su[:-1]) | (si[1:] != si[:-1])
    series = np.bincount(su[first], minlength=U)
    pairs = np.unique(su[ok].astype(np.int64) * I + si[ok])
    distinct = np.bincount((pairs // I).astype(np.int64), minlength=U)
    within = np.diff(off)[:U] <= GROUP_CAP
    assert within.any()
    # every positive of a run in one stretch <=> the run has as many series as distinct positives
    assert np.array_equal(series[within], distinct[within]), "a positive of a run within the capacity lies in two stretches"
    assert (series >= distinct).all()
    valid = int(ok[within[su]].sum())
    print("%s: n %d, runs within the capacity %d of %d, series %d / valid samples %d = %.4f (distinct (user, positive) pairs %d)"
          % (label, n, int(within.sum()), int((np.diff(off)[:U] > 0).sum()), int(series[within].sum()), valid,
             series[within].sum() / max(valid, 1), int(distinct[within].sum())))
    return within, series, distinct


def test_prepared_chunk_groups_every_positive_of_a_run():
    L = capi.lib()
    data = synth.s_ml1m()
    mf = capi.MF(data.U, data.I, 64, data.uptr, data.uidx)
    assert mf.bpr_user_runs()
    for variant in (0, 1 << 21):  # the binned preparation and the one without bins
        L.gorse_hip_test_set_variant(variant)
        try:
            within, series, distinct = _check_chunk(mf, data.U, data.I, data.n_train, 2024, 3, 1 << 40, "S-ml1m variant %d" % variant)
        finally:
            L.gorse_hip_test_set_variant(0)
        assert within.all()  # the epoch is one chunk of ~165 samples per user: every run is grouped
        assert int(series.sum()) == int(distinct.sum())
        # about half of an epoch's samples repeat a (user, positive) pair of their run: sum_u n_u (1 - exp(-165 / n_u)) / N = 0.49
        assert 0.45 < series.sum() / data.n_train < 0.53
    mf.close()
    U, I, uptr, uidx = _ragged()
    L.gorse_hip_test_set_variant(VARIANT_USER_RUNS)
    try:
        mf = capi.MF(U, I, 16, uptr, uidx)
        for (seed, epoch, base, n) in [(1, 0, 0, 20000), (0xDEADBEEFCAFE, 7, 123456789012, 5000)]:
            _check_chunk(mf, U, I, n, seed, epoch, base, "ragged")
        mf.close()
    finally:
        L.gorse_hip_test_set_variant(0)


# ---- combining -------------------------------------------------------------------------------------------------------------
CU, CI, CLEN = 2000, 4000, 40
HOT, WARM = 0, 3000  # item 0 in every row (hot: replicas); item 3000 in a handful of rows (no replicas)


def _dataset():
    rng = np.random.default_rng(3)
    rows = [{HOT} for _ in range(CU)]
    for k in range(1, 81):
        for u in rng.choice(CU, 70, replace=False):
            rows[u].add(k)
    for r in rows:
        while len(r) < CLEN:
            r.add(int(rng.integers(81, CI)))
    rows[5].add(WARM)
    uidx = np.concatenate([np.sort(np.fromiter(r, np.int32)) for r in rows])
    uptr = np.zeros(CU + 1, np.int64)
    uptr[1:] = np.cumsum([len(r) for r in rows])
    return uptr, uidx


@pytest.fixture(scope="module")
def cdata():
    return _dataset()


def _expected_moves(P, Q, u, i, j, lr):
    """per-row sum of the per-sample deltas computed from the initial state (reg = 0), float64"""
    P64, Q64 = P.astype(np.float64), Q.astype(np.float64)
    diff = np.einsum("nd,nd->n", P64[u], Q64[i] - Q64[j])
    step = lr / (1.0 + np.exp(diff))[:, None] * P64[u]
    move = np.zeros_like(Q64)
    np.add.at(move, i, step)
    np.add.at(move, j, -step)
    return move


def _streams(x, rng):
    """hand-made streams around positive x; every user's samples consecutive (the stable-rank hook keeps that order in the run)"""
    free = np.setdiff1d(np.arange(81, CI), [x, WARM])
    neg = rng.permutation(free)
    y = int(neg[-1])
    out = {}
    for k in (1, 2, 7, 40):  # one user, the positive k times against distinct negatives
        out["k%d" % k] = (np.full(k, 11, np.int32), np.full(k, x, np.int32), neg[:k].astype(np.int32))
    ks = (1, 2, 3, 5, 7, 9)  # several users sharing the positive, a series each
    u = np.concatenate([np.full(k, 100 + 7 * t, np.int32) for t, k in enumerate(ks)])
    out["shared"] = (u, np.full(u.size, x, np.int32), neg[:u.size].astype(np.int32))
    # negatives that meet the run's own positives: j = the positive of the series just walked (twice in a row, and again later), a
    # sample with i == j inside a series, the series' positive as the negative of the sample that follows a foreign positive
    i = np.array([x, x, x, y, y, x, x, x, x, y, x, x], np.int32)
    j = np.array([neg[0], neg[1], neg[2], x, x, neg[3], x, neg[4], neg[5], neg[6], y, neg[7]], np.int32)
    out["own"] = (np.full(i.size, 11, np.int32), i, j)
    return out


@pytest.mark.parametrize("d", [8, 16, 64, 128])
@pytest.mark.parametrize("mode", [capi.BPR_HOGWILD_ATOMIC, capi.BPR_HOGWILD_STORES])
@pytest.mark.parametrize("x", [HOT, WARM])
def test_series_lose_and_double_no_update(cdata, d, mode, x):
    """reg = 0 and a tiny step: every sample sees (almost) the initial state, so each touched row of Q moves by the sum of its
    per-sample deltas.  The bound is 2 %: one lost or doubled update of 40 shows as 2.5 %, of fewer as more.  What the bound has to
    leave room for: the change of the gradient along 40 steps (40 lr |p|^2 / 4 < 0.3 % at d = 128) and the rounding of an fp32 add
    onto a row of |q| ~ 0.03 (half an ulp = 2e-9 against deltas of ~5e-6)."""
    L = capi.lib()
    uptr, uidx = cdata
    mf = capi.MF(CU, CI, d, uptr, uidx)
    rng = np.random.default_rng(1000 * d + 10 * mode + x)
    P = rng.normal(0, 0.3, (CU, d)).astype(np.float32)
    Q = rng.normal(0, 0.03, (CI, d)).astype(np.float32)
    lr = 2e-5
    L.gorse_hip_test_set_variant(VARIANT_USER_RUNS | VARIANT_STABLE_RANK)
    try:
        for name, (u, i, j) in _streams(x, rng).items():
            mf.set_factors(P, Q)
            mf.bpr_apply_triplets(u, i, j, lr, 0.0, mode)
            gQ = mf.get_factors()[1]
            moved = gQ.astype(np.float64) - Q.astype(np.float64)
            expect = _expected_moves(P, Q, u, i, j, lr)
            rows = np.unique(np.concatenate([i, j]))
            worst = 0.0
            for r in rows:
                scale = np.abs(expect[r]).max()
                if scale == 0.0:
                    continue
                worst = max(worst, float(np.abs(moved[r] - expect[r]).max() / scale))
            print("d %d mode %d positive %d stream %s: worst row |moved - expected| / max |expected| = %.2e" % (d, mode, x, name, worst))
            assert worst < 0.02, (name, worst)
            other = np.ones(CI, bool)
            other[rows] = False
            assert np.array_equal(bits(gQ[other]), bits(Q[other]))  # nothing else moved
    finally:
        L.gorse_hip_test_set_variant(0)
        mf.close()


@pytest.mark.parametrize("d", [8, 16, 64, 128])
@pytest.mark.parametrize("mode", [capi.BPR_HOGWILD_ATOMIC, capi.BPR_HOGWILD_STORES])
@pytest.mark.parametrize("x", [HOT, WARM])
def test_single_user_series_equal_the_sequential_oracle(oracle, cdata, d, mode, x):
    """One user, one positive k times against distinct negatives, a realistic step: the first sample computes from the gathered row,
    every later one from the row the group itself has left -- the sequential code's own operands -- so P equals the oracle bit for
    bit; Q[x] receives the summed change in one atomic per kSeriesFlush samples where the oracle rounds after every sample
    (rel_err < 1e-6, the bar of test_bpr_user_runs_equal_the_sequential_result_when_items_are_disjoint)."""
    oracle.set_exp(1)
    L = capi.lib()
    L.gorse_hip_test_set_exact_exp(1)
    uptr, uidx = cdata
    mf = capi.MF(CU, CI, d, uptr, uidx)
    P, Q = synth.init_factors(CU, CI, d, 0.0, 0.1, 9)
    rng = np.random.default_rng(77 * d + mode + x)
    L.gorse_hip_test_set_variant(VARIANT_USER_RUNS | VARIANT_STABLE_RANK)
    try:
        for name, (u, i, j) in _streams(x, rng).items():
            if not name.startswith("k"):
                continue
            mf.set_factors(P, Q)
            mf.bpr_apply_triplets(u, i, j, 0.05, 0.01, mode)
            gP, gQ = mf.get_factors()
            eP, eQ, _ = oracle.bpr_apply_triplets(P, Q, u, i, j, 0.05, 0.01)
            err = rel_err(gQ, eQ)
            print("d %d mode %d positive %d %s: P equal %s, Q rel_err %.2e" % (d, mode, x, name, np.array_equal(bits(gP), bits(eP)), err))
            assert np.array_equal(bits(gP), bits(eP)), name
            assert err < 1e-6, (name, err)
    finally:
        L.gorse_hip_test_set_variant(0)
        mf.close()


# ---- stability -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [8, 16])
def test_thirty_epochs_on_s_ml1m_stay_finite_and_on_the_oracle(oracle, d):
    """S-ml1m, 30 epochs of the production mode, three handles (sampler seeds): factors finite, three-seed-mean NDCG@10 within 0.01 of
    the sequential oracle on the same sampler streams -- the widths and the duration at which the fold-period sweep of
    kDefaultFoldPeriod found a late hot-row update to diverge."""
    oracle.set_exp(0)
    capi.lib().gorse_hip_test_set_exact_exp(0)
    data = synth.s_ml1m()
    lr, reg, epochs = 0.05, 0.01, 30
    P0, Q0 = synth.init_factors(data.U, data.I, d, 0.0, 0.001, 1)
    srt = orc.sort_rows(data.uptr, data.uidx)
    refs, gots = [], []
    for seed in (2024, 7, 99):
        mf = capi.MF(data.U, data.I, d, data.uptr, data.uidx)
        assert mf.bpr_user_runs()
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
