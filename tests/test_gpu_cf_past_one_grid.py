"""The matrix-factorisation kernels past their grid caps, where their grid-stride loops take a second step.

Every launch of the BPR units (csrc/bpr_prepare.hip, csrc/bpr_update.hip, csrc/bpr_update_users.hip), csrc/mf_rank.hip and csrc/mf.hip caps its grid and walks the rest of its work in a grid-stride loop; the
neighbouring modules pin these kernels per element at every factor width but give none of them more work than one grid holds.  The
strided iteration is where state survives from one item of work to the next -- the LDS rows a group reuses behind a wave barrier, the
"last two samples" history of a user-run group -- and it is what the product's shapes run (S-ml1m: 6040 users, C3: a million).  The
caps are the literals of cf_cases.py (GRID_*), held against the launchers' text by tests/test_mf_grid_caps_cpu.py, whose docstring also
tabulates which test crosses which cap.  Every comparison and bar is the one of the test the case starts from (named in its docstring):
tests/test_gpu_cf_parity.py and tests/test_gpu_cf_factor_widths.py."""
import numpy as np
import pytest

from cf_cases import (GRID_DELTA_FLOATS, GRID_FOLD_ELEMENTS, GRID_RANK_LISTS, GRID_SAMPLES, GRID_SCORE_PAIRS, GRID_SORT_SAMPLES,
                      GRID_USER_RUNS, GRID_USER_RUNS_D8, SCAN_ONE_WORKGROUP, bits, make_mf, rel_err)
from gorse_amd import capi, synth
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

VARIANT_USER_RUNS, VARIANT_STABLE_RANK = 128, 1 << 29
TAIL = 37  # users past one grid of user runs: slots 0 .. 36 take a second run


@pytest.fixture(scope="module")
def small():
    return synth.synth_cf(300, 200, 6000, seed=7, min_len=3, n_neg=50)


@pytest.fixture(autouse=True)
def _reset(oracle):
    oracle.set_isa(orc.ISA_AVX512)
    oracle.set_exp(0)
    capi.lib().gorse_hip_test_set_exact_exp(0)
    yield
    oracle.set_isa(orc.ISA_AVX512)
    oracle.set_exp(0)
    capi.lib().gorse_hip_test_set_exact_exp(0)


def three_of_forty(U, rng):
    """the training CSR that only sets up a handle: three distinct items of the first 40 per user (those 40 are its hot items)"""
    base = rng.integers(0, 40, U)
    uidx = ((base[:, None] + np.array([0, 13, 27])) % 40).astype(np.int32).reshape(-1)
    return np.arange(0, 3 * U + 1, 3, dtype=np.int64), uidx


# ---- 1. / 2. user runs past one grid ------------------------------------------------------------------------------------------
# group slots g < TAIL of a grid of S runs, by which of user g (first step of the stride) and user g + S (second step) own a run
BOTH = np.array([0, 1, 2, 3, 15, 16, 17, 20, 21, 36])  # (0, 1), (2, 3), (16, 17), (20, 21): the two halves of a group at nFactors 8
ONLY_SECOND = np.array([4, 5, 9, 22, 30, 35])          # the first step takes the empty run's `continue`
ONLY_FIRST = np.array([6, 7, 10, 14, 23, 31])          # (10 without 11, 23 without 22: half a group idle at nFactors 8)


def run_stream(S, rng):
    """(U, u): U = S + TAIL users and a stream in which ~240 of them own runs of 1 .. 12 samples in shuffled order, with one skipped
    sample (u = -1).  A run's length is 1 + (5 slot + 7 step) mod 12: the two runs of a slot differ by 7, the runs of neighbouring
    slots (the halves of a group at nFactors 8) by 5, in both steps."""
    U = S + TAIL
    far = np.array([37, 38, 255, 256, 4095, 4096, S // 2, S // 2 + 1, S - 2, S - 1])
    more = rng.choice(np.arange(39, S - 2), 190, replace=False)
    users = np.unique(np.concatenate([BOTH, BOTH + S, ONLY_SECOND + S, ONLY_FIRST, far, more]))
    lens = 1 + (5 * (users % S) + 7 * (users // S)) % 12
    u = rng.permutation(np.repeat(users, lens)).astype(np.int32)
    u = np.insert(u, 5, -1).astype(np.int32)
    # the five situations of the stride, stated on the stream itself
    runs = np.bincount(u[u >= 0], minlength=U)
    first, second = runs[:TAIL], runs[S:]
    assert second.size == TAIL and runs.max() <= 12
    both = (first > 0) & (second > 0)
    assert both.sum() == BOTH.size and (first[both] != second[both]).all()
    assert ((first == 0) & (second > 0)).sum() == ONLY_SECOND.size and ((first > 0) & (second == 0)).sum() == ONLY_FIRST.size
    assert ((first == 0) & (second == 0)).any()
    assert all(runs[x] > 0 for x in (0, 15, 16, S - 1, U - 1)) and (u < 0).sum() == 1
    for g in (0, 2, 16, 20):  # halves of one group with unequal runs in both steps
        assert runs[g] != runs[g + 1] and runs[g + S] != runs[g + 1 + S] and min(runs[g], runs[g + 1], runs[g + S], runs[g + 1 + S]) > 0
    return U, u


@pytest.mark.parametrize("d", [16, 32, 64, 128, 8])
def test_bpr_user_runs_past_one_grid_equal_the_sequential_result(oracle, d):
    """bpr_update_user_kernel<NC, false, D8> through bpr_launch_update_users, whose grid holds 256 * 16 workgroups x 16 groups = 65,536
    user runs (131,072 at nFactors 8: a run per half group): U = cap + 37, so groups 0 .. 36 walk a SECOND user (cap + slot) with the
    history (im1 .. jm2), the series state and the registers the first run left.  The recipe and the assertions of
    test_bpr_user_runs_equal_the_sequential_result_when_items_are_disjoint (tests/test_gpu_cf_parity.py): every item row touched by one
    sample, ranks in stream order, restated exp -- P bit-equal to the sequential oracle, Q within 1e-6, untouched rows of Q and the P
    rows of users without samples bit for bit as they were (a stride that visits a wrong or a repeated user shows there).  Past the
    cap: the runs of users cap + {0, 1, 2, 3, 15, 16, 17, 20, 21, 36} (slot walked in both steps, different lengths) and of cap +
    {4, 5, 9, 22, 30, 35} (first step empty: the `continue` before the stride); slots {6, 7, 10, 14, 23, 31} only in the first.
    U + 2 = 65,575 run counters also take launch_user_sort through the three-kernel exclusive_scan_i32 (more than 32,768)."""
    oracle.set_exp(1)
    L = capi.lib()
    L.gorse_hip_test_set_exact_exp(1)
    rng = np.random.default_rng(d)
    S = GRID_USER_RUNS_D8 if d == 8 else GRID_USER_RUNS
    U, u = run_stream(S, rng)
    assert U + 2 > SCAN_ONE_WORKGROUP
    n = u.size
    I = 2 * n + 40
    uptr, uidx = three_of_forty(U, rng)
    items = np.empty(2 * n, np.int32)
    items[:30] = rng.permutation(40)[:30]  # positives among the handle's hot items, still all distinct
    items[30:] = 40 + rng.permutation(I - 40)[:2 * n - 30]
    i, j = items[:n].copy(), items[n:].copy()
    P, Q = synth.init_factors(U, I, d, 0.0, 0.1, 9)
    mf = capi.MF(U, I, d, uptr, uidx)
    mf.set_factors(P, Q)
    L.gorse_hip_test_set_variant(VARIANT_USER_RUNS | VARIANT_STABLE_RANK)
    try:
        assert mf.bpr_user_runs()
        mf.bpr_apply_triplets(u, i, j, 0.05, 0.01, capi.BPR_HOGWILD_ATOMIC)
    finally:
        L.gorse_hip_test_set_variant(0)
    keep = u >= 0
    eP, eQ, _ = oracle.bpr_apply_triplets(P, Q, u[keep], i[keep], j[keep], 0.05, 0.01)
    gP, gQ = mf.get_factors()
    mf.close()
    assert np.array_equal(bits(gP), bits(eP))
    assert rel_err(gQ, eQ) < 1e-6
    touched = np.zeros(I, bool)
    touched[i[keep]] = True
    touched[j[keep]] = True
    assert np.array_equal(bits(gQ[~touched]), bits(Q[~touched]))  # nothing else moved
    idle = np.ones(U, bool)
    idle[u[keep]] = False
    assert idle.sum() > U - 300 and np.array_equal(bits(gP[idle]), bits(P[idle]))
    assert not np.array_equal(bits(gP[S:]), bits(P[S:]))  # (the second step did write)


@pytest.mark.parametrize("d", [16, 64])
def test_bpr_user_runs_store_route_past_one_grid(oracle, d):
    """bpr_update_user_kernel<NC, true> (NEG_STORE; store mode 1, GORSE_BPR_HOGWILD_STORES) at U = 65,536 + 37: the recipe of
    test_bpr_user_runs_cold_rows_by_store_are_bit_exact with the second step of the stride in it.  A handle of this many users would
    take the accumulated tier and keep no cold item (hot_rows.hpp acc_rows_eligible), so it is created with the tier off; its window
    then makes every item outside the data set cold.
    Disjoint part: every negative's row goes out as one store of fma(t, lr, row) -- bit-equal to the oracle for the runs of the first
    step AND for those of users >= 65,536.
    Shared cold row: for g in {0, 15, 16, 36} user g's LAST sample and user 65,536 + g's FIRST sample have the same cold negative X,
    which nobody else touches (lr 1e-4, reg 0).  Both updates must be in Q[X], within the 2 % of the summed step that the
    three-in-a-row check of that test allows: the group's history (im1 .. jm2) lives across the loop over users, so the second
    update takes the atomic route; one that overwrote the first would leave half the displacement.  (Seen on an MI355X: 0.03 % ..
    0.07 % of the summed step.  A build that resets the history for every run passes as well: a run's first gathers are issued after
    the stores of the run before it, by the same lanes to the same addresses, so its snapshot holds them and a store computed from it
    loses nothing.  The history across runs is spare caution, not something a result depends on; the check pins that both updates
    land, whichever route the second one takes.)"""
    oracle.set_exp(1)
    L = capi.lib()
    L.gorse_hip_test_set_exact_exp(1)
    rng = np.random.default_rng(200 + d)
    S = GRID_USER_RUNS
    U, u = run_stream(S, rng)
    n = u.size
    I = 2 * n + 40
    uptr, uidx = three_of_forty(U, rng)
    items = (40 + rng.permutation(I - 40)).astype(np.int32)  # never among the data set's items: class "cold"
    i, j = items[:n].copy(), items[n:].copy()
    P, Q = synth.init_factors(U, I, d, 0.0, 0.1, 9)
    L.gorse_hip_test_set_bpr_store_mode(1)
    L.gorse_hip_test_set_bpr_acc_rows(0)
    L.gorse_hip_test_set_variant(VARIANT_USER_RUNS | VARIANT_STABLE_RANK)
    try:
        mf = capi.MF(U, I, d, uptr, uidx)
        assert mf.set_bpr_cold_window(1024) >= I - 40
        mf.set_factors(P, Q)
        keep = u >= 0
        eP, eQ, _ = oracle.bpr_apply_triplets(P, Q, u[keep], i[keep], j[keep], 0.05, 0.01)
        mf.bpr_apply_triplets(u, i, j, 0.05, 0.01, capi.BPR_HOGWILD_STORES)
        gP, gQ = mf.get_factors()
        assert np.array_equal(bits(gP), bits(eP))
        for step in (u[keep] < S, u[keep] >= S):
            rows = j[keep][step]
            assert rows.size > 40 and np.array_equal(bits(gQ[rows]), bits(eQ[rows]))
        assert rel_err(gQ, eQ) < 1e-6
        touched = np.zeros(I, bool)
        touched[i[keep]] = True
        touched[j[keep]] = True
        assert np.array_equal(bits(gQ[~touched]), bits(Q[~touched]))
        # the shared cold rows: runs of three samples, X last in user g's and first in user S + g's
        mf.set_factors(P, Q)
        gs = np.array([0, 15, 16, 36])
        k = gs.size
        X, pos, other = items[:k], items[k:3 * k].reshape(2, k), items[3 * k:11 * k].reshape(2, 2, 2, k)  # other[step, sample, i / j]
        u2 = np.concatenate([np.repeat(gs, 3), np.repeat(gs + S, 3)]).astype(np.int32)
        i2 = np.concatenate([np.stack([other[0, 0, 0], other[0, 1, 0], pos[0]], 1).reshape(-1),
                             np.stack([pos[1], other[1, 0, 0], other[1, 1, 0]], 1).reshape(-1)]).astype(np.int32)
        j2 = np.concatenate([np.stack([other[0, 0, 1], other[0, 1, 1], X], 1).reshape(-1),
                             np.stack([X, other[1, 0, 1], other[1, 1, 1]], 1).reshape(-1)]).astype(np.int32)
        assert (j2[2:3 * k:3] == X).all() and (j2[3 * k::3] == X).all() and (np.bincount(j2, minlength=I)[X] == 2).all()
        lr = 1e-4
        mf.bpr_apply_triplets(u2, i2, j2, lr, 0.0, capi.BPR_HOGWILD_STORES)
        _, gQ2 = mf.get_factors()
        mf.close()
        P64, Q64 = P.astype(np.float64), Q.astype(np.float64)
        steps = []
        for step, users in enumerate((gs, gs + S)):
            diff = np.einsum("kd,kd->k", P64[users], Q64[pos[step]] - Q64[X])
            steps.append(lr / (1.0 + np.exp(diff))[:, None] * P64[users])
            moved = (gQ2[pos[step]] - Q[pos[step]]).astype(np.float64)
            assert (np.abs(moved - steps[step]).max(axis=1) < 0.02 * np.abs(steps[step]).max(axis=1)).all()
        total = steps[0] + steps[1]
        moved = (gQ2[X] - Q[X]).astype(np.float64)
        short = np.abs(moved + total).max(axis=1) / np.abs(total).max(axis=1)
        print("shared cold rows d=%d: max |moved + both steps| / max |both steps| per row %s" % (d, short))
        assert (short < 0.02).all()
    finally:
        L.gorse_hip_test_set_variant(0)
        L.gorse_hip_test_set_bpr_acc_rows(-1)
        L.gorse_hip_test_set_bpr_store_mode(-1)


def test_bpr_user_sort_past_one_grid(oracle):
    """launch_user_sort without the stable-rank hook -- bpr_rank_kernel and bpr_scatter_by_kernel on 256 * 8 workgroups x 256 threads =
    524,288 samples, striding beyond -- with 524,288 + 300 samples of pairwise distinct users and items (one sample per run: the
    arrival order inside a run cannot matter), then bpr_update_user_kernel<1, false, true> (nFactors 8) over 524,625 users = four full
    grids of 131,072 and a fifth step.  A sample the strided part ranks or scatters wrongly is a missing or a doubled update: compared
    as test_bpr_user_runs_equal_the_sequential_result_when_items_are_disjoint compares.  Three samples are skipped (u = -1: key U,
    behind every run), two of them past the cap."""
    oracle.set_exp(1)
    L = capi.lib()
    L.gorse_hip_test_set_exact_exp(1)
    rng = np.random.default_rng(77)
    n, d = GRID_SORT_SAMPLES + 300, 8
    U, I = n + TAIL, 2 * n + 40
    uptr, uidx = three_of_forty(U, rng)
    u = rng.permutation(U)[:n].astype(np.int32)
    u[[5, n - 200, n - 1]] = -1
    items = (40 + rng.permutation(I - 40)).astype(np.int32)
    items[:30] = rng.permutation(40)[:30]
    i, j = items[:n].copy(), items[n:2 * n].copy()
    assert np.unique(np.concatenate([i, j])).size == 2 * n
    P, Q = synth.init_factors(U, I, d, 0.0, 0.1, 9)
    mf = capi.MF(U, I, d, uptr, uidx)
    mf.set_factors(P, Q)
    assert mf.bpr_user_runs()
    mf.bpr_apply_triplets(u, i, j, 0.05, 0.01, capi.BPR_HOGWILD_ATOMIC)
    keep = u >= 0
    eP, eQ, _ = oracle.bpr_apply_triplets(P, Q, u[keep], i[keep], j[keep], 0.05, 0.01)
    gP, gQ = mf.get_factors()
    mf.close()
    assert np.array_equal(bits(gP), bits(eP))
    assert rel_err(gQ, eQ) < 1e-6
    touched = np.zeros(I, bool)
    touched[i[keep]] = True
    touched[j[keep]] = True
    assert (~touched).sum() == 40 + 6 and np.array_equal(bits(gQ[~touched]), bits(Q[~touched]))
    idle = np.ones(U, bool)
    idle[u[keep]] = False
    assert idle.sum() == TAIL + 3 and np.array_equal(bits(gP[idle]), bits(P[idle]))


# ---- 3. per-sample schedule past one launch grid ------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,d", [(capi.BPR_HOGWILD_RACY, 16), (capi.BPR_HOGWILD_RACY, 24), (capi.BPR_HOGWILD_ATOMIC, 24),
                                    (capi.BPR_HOGWILD_ATOMIC, 48)])
def test_bpr_per_sample_conflict_free_batch_past_one_grid(oracle, mode, d):
    """bpr_update_kernel<1, MODE_RACY> (16: registers), <0, MODE_RACY> and <0, MODE_ATOMIC> (24: the LDS form) and <3, MODE_ATOMIC>
    (48) through launch_update_mode, whose grid holds 256 * 16 workgroups x 16 groups = 65,536 samples: ONE launch of n = 65,536 + 300
    (ensure_trip gives a chunk of at least 4M samples), so groups 0 .. 299 take a second sample -- in the LDS form onto the three rows
    they staged for the first, with a wave barrier between.  The batch of test_bpr_hogwild_conflict_free_batch: users and items
    pairwise distinct, so every schedule agrees with the sequential oracle (rel_err < 2e-5 on P and Q) and untouched rows of P and Q
    keep their bits.  The racy mode is per-sample by its mode; at 24 and 48 the user-run schedule does not serve the width, so the
    per-sample kernel runs although U >= 4096 (bpr_user_runs() says so).  The samples past the cap are the last 300: their users and
    items move only if the stride reaches them."""
    rng = np.random.default_rng(1000 * mode + d)
    n = GRID_SAMPLES + 300
    U, I = n + 64, 2 * n + 104
    uptr, uidx = three_of_forty(U, rng)
    P, Q = synth.init_factors(U, I, d, 0.0, 0.3, 3)
    mf = capi.MF(U, I, d, uptr, uidx)
    mf.set_factors(P, Q)
    assert mf.bpr_user_runs() == (d == 16)
    u = rng.permutation(U)[:n].astype(np.int32)
    items = (40 + rng.permutation(I - 40))[:2 * n].astype(np.int32)
    items[:30] = rng.permutation(40)[:30]  # hot positives: through the replicas and the fold in MODE_ATOMIC
    i, j = items[:n].copy(), items[n:].copy()
    eP, eQ, _ = oracle.bpr_apply_triplets(P, Q, u, i, j, 0.05, 0.01)
    mf.bpr_apply_triplets(u, i, j, 0.05, 0.01, mode)
    gP, gQ = mf.get_factors()
    mf.close()
    assert rel_err(gP, eP) < 2e-5 and rel_err(gQ, eQ) < 2e-5
    mask = np.ones(U, bool)
    mask[u] = False
    assert mask.sum() == 64 and np.array_equal(bits(gP[mask]), bits(P[mask]))
    qmask = np.ones(I, bool)
    qmask[items] = False
    assert qmask.sum() == I - 2 * n and np.array_equal(bits(gQ[qmask]), bits(Q[qmask]))
    assert not np.array_equal(bits(gP[u[GRID_SAMPLES:]]), bits(P[u[GRID_SAMPLES:]]))


def test_bpr_fold_kernel_past_one_grid(oracle):
    """bpr_fold_kernel, which follows every per-sample MODE_ATOMIC launch of a handle with hot rows, on 512 workgroups x 256 threads =
    131,072 row elements: a handle with the most hot items there can be (1024, each with 64 of the 65,536 feedbacks) at nFactors 129
    has 1024 * 129 = 132,096 elements of at least one replica row each, so the elements of the last eight hot slots are the strided
    part.  The batch and bars of test_bpr_hogwild_conflict_free_batch_at_skipped_widths with every hot item the positive of one
    sample: an update that stays in its replica row leaves that row of Q short."""
    d, U, I, n = 129, 1024, 4096, 1024
    k = np.arange(64)
    uidx = ((np.arange(U)[:, None] + 16 * k[None, :]) % 1024).astype(np.int32).reshape(-1)
    uptr = np.arange(0, 64 * U + 1, 64, dtype=np.int64)
    assert (np.bincount(uidx, minlength=I)[:1024] == 64).all() and 1024 * d > GRID_FOLD_ELEMENTS
    rng = np.random.default_rng(13)
    P, Q = synth.init_factors(U, I, d, 0.0, 0.3, 3)
    mf = capi.MF(U, I, d, uptr, uidx)
    mf.set_factors(P, Q)
    assert not mf.bpr_user_runs()
    stats = np.zeros(3, np.int64)
    capi.check(capi.lib().gorse_hip_test_bpr_fold_stats(mf.h, stats.ctypes.data))
    n_hot, rep_rows = int(stats[1]), int(stats[2])
    assert n_hot == 1024 and rep_rows >= n_hot
    u = rng.permutation(U)[:n].astype(np.int32)
    i = rng.permutation(1024).astype(np.int32)
    j = (1024 + rng.permutation(I - 1024)[:n]).astype(np.int32)
    eP, eQ, _ = oracle.bpr_apply_triplets(P, Q, u, i, j, 0.05, 0.01)
    mf.bpr_apply_triplets(u, i, j, 0.05, 0.01, capi.BPR_HOGWILD_ATOMIC)
    gP, gQ = mf.get_factors()
    assert rel_err(gP, eP) < 2e-5 and rel_err(gQ, eQ) < 2e-5
    qmask = np.ones(I, bool)
    qmask[i] = False
    qmask[j] = False
    assert qmask.sum() == I - 2 * n and np.array_equal(bits(gQ[qmask]), bits(Q[qmask]))
    rep = np.full(rep_rows * d, np.nan, np.float32)
    capi.check(capi.lib().gorse_hip_test_bpr_hot_state(mf.h, None, None, rep.ctypes.data))
    assert (rep == 0).all()  # every replica row drained, the last eight slots' too
    # a second call starts from clean replicas (a row the fold did not clear would be added twice)
    mf.bpr_apply_triplets(u[:8], j[:8], i[:8], 0.05, 0.01, capi.BPR_HOGWILD_ATOMIC)
    e2P, e2Q, _ = oracle.bpr_apply_triplets(eP, eQ, u[:8], j[:8], i[:8], 0.05, 0.01)
    g2P, g2Q = mf.get_factors()
    mf.close()
    assert rel_err(g2P, e2P) < 2e-5 and rel_err(g2Q, e2Q) < 2e-5


# ---- 4. score past one grid ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [16, 128, 24, 200])
def test_score_bit_exact_past_one_grid(oracle, small, d):
    """mf_score_kernel<1>, <8> (registers) and <0> (24, 200: two rows per group staged in LDS, reused for the group's next pair behind a
    wave barrier) through mf_score_device, whose grid holds 256 * 32 workgroups x 16 groups = 131,072 pairs: n = 131,072 + 100, so
    groups 0 .. 99 score a second pair.  Bit-equal to floats.Dot in the reference's AVX512 order, as test_score_bit_exact; unknown
    users / items (-1) score 0, among them pairs 131,072 + {3, 50}.  The last 100 pairs are built to differ from the first 100 (the
    pairs the same groups scored first): a walk that wraps round or stays on its first pair shows."""
    mf, P, Q = make_mf(small, d)
    rng = np.random.default_rng(d)
    n = GRID_SCORE_PAIRS + 100
    u = rng.integers(0, small.U, n).astype(np.int32)
    i = rng.integers(0, small.I, n).astype(np.int32)
    u[-100:] = (u[:100] + 1 + rng.integers(0, small.U - 1, 100)) % small.U
    u[:3] = -1
    i[3:5] = -1
    u[GRID_SCORE_PAIRS + 3] = -1
    i[GRID_SCORE_PAIRS + 50] = -1
    got = mf.score(u, i)
    exp = oracle.mf_score(P, Q, u, i)
    mf.close()
    assert (exp[-100:] != exp[:100]).sum() >= 95 and (exp[:5] == 0).all() and exp[GRID_SCORE_PAIRS + 3] == 0
    assert np.array_equal(bits(got), bits(exp))


# ---- 5. rank with more lists than expand_users_kernel's grid -------------------------------------------------------------------------
def test_rank_exact_past_one_grid_of_lists(oracle, small):
    """expand_users_kernel (mf_rank_device: one workgroup per list, at most 4096, striding beyond) with 4096 + 5 lists of 0 .. 3
    candidates, user ids repeating modulo U, empty lists at positions 0, 4095, 4096 and at the last one, topk 2: index-exact against
    cf.Rank / TopKFilter as test_rank_exact (scores quantised to force ties).  A list past the cap whose pairs keep a stale user id
    is ranked by another user's scores.
    The fused route (mf_eval_user_kernel, a group per list, no cap) must agree past the literal route's cap.  gorse_mf_evaluate
    returns no rank lists for lists given by the caller (only the resident entry does), so the ranks are read off its per-user NDCG:
    in pass k every list's only target is its k-th candidate, whose NDCG@2 is 1 at rank 0, 1 / log2(3) at rank 1 and 0 outside the
    list -- three passes state every candidate's rank."""
    d = 16
    mf, P, Q = make_mf(small, d)
    Pq = np.round(P * 4) / 4
    Qq = np.round(Q * 4) / 4
    mf.set_factors(Pq, Qq)
    rng = np.random.default_rng(4)
    n, topk = GRID_RANK_LISTS + 5, 2
    users = (np.arange(n) % small.U).astype(np.int32)
    lens = rng.integers(0, 4, n)
    lens[[0, GRID_RANK_LISTS - 1, GRID_RANK_LISTS, n - 1]] = 0
    lens[[GRID_RANK_LISTS + 1, GRID_RANK_LISTS + 2, GRID_RANK_LISTS + 3]] = (3, 1, 2)
    three = (rng.integers(0, small.I, n)[:, None] + np.array([0, 7, 19])) % small.I  # distinct within a list
    has = np.arange(3)[None, :] < lens[:, None]
    cand = three[has].astype(np.int32)
    cptr = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=cptr[1:])
    got, glen = mf.rank(users, cptr, cand, topk)
    exp, elen = oracle.mf_rank(Pq, Qq, users, cptr, cand, topk)
    assert np.array_equal(glen, elen) and np.array_equal(glen, np.minimum(lens, topk))
    assert np.array_equal(got, exp)
    for k in range(3):
        tlen = (lens > k).astype(np.int64)
        tptr = np.zeros(n + 1, np.int64)
        np.cumsum(tlen, out=tptr[1:])
        target = three[lens > k, k].astype(np.int32)
        _, count, per_user = mf.evaluate(users, tptr, target, cptr, cand, topk, per_user=True)
        assert count == np.float32(tlen.sum())
        ndcg = per_user[0][lens > k]
        assert np.isclose(ndcg[:, None], [0.0, 1.0 / np.log2(3.0), 1.0], rtol=0, atol=1e-6).any(axis=1).all()
        fused = np.where(ndcg > 0.9, 0, np.where(ndcg > 0.0, 1, -1))
        lit = got[lens > k]
        literal = np.where(lit[:, 0] == target, 0, np.where(lit[:, 1] == target, 1, -1))
        assert np.array_equal(fused, literal), k
        assert (per_user[:, lens <= k] == 0).all()
    mf.close()


# ---- 6. item-delta exchange past one grid ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("misaligned", [False, True])
def test_item_delta_exchange_past_one_grid(misaligned):
    """delta_export_kernel / delta_import_kernel on 2048 workgroups x 256 threads, a float4 each = 2,097,152 floats per grid: I = 16,401
    items at nFactors 129 are 2,115,729 floats (I * d mod 4 = 1), so the float4s of items 16,257 .. 16,400 are the strided part and the
    last float goes through delta_export_tail / delta_import_tail; a buffer that is not 16-byte aligned sends the whole matrix through
    the tail kernels (one thread per float, no cap).  The bit comparisons of test_item_delta_exchange_tails: export = Q1 - Q0, import
    of the doubled buffer = Q0 + 2 delta, an export straight after the import is all zeros, the float on either side of the buffer
    stays.  Q moves between the mark and the export by one conflict-free batch whose items include the first, the last and others
    past the cap."""
    import torch
    d, U, I = 129, 300, 16_401
    n = I * d
    assert n == 2_115_729 and n > GRID_DELTA_FLOATS and n % 4 == 1
    rng = np.random.default_rng(21)
    uptr, uidx = three_of_forty(U, rng)
    P, Q0 = synth.init_factors(U, I, d, 0.0, 0.3, 3)
    mf = capi.MF(U, I, d, uptr, uidx)
    mf.set_factors(P, Q0)
    mf.item_sync_mark()
    first_past = GRID_DELTA_FLOATS // d + 1
    items = np.concatenate([[0, I - 1, I - 2, first_past], rng.permutation(np.arange(1, first_past))[:196],
                            rng.permutation(np.arange(first_past + 1, I - 2))[:80]]).astype(np.int32)
    u = rng.permutation(U)[:140].astype(np.int32)
    mf.bpr_apply_triplets(u, items[:140], items[140:], 0.05, 0.01, capi.BPR_HOGWILD_ATOMIC)
    _, Q1 = mf.get_factors()
    moved = (bits(Q1) != bits(Q0)).any(axis=1)
    assert moved[items].all() and moved.sum() == 280 and bits(Q1)[I - 1, d - 1] != bits(Q0)[I - 1, d - 1]
    raw = torch.full((n + 2,), 77.0, dtype=torch.float32, device="cuda")
    off = 1 if misaligned else 0
    buf = raw[off:off + n]
    torch.cuda.synchronize()
    assert raw.data_ptr() % 16 == 0 and buf.data_ptr() % 16 == 4 * off
    mf.item_delta_export(buf.data_ptr())
    delta = buf.cpu().numpy().reshape(I, d)
    assert np.array_equal(bits(delta), bits(Q1 - Q0))
    buf.mul_(2.0)  # pretend a second rank produced the same delta
    torch.cuda.synchronize()
    mf.item_delta_import(buf.data_ptr())
    _, Q2 = mf.get_factors()
    assert np.array_equal(bits(Q2), bits(Q0 + np.float32(2.0) * delta))
    mf.item_delta_export(buf.data_ptr())
    again = buf.cpu().numpy()
    assert not again.any()
    guard = raw.cpu().numpy()
    assert (guard[:off] == 77.0).all() and (guard[off + n:] == 77.0).all()
    mf.close()
