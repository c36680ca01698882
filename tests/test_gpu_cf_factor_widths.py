"""GPU parity tests of the matrix-factorisation paths at the factor widths the rest of the suite never creates.

gorse_mf_create accepts nFactors up to 256; tests/test_gpu_cf_parity.py stops at 128.  Above 128 every kernel is the generic
(LDS-staged) instantiation at its largest footprint, ALS takes als_gram_naive_kernel + the residual sweep with a handful of
staged rows, and none of it is compared with anything there.  WIDE covers the four shapes of a wide row:
129 = eight 16-chunks + a one-element scalar tail, 200 = twelve chunks + the unfused 8-lane tail, 255 = 8-lane tail + a
seven-element scalar tail, 256 = the LDS maximum of every generic kernel.  The module also runs the instantiations and
branches at ordinary widths that the neighbouring tests skip (per-sample Hogwild at 8 / 32 / 7, Rank with topk past the list
and an empty list, the scalar tails of the item-delta exchange).  Bars are those of tests/test_gpu_cf_parity.py (cf_cases.py)."""
import numpy as np
import pytest

from cf_cases import als_half_fp64, assert_als_close, bits, make_mf, rel_err, report_elementwise
from gorse_amd import capi, synth
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

WIDE = [129, 200, 255, 256]


@pytest.fixture(scope="module")
def small():
    # every item holds >= 1/2048 of the feedback: all 200 are hot rows (MODE_ATOMIC goes through the replicas and the fold)
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


@pytest.fixture
def als_paths():
    """restores the automatic ALS row-solve choice and the default row plan after a test"""
    yield
    capi.lib().gorse_hip_test_set_als_path(0)
    capi.lib().gorse_hip_test_set_als_plan(0, 0)


# ---- 1. Score and Rank ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", WIDE)
def test_score_bit_exact_at_wide_factors(oracle, small, d):
    """mf_score_kernel<0> with two rows of up to 256 floats staged per group (32 KB of LDS at 256), dot512_lds over 8..16 chunks
    + 8-lane tail + scalar tail: bit-equal to floats.Dot in the reference's AVX512 order; set / get_factors round trip."""
    mf, P, Q = make_mf(small, d)
    rng = np.random.default_rng(1)
    u = rng.integers(0, small.U, 5000).astype(np.int32)
    i = rng.integers(0, small.I, 5000).astype(np.int32)
    u[:3] = -1  # unknown user -> 0
    got = mf.score(u, i)
    exp = oracle.mf_score(P, Q, u, i)
    assert np.array_equal(bits(got), bits(exp))
    assert (got[:3] == 0).all()
    P2, Q2 = mf.get_factors()
    assert np.array_equal(bits(P2), bits(P)) and np.array_equal(bits(Q2), bits(Q))
    mf.close()


@pytest.mark.parametrize("d", [48, 80, 96, 112, 128, 144])
def test_score_bit_exact_at_every_register_chunk_count(oracle, small, d):
    """mf_score_kernel<3 | 5 | 6 | 7> (nFactors 48, 80, 96, 112: the register form for every multiple of 16 up to 128, the widths
    with_factor_chunks sends there besides 16, 32, 64, 128) and either side of the edge: 112 and 128 in registers, 144 = nine
    chunks staged in LDS.  Bit-equal to floats.Dot in the reference's AVX512 order, unknown users and items scoring 0."""
    mf, P, Q = make_mf(small, d)
    rng = np.random.default_rng(2)
    u = rng.integers(0, small.U, 5000).astype(np.int32)
    i = rng.integers(0, small.I, 5000).astype(np.int32)
    u[:3] = -1
    i[3:5] = -1
    got = mf.score(u, i)
    exp = oracle.mf_score(P, Q, u, i)
    assert np.array_equal(bits(got), bits(exp))
    assert (got[:5] == 0).all() and (got[5:] != 0).any()
    mf.close()


@pytest.mark.parametrize("d", [200, 16])
def test_rank_topk_past_the_list_and_an_empty_list(oracle, small, d):
    """mf_rank_kernel where the heap never fills (topk 100 > every candidate list: rank_len = the list's length, the row padded
    with -1) and where a user's list is empty (two equal cand_indptr entries: length 0, all -1), over mf_score_kernel<0> (200)
    and <1> (16); index-exact against cf.Rank / TopKFilter, ties included (scores quantised to multiples of 1/16)."""
    mf, P, Q = make_mf(small, d)
    Pq = np.round(P * 4) / 4
    Qq = np.round(Q * 4) / 4
    mf.set_factors(Pq, Qq)
    users, cptr, cand = small.candidates()
    empty = 3
    lens = np.diff(cptr)
    cand = np.concatenate([cand[:cptr[empty]], cand[cptr[empty + 1]:]])
    lens[empty] = 0
    cptr = np.zeros(users.size + 1, np.int64)
    np.cumsum(lens, out=cptr[1:])
    assert 10 < lens.max() < 100 and cptr[empty] == cptr[empty + 1] and cptr[-1] == cand.size
    for topk in (1, 10, 100):
        got, glen = mf.rank(users, cptr, cand, topk)
        exp, elen = oracle.mf_rank(Pq, Qq, users, cptr, cand, topk)
        assert np.array_equal(glen, elen)
        assert np.array_equal(got, exp)
        assert np.array_equal(glen, np.minimum(lens, topk))
        assert glen[empty] == 0 and (got[empty] == -1).all()
        for t in range(users.size):
            assert (got[t, :glen[t]] >= 0).all() and (got[t, glen[t]:] == -1).all()
    mf.close()


# ---- 2. BPR -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", WIDE)
def test_bpr_sequential_bit_exact_at_wide_factors(oracle, small, d):
    """bpr_update_kernel<0, MODE_EXACT> under the levelled (sequential) schedule, three rows of d floats per group in LDS (48 KB at
    256): same triplet stream, restated exp on both sides, P and Q bit for bit the oracle's."""
    mf, P, Q = make_mf(small, d, std=0.3)
    u, i, j = oracle.bpr_sample(small.U, small.I, small.uptr, small.uidx, 4000, 11, 0)
    oracle.set_exp(1)
    capi.lib().gorse_hip_test_set_exact_exp(1)
    eP, eQ, _ = oracle.bpr_apply_triplets(P, Q, u, i, j, 0.05, 0.01)
    mf.bpr_apply_triplets(u, i, j, 0.05, 0.01, capi.BPR_SEQUENTIAL)
    gP, gQ = mf.get_factors()
    assert np.array_equal(bits(gP), bits(eP))
    assert np.array_equal(bits(gQ), bits(eQ))
    mf.close()


def test_bpr_sequential_epoch_equals_replay_at_wide_factors(oracle, small):
    """gorse_bpr_epoch(mode = sequential) at nFactors 255 (8-lane tail + seven scalar elements): sampler, level schedule and
    bpr_update_kernel<0, MODE_EXACT> with the loss sum == the oracle applied to the stream gorse_bpr_sample_triplets reports."""
    d = 255
    mf, P, Q = make_mf(small, d, std=0.2)
    oracle.set_exp(1)
    capi.lib().gorse_hip_test_set_exact_exp(1)
    n = small.n_train
    u, i, j = mf.bpr_sample_triplets(n, 99, 3)
    loss = mf.bpr_epoch(n, 0.05, 0.01, 99, 3, mode=capi.BPR_SEQUENTIAL, want_loss=True)
    eP, eQ, cost = oracle.bpr_apply_triplets(P, Q, u, i, j, 0.05, 0.01)
    gP, gQ = mf.get_factors()
    assert np.array_equal(bits(gP), bits(eP)) and np.array_equal(bits(gQ), bits(eQ))
    assert abs(loss - cost) < 1e-3 * abs(cost)
    mf.close()


@pytest.mark.parametrize("mode", [capi.BPR_HOGWILD_ATOMIC, capi.BPR_HOGWILD_RACY])
@pytest.mark.parametrize("d", WIDE + [8, 32, 7])
def test_bpr_hogwild_conflict_free_batch_at_skipped_widths(oracle, small, mode, d):
    """bpr_update_kernel<0, MODE_ATOMIC / MODE_RACY> at the wide widths, <2, ...> at 32, and the generic form at 8 (nfull == 0: only
    the 8-lane tail contributes to the dot) and 7 (scalar tail alone).  One batch on pairwise distinct rows: every schedule agrees
    with the sequential oracle.  In MODE_ATOMIC the positive updates land in the hot-row replicas (rows of d floats) and reach Q
    through bpr_fold_kernel striding by d: a replica row or a fold written with another stride moves a row of Q that no sample
    touched, or leaves a touched one short -- hence the untouched rows of Q, not only of P, are compared bit for bit."""
    mf, P, Q = make_mf(small, d, std=0.3)
    rng = np.random.default_rng(5)
    n = 60
    u = rng.permutation(small.U)[:n].astype(np.int32)
    items = rng.permutation(small.I)[:2 * n].astype(np.int32)
    i, j = items[:n], items[n:]
    eP, eQ, _ = oracle.bpr_apply_triplets(P, Q, u, i, j, 0.05, 0.01)
    mf.bpr_apply_triplets(u, i, j, 0.05, 0.01, mode)
    gP, gQ = mf.get_factors()
    assert rel_err(gP, eP) < 2e-5 and rel_err(gQ, eQ) < 2e-5
    mask = np.ones(small.U, bool)
    mask[u] = False
    assert np.array_equal(bits(gP[mask]), bits(P[mask]))
    qmask = np.ones(small.I, bool)
    qmask[items] = False
    assert qmask.sum() == small.I - 2 * n
    assert np.array_equal(bits(gQ[qmask]), bits(Q[qmask]))
    mf.close()


@pytest.mark.parametrize("d", [200, 256])
def test_bpr_atomic_hot_rows_fold_exactly_at_wide_factors(oracle, small, d):
    """MODE_ATOMIC at nFactors 200 / 256: the 40 positive updates of one hot item land in its replica rows (hot_row: base * d) and
    reach Q through the folders / bpr_fold_kernel (element w -> slot w / d, column w % d).  All 40 must be in Q when the call
    returns (sum of the per-sample deltas from the state the call starts from, reg = 0; one lost update is a 2.5 % shortfall), and
    a second call starts from clean replicas.  The second call's deltas are taken from the factors the first one left: a call
    moves every dot product by about lr * grad * (2 |p|^2 + |q_i - q_j|^2), which grows with nFactors, and an exact sequential
    float64 pass over these triplets is already 0.61 % / 1.53 % / 1.73 % away from the INITIAL state's deltas on its second
    call at nFactors 64 / 200 / 256 -- past the 1.2 % bar with nothing lost -- but 0.06 % / 0.07 % / 0.09 % from its own start's."""
    mf, P, Q = make_mf(small, d, std=0.3)
    rng = np.random.default_rng(11)
    items = rng.permutation(small.I)
    u = rng.permutation(small.U)[:40].astype(np.int32)
    i = np.full(40, items[0], np.int32)
    j = items[1:41].astype(np.int32)
    lr = 1e-3

    def deltas(P, Q):
        diff = np.einsum("nd,nd->n", P[u].astype(np.float64), (Q[i] - Q[j]).astype(np.float64))
        grad = 1.0 / (1.0 + np.exp(diff))
        return lr * (grad[:, None] * P[u].astype(np.float64)).sum(axis=0)

    mf.bpr_apply_triplets(u, i, j, lr, 0.0, capi.BPR_HOGWILD_ATOMIC)
    gP, gQ = mf.get_factors()
    expect = deltas(P, Q)
    moved = (gQ[items[0]] - Q[items[0]]).astype(np.float64)
    print("fold d=%d call 1: max |moved - expect| / max |expect| %.2e" % (d, np.abs(moved - expect).max() / np.abs(expect).max()))
    assert np.abs(moved - expect).max() < 1e-2 * np.abs(expect).max()
    mf.bpr_apply_triplets(u, i, j, lr, 0.0, capi.BPR_HOGWILD_ATOMIC)
    gQ2 = mf.get_factors()[1]
    expect2 = deltas(gP, gQ)
    moved2 = (gQ2[items[0]] - gQ[items[0]]).astype(np.float64)
    print("fold d=%d call 2: max |moved - expect| / max |expect| %.2e" % (d, np.abs(moved2 - expect2).max() / np.abs(expect2).max()))
    assert np.abs(moved2 - expect2).max() < 1.2e-2 * np.abs(expect2).max()
    mf.close()


def test_bpr_hogwild_epoch_at_wide_factors(oracle):
    """One Hogwild epoch at nFactors 200 through the two-stream pipeline on the per-sample schedule (user runs need nFactors in
    {8, 16, 32, 64, 128}): bpr_sample_kernel + bpr_update_kernel<0, MODE_ATOMIC> with folders + bpr_fold_kernel.  The ragged
    48 x 32 set with one user who holds every item: its samples are skipped (-1 triplets), its row stays as it was; the rest
    against the oracle's sequential pass over the triplets that exist (lr 1e-4, reg 0: the order matters little next to the move)."""
    U, I, d = 48, 32, 200
    lens = np.full(U, 4, np.int64)
    lens[7] = I
    uptr = np.zeros(U + 1, np.int64)
    np.cumsum(lens, out=uptr[1:])
    rng = np.random.default_rng(5)
    uidx = np.concatenate([rng.permutation(I)[:n] for n in lens]).astype(np.int32)
    P, Q = synth.init_factors(U, I, d, 0.0, 0.1, 2)
    mf = capi.MF(U, I, d, uptr, uidx)
    assert not mf.bpr_user_runs()
    mf.set_factors(P, Q)
    mf.bpr_epoch(3000, 1e-4, 0.0, 9, 1)
    gP, gQ = mf.get_factors()
    assert np.isfinite(gP).all() and np.isfinite(gQ).all()
    assert np.array_equal(bits(gP[7]), bits(P[7]))  # every sample of user 7 was skipped
    gu, gi, gj = mf.bpr_sample_triplets(3000, 9, 1)
    keep = gu >= 0
    assert (gu[keep] != 7).all() and (~keep).sum() > 0
    eP, eQ, _ = oracle.bpr_apply_triplets(P, Q, gu[keep], gi[keep], gj[keep], 1e-4, 0.0)
    assert np.abs(gQ - eQ).max() < 2e-2 * np.abs(eQ - Q).max()
    assert np.abs(gP - eP).max() < 2e-2 * np.abs(eP - P).max()
    mf.close()


# ---- 3. ALS -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", WIDE)
def test_als_epochs_at_wide_factors(oracle, small, d, als_paths):
    """nFactors > 128: run_gram launches als_gram_naive_kernel (a thread per entry of S; als_gram_partial_kernel holds 64 entries per
    thread = 128 x 128 and would leave the rest of S unwritten), run_sweep carves als_sweep_kernel's 64 KB by formula (q_cap = 14
    staged rows at 256: nearly every row reads B from global memory past them).  Two epochs against the oracle."""
    capi.lib().gorse_hip_test_set_als_path(0)
    mf, P, Q = make_mf(small, d, std=0.1)
    eP, eQ = P, Q
    for _ in range(2):
        eP, eQ = oracle.als_epoch(eP, eQ, small.uptr, small.uidx, small.iptr, small.iidx, 0.05, 0.015)
        mf.als_epoch(0.05, 0.015)
    gP, gQ = mf.get_factors()
    assert np.isfinite(gP).all() and np.isfinite(gQ).all()
    scale = max(np.abs(eP).max(), np.abs(eQ).max())
    report_elementwise("ALS d=%d" % d, (("P", gP, eP), ("Q", gQ, eQ)))
    assert np.abs(gP - eP).max() < 1e-4 * scale and np.abs(gQ - eQ).max() < 1e-4 * scale
    assert_als_close(gP, eP, "P")
    assert_als_close(gQ, eQ, "Q")
    mf.close()


@pytest.mark.parametrize("d", WIDE)
def test_als_half_sweep_against_float64_at_wide_factors(oracle, small, d, als_paths):
    """One user half-sweep (als_gram_naive_kernel + als_sweep_kernel), every third row, three answers: float64 (als_half_fp64), the
    oracle's float32 recurrence and the device's.  Both float32 forms meet the ALS bar against float64; their distances from it
    per row scale are printed and carry no bar of their own (nobody has measured one for the residual sweep at these widths).
    Seen on an MI355X (max error / row scale; device median, max | oracle median, max; run with -s to print them):
    129: 2.27e-07, 4.84e-07 | 2.47e-07, 4.68e-07      200: 2.74e-07, 4.61e-07 | 2.87e-07, 4.58e-07
    255: 2.99e-07, 6.28e-07 | 3.24e-07, 5.31e-07      256: 3.23e-07, 4.75e-07 | 3.26e-07, 6.16e-07"""
    capi.lib().gorse_hip_test_set_als_path(0)
    mf, P, Q = make_mf(small, d, std=0.1)
    w, reg = 0.05, 0.015
    mf.als_half_epoch(0, w, reg)
    gP, _ = mf.get_factors()
    assert np.isfinite(gP).all()
    rows = np.arange(0, small.U, 3)
    exact = als_half_fp64(P, Q, small.uptr, small.uidx, small.iptr, w, reg, rows)
    oP = P.copy()
    oracle.als_half_range(oP, Q, small.uptr, small.uidx, small.iptr, w, reg, 0, small.U)
    err_dev = np.abs(gP[rows] - exact).max(axis=1) / np.abs(exact).max(axis=1)
    err_ref = np.abs(oP[rows] - exact).max(axis=1) / np.abs(exact).max(axis=1)
    print("ALS d=%d vs float64, max error / row scale: device median %.2e max %.2e; reference recurrence (oracle) median %.2e max %.2e"
          % (d, np.median(err_dev), err_dev.max(), np.median(err_ref), err_ref.max()))
    assert_als_close(gP[rows], exact, "device vs float64")
    assert_als_close(oP[rows], exact, "oracle vs float64")
    mf.close()


def test_als_rows_without_feedback_at_wide_factors(oracle, als_paths):
    """als_gram_naive_kernel must leave out the rows of the other side that have no feedback (model.go:647-651), and als_sweep_kernel
    still solves a row without feedback to p_f = -b / (w S_ff + reg): nFactors 200, every third user and the last five items
    empty, the automatic path and the forced residual sweep."""
    rng = np.random.default_rng(3)
    U, I, d = 50, 40, 200
    rows = [np.sort(rng.choice(I - 5, rng.integers(0, 6), replace=False)).astype(np.int32) if u % 3 else
            np.zeros(0, np.int32) for u in range(U)]
    uptr = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int64)
    uidx = np.concatenate(rows).astype(np.int32)
    cols = [[] for _ in range(I)]
    for u, r in enumerate(rows):
        for i in r:
            cols[i].append(u)
    iptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int64)
    iidx = np.array([u for c in cols for u in c], np.int32)
    P, Q = synth.init_factors(U, I, d, 0.0, 0.1, 5)
    eP, eQ = oracle.als_epoch(P, Q, uptr, uidx, iptr, iidx, 0.05, 0.015)
    scale = max(np.abs(eP).max(), np.abs(eQ).max())
    for path in (0, 1):
        capi.lib().gorse_hip_test_set_als_path(path)
        mf = capi.MF(U, I, d, uptr, uidx, iptr, iidx)
        mf.set_factors(P, Q)
        mf.als_epoch(0.05, 0.015)
        gP, gQ = mf.get_factors()
        mf.close()
        assert np.isfinite(gP).all() and np.isfinite(gQ).all()
        report_elementwise("ALS d=200, rows without feedback, path %d" % path, (("P", gP, eP), ("Q", gQ, eQ)))
        assert np.abs(gP - eP).max() < 1e-4 * scale and np.abs(gQ - eQ).max() < 1e-4 * scale


def test_als_heavy_rows_at_wide_factors(oracle, als_paths):
    """als_sweep_kernel at nFactors 200 with rows longer than pred_cap = 4096 (pred in the global scratch, one stripe of max_row
    floats per workgroup) next to short ones (pred in LDS), all but the first q_cap = 28 entries of B read from global memory."""
    capi.lib().gorse_hip_test_set_als_path(0)
    data = synth.synth_cf(40, 6000, 60000, seed=9, min_len=3, max_frac=0.9, n_neg=10)
    assert np.diff(data.uptr).max() > 4096 and np.diff(data.uptr).min() < 4096
    mf, P, Q = make_mf(data, 200, std=0.1)
    eP, eQ = oracle.als_epoch(P, Q, data.uptr, data.uidx, data.iptr, data.iidx, 0.05, 0.015)
    mf.als_epoch(0.05, 0.015)
    gP, gQ = mf.get_factors()
    assert np.isfinite(gP).all() and np.isfinite(gQ).all()
    scale = max(np.abs(eP).max(), np.abs(eQ).max())
    report_elementwise("ALS d=200, heavy rows", (("P", gP, eP), ("Q", gQ, eQ)))
    assert np.abs(gP - eP).max() < 1e-4 * scale and np.abs(gQ - eQ).max() < 1e-4 * scale
    assert_als_close(gP, eP, "P")
    assert_als_close(gQ, eQ, "Q")
    mf.close()


def test_als_gram_form_rejects_nfactors_200(small, als_paths):
    """als_check: the forced Gram form (path 2) covers nFactors <= 64 and answers GORSE_ERR_INVALID at 200 without launching
    anything; the automatic choice (als_gram_naive_kernel + als_sweep_kernel) then runs on the same handle."""
    capi.lib().gorse_hip_test_set_als_path(2)
    mf, P, _ = make_mf(small, 200, std=0.1)
    with pytest.raises(capi.GorseHipError) as e:
        mf.als_epoch(0.05, 0.015)
    assert e.value.code == capi.ERR_INVALID
    assert np.array_equal(bits(mf.get_factors()[0]), bits(P))
    capi.lib().gorse_hip_test_set_als_path(0)
    mf.als_epoch(0.05, 0.015)
    gP, gQ = mf.get_factors()
    assert np.isfinite(gP).all() and np.isfinite(gQ).all() and not np.array_equal(bits(gP), bits(P))
    mf.close()


# ---- 4. range edge ----------------------------------------------------------------------------------------------------------
def test_nfactors_range_edge(oracle, small):
    """gorse_mf_create: nFactors 257 is GORSE_ERR_INVALID, 256 (the largest LDS footprint of every generic kernel) is created,
    scored and closed."""
    with pytest.raises(capi.GorseHipError) as e:
        capi.MF(small.U, small.I, 257, small.uptr, small.uidx, small.iptr, small.iidx)
    assert e.value.code == capi.ERR_INVALID
    mf, P, Q = make_mf(small, 256)
    u = np.arange(64, dtype=np.int32) % small.U
    i = np.arange(64, dtype=np.int32)[::-1] % small.I
    assert np.array_equal(bits(mf.score(u, i)), bits(oracle.mf_score(P, Q, u, i)))
    mf.close()


# ---- 6. item-delta exchange tails -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def odd_items():
    return synth.synth_cf(300, 201, 6000, seed=7, min_len=3, n_neg=5)


@pytest.mark.parametrize("misaligned", [False, True])
@pytest.mark.parametrize("d", [129, 10, 7, 32])
def test_item_delta_exchange_tails(odd_items, d, misaligned):
    """delta_export_tail / delta_import_tail: with 201 items, I * d mod 4 is 1 (nFactors 129), 2 (10), 3 (7) and 0 (32: no tail), and
    a caller's buffer that is not 16-byte aligned sends the WHOLE matrix through the tail kernels (n4 = 0).  Every call is one
    IEEE operation per element, so bits are compared: export = Q1 - Q0, import of the doubled buffer = Q0 + 2 delta, and an
    export straight after the import is all zeros (Q_sync <- Q).  The float on either side of the buffer stays as it was."""
    import torch
    data = odd_items
    n = data.I * d
    assert n % 4 == {129: 1, 10: 2, 7: 3, 32: 0}[d]
    mf, P, Q0 = make_mf(data, d, std=0.3)
    mf.item_sync_mark()
    mf.bpr_epoch(data.n_train, 0.05, 0.01, 5, 1)
    _, Q1 = mf.get_factors()
    assert not np.array_equal(bits(Q1), bits(Q0))
    raw = torch.full((n + 2,), 77.0, dtype=torch.float32, device="cuda")
    off = 1 if misaligned else 0
    buf = raw[off:off + n]
    torch.cuda.synchronize()
    assert raw.data_ptr() % 16 == 0 and buf.data_ptr() % 16 == 4 * off
    mf.item_delta_export(buf.data_ptr())
    delta = buf.cpu().numpy().reshape(data.I, d)
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
