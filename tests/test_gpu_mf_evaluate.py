"""gorse_mf_evaluate / gorse_mf_evaluate_resident (csrc/mf_eval.hip): cf.Evaluate's rank lists, six metrics and user-order sums on
the device.  The yardsticks are the route that was there before -- Mf.rank / rank_resident for the lists, the host mirror's metric
functions (cf.metric) per user, cf.Evaluate under SetHostEvaluate(True) for the result -- and a numpy restatement of the float32
user-order chain.  Everything is compared bit for bit (NaN by NaN-ness)."""
import functools
import re

import numpy as np
import pytest

from gorse_amd import capi, cf, synth

pytestmark = pytest.mark.gpu
CAP = capi.MF_EVAL_MAX_TOPK
SLICE = 64  # candidates the kernel scores between two visits of the heap (mf_eval.hip kSlice)
TOPKS = (1, 3, 10, CAP)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same(got, exp, what=""):
    got, exp = np.asarray(got, np.float32), np.asarray(exp, np.float32)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    nan = np.isnan(exp)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN pattern", got, exp)
    assert np.array_equal(bits(got)[~nan], bits(exp)[~nan]), (what, got, exp)


def host_per_user(target_rows, rank, rlen):
    """6 x n: the host mirror's metric functions on each user's target row and rank list; a user without targets: zeros"""
    out = np.zeros((6, len(target_rows)), np.float32)
    for t, row in enumerate(target_rows):
        if len(row):
            for mid in range(6):
                out[mid, t] = cf.metric(mid, row, rank[t, :rlen[t]])
    return out


def chain(per_user):
    """the float32 running sum of every metric over the users, user after user (np.cumsum adds in order)"""
    if per_user.shape[1] == 0:
        return np.zeros(6, np.float32)
    return np.cumsum(per_user, axis=1, dtype=np.float32)[:, -1]


def csr(rows):
    ptr = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=ptr[1:])
    flat = np.concatenate([np.asarray(r, np.int32) for r in rows] + [np.zeros(0, np.int32)]).astype(np.int32)
    return ptr, flat


def handle(U, I, d, P, Q):
    mf = capi.MF(U, I, d, np.arange(U + 1, dtype=np.int64), (np.arange(U) % I).astype(np.int32))
    mf.set_factors(P, Q)
    return mf


# ---- the general entry: every list length against every topK and the slice, every target-row shape ----------------------------
N_ITEMS = 700
LENGTHS = (0, 1, 2, 3, 4, 9, 10, 11, SLICE - 1, SLICE, SLICE + 1, CAP - 1, CAP, CAP + 1, 3 * SLICE + 5, 5 * SLICE)


@functools.lru_cache(None)
def general_lists():
    """(users, target rows, candidate rows): one user per candidate-list length, in three target-row shapes"""
    rng = np.random.default_rng(12)
    users, targets, cands = [], [], []
    for shape in range(3):
        for n in LENGTHS:
            c = rng.permutation(N_ITEMS)[:n].astype(np.int32)
            absent = np.setdiff1d(np.arange(N_ITEMS, dtype=np.int32), c)
            if shape == 0:    # a few targets, all among the candidates (when there are any), one absent
                t = np.concatenate([c[:min(n, 2)], absent[:1]])
            elif shape == 1:  # duplicates: the denominators count distinct items
                t = np.concatenate([c[:min(n, 3)], c[:min(n, 3)], absent[:2], absent[:1]])
            else:             # more targets than any topK: IDCG is capped by the list's length; most of them absent
                t = np.concatenate([c[::2], absent[:CAP + 12], c[:1]])
            users.append(len(users) % 37)
            targets.append(rng.permutation(t).astype(np.int32))
            cands.append(c)
    # a user with an empty target row between two counted ones, and a counted user with an empty candidate list (LENGTHS[0])
    users.insert(5, 3)
    targets.insert(5, np.zeros(0, np.int32))
    cands.insert(5, rng.permutation(N_ITEMS)[:20].astype(np.int32))
    return np.asarray(users, np.int32), targets, cands


# every form of the width dispatch (cf_device.hpp with_factor_chunks): 16 .. 128 in registers, the others staged in LDS
@pytest.mark.parametrize("d", [8, 16, 24, 32, 48, 64, 80, 96, 112, 128, 129, 200])
def test_per_user_metrics_and_sums_equal_the_host_route(d):
    users, targets, cands = general_lists()
    P, Q = synth.init_factors(40, N_ITEMS, d, 0.0, 0.5, 100 + d)
    mf = handle(40, N_ITEMS, d, P, Q)
    tptr, tflat = csr(targets)
    cptr, cflat = csr(cands)
    counted = sum(1 for r in targets if len(r))
    assert counted == len(users) - 1
    for topk in TOPKS:
        rank, rlen = mf.rank(users, cptr, cflat, topk)
        assert rlen.min() == 0 and (rlen < topk).any() and (rlen == topk).any()
        exp = host_per_user(targets, rank, rlen)
        sums, count, per_user = mf.evaluate(users, tptr, tflat, cptr, cflat, topk, per_user=True)
        assert_same(per_user, exp, "d %d topk %d" % (d, topk))
        assert np.isnan(per_user[0]).sum() == 3 and np.isnan(per_user[1]).sum() == 3  # the empty candidate lists: 0 / 0
        assert_same(sums, chain(per_user), "sums, d %d topk %d" % (d, topk))
        assert count == np.float32(counted)
        assert mf.evaluate_stats()[:2] == (counted, int(cptr[-1]))


# ---- the resident entry -----------------------------------------------------------------------------------------------------
def resident_split(U, I, seed, per_user_rows=(0, 1, 2, 3)):
    """a training CSR and a test split whose rows hold 0 .. 3 items, some of them twice"""
    rng = np.random.default_rng(seed)
    train = [rng.permutation(I)[:rng.integers(1, 6)].astype(np.int32) for _ in range(U)]
    test = []
    for u in range(U):
        n = per_user_rows[u % len(per_user_rows)]
        row = np.setdiff1d(rng.permutation(I)[:n + 8], train[u])[:n].astype(np.int32)
        if n >= 2 and u % 3 == 0:
            row = np.concatenate([row, row[:1]])  # a duplicate
        test.append(row)
    return train, test


@pytest.mark.parametrize("d", [16, 129])
def test_resident_lists_ranks_and_metrics(d):
    U, I = 90, 400
    train, test = resident_split(U, I, 5)
    uptr, uidx = csr(train)
    tptr, tidx = csr(test)
    P, Q = synth.init_factors(U, I, d, 0.0, 0.5, 7)
    mf = capi.MF(U, I, d, uptr, uidx)
    mf.set_factors(P, Q)
    last = None
    for n_neg, topks in ((2, (1, 3, 10)), (9, (3, 10)), (SLICE - 2, (10, CAP)), (CAP - 1, (CAP,)), (3 * SLICE, (10, CAP))):
        mf.sample_user_negatives(tptr, tidx, n_neg, seed=3, fetch=False)  # every sampling replaces the lists
        for topk in topks:
            eu, erank, erlen = mf.rank_resident(topk)
            rows = [test[u] for u in eu]
            assert all(len(r) for r in rows) and len(rows) == sum(1 for r in test if len(r))
            sums, count, per_user, rank, rlen = mf.evaluate_resident(topk, per_user=True, ranks=True)
            assert np.array_equal(rlen, erlen) and np.array_equal(rank, erank), (n_neg, topk)
            assert_same(per_user, host_per_user(rows, rank, rlen), "n_neg %d topk %d" % (n_neg, topk))
            assert_same(sums, chain(per_user))
            assert count == np.float32(len(rows))
            only_sums = mf.evaluate_resident(topk)
            assert_same(only_sums[0], sums)
            assert only_sums[1] == count
            if last is not None and topk == 10:
                assert not np.array_equal(bits(per_user), bits(last))  # the result follows the new lists
            if topk == 10:
                last = per_user


def test_ties_fall_as_the_literal_heap_lets_them():
    """small integer factors: many candidates of a user score equal, targets and non-targets tied across the cut"""
    U, I, d = 60, 300, 16
    rng = np.random.default_rng(21)
    P = rng.integers(-1, 2, (U, d)).astype(np.float32)
    Q = rng.integers(-1, 2, (I, d)).astype(np.float32)
    P[:6] = 0  # every candidate of these users scores 0: the whole list is one tie
    train, test = resident_split(U, I, 9, per_user_rows=(1, 2, 3))
    uptr, uidx = csr(train)
    tptr, tidx = csr(test)
    mf = capi.MF(U, I, d, uptr, uidx)
    mf.set_factors(P, Q)
    mf.sample_user_negatives(tptr, tidx, 40, seed=1, fetch=False)
    for topk in (1, 3, 10):
        eu, erank, erlen = mf.rank_resident(topk)
        sums, count, per_user, rank, rlen = mf.evaluate_resident(topk, per_user=True, ranks=True)
        assert np.array_equal(rank, erank) and np.array_equal(rlen, erlen)
        assert_same(per_user, host_per_user([test[u] for u in eu], rank, rlen))
        assert_same(sums, chain(per_user))
    # the general entry: the targets sit in the middle of the candidate list, so a tie across the cut has targets on both sides
    users = np.arange(U, dtype=np.int32)
    cands = [rng.permutation(I)[:30].astype(np.int32) for _ in range(U)]
    targets = [c[10:20:2] for c in cands]
    cptr, cflat = csr(cands)
    tp, tf = csr(targets)
    s = mf.score(np.repeat(users, 30), cflat).reshape(U, 30)
    for topk in (3, 10):
        kth = -np.sort(-s, axis=1)[:, topk - 1:topk + 1]
        assert (kth[:, 0] == kth[:, 1]).sum() > U // 2  # most users have a tie exactly at the cut
        rank, rlen = mf.rank(users, cptr, cflat, topk)
        sums, count, per_user = mf.evaluate(users, tp, tf, cptr, cflat, topk, per_user=True)
        assert_same(per_user, host_per_user(targets, rank, rlen))
        assert_same(sums, chain(per_user))
        hits = per_user[3]
        assert 0 < hits.sum() < U


# ---- sums: long enough for the chains to round -------------------------------------------------------------------------------
@functools.lru_cache(None)
def sums_case():
    data = synth.synth_cf(5000, 400, 60000, seed=31, min_len=3, n_neg=19)
    P, Q = synth.init_factors(data.U, data.I, 8, 0.0, 0.3, 8)
    return data, P, Q


def test_sums_equal_the_user_order_chain_and_the_host_route():
    data, P, Q = sums_case()
    users, cptr, cand = data.candidates()
    assert users.size > 4900 and int(np.diff(cptr).max()) == 20
    targets = [data.test_idx[data.test_ptr[u]:data.test_ptr[u + 1]] for u in users]
    tptr, tflat = csr(targets)
    mf = capi.MF(data.U, data.I, 8, data.uptr, data.uidx)
    mf.set_factors(P, Q)
    sums, count, per_user = mf.evaluate(users, tptr, tflat, cptr, cand, 10, per_user=True)
    exp = chain(per_user)
    assert_same(sums, exp)
    assert count == np.float32(users.size)
    # the chains do round: the exact sum differs from the float32 one for some metric
    assert any(np.float32(per_user[m].astype(np.float64).sum()) != exp[m] for m in (0, 2, 4, 5))
    # either side of a 64-entry load of the chain kernel, twice
    for n in (64 * 3 - 1, 64 * 3, 64 * 3 + 1, 64 * 77 - 1, 64 * 77, 64 * 77 + 1):
        s, c, pu = mf.evaluate(users[:n], tptr[:n + 1], tflat, cptr[:n + 1], cand, 10, per_user=True)
        assert_same(pu, per_user[:, :n])
        assert_same(s, chain(pu), "n %d" % n)
        assert c == np.float32(n)
    # cf.Evaluate: the host route (rank lists down, metrics on the host) and the device route, preloaded negatives
    train, test = cf.datasets_from_synth(data)
    m = cf.NewBPR({"NFactors": 8})
    m.load_factors(P, Q)
    all_six = (cf.NDCG, cf.Precision, cf.Recall, cf.HR, cf.MAP, cf.MRR)
    m.SetHostEvaluate(True)
    host = cf.Evaluate(m, test, train, 10, 19, 1, *all_six)
    m.SetHostEvaluate(False)
    dev = cf.Evaluate(m, test, train, 10, 19, 1, *all_six)
    mine = sums * (np.float32(1) / count)
    assert_same(dev, host)
    assert_same(mine, host)
    # scorers picked and ordered by the caller
    assert_same(cf.Evaluate(m, test, train, 10, 19, 1, cf.MRR, cf.NDCG), host[[5, 0]])


def test_resident_sums_equal_the_host_route_on_a_production_split():
    """no preloaded negatives: the host mirror samples the lists the device samples (seed 0), so cf.Evaluate's host route over its own
    lists and gorse_mf_evaluate_resident over the handle's agree in every bit"""
    data, P, Q = sums_case()
    mf = capi.MF(data.U, data.I, 8, data.uptr, data.uidx)
    mf.set_factors(P, Q)
    mf.sample_user_negatives(data.test_ptr, data.test_idx, 19, seed=0, fetch=False)
    sums, count, per_user = mf.evaluate_resident(10, per_user=True)
    assert_same(sums, chain(per_user))
    train, test = cf.datasets_from_synth(data, preload_negatives=False)
    m = cf.NewBPR({"NFactors": 8})
    m.load_factors(P, Q)
    m.SetHostEvaluate(True)
    host = cf.Evaluate(m, test, train, 10, 19, 1, cf.NDCG, cf.Precision, cf.Recall, cf.HR, cf.MAP, cf.MRR)
    assert_same(sums * (np.float32(1) / count), host)


# ---- residency and errors ----------------------------------------------------------------------------------------------------
def test_residency_and_errors():
    U, I, d = 50, 200, 24
    train, test = resident_split(U, I, 2)
    uptr, uidx = csr(train)
    tptr, tidx = csr(test)
    P, Q = synth.init_factors(U, I, d, 0.0, 0.5, 3)
    mf = capi.MF(U, I, d, uptr, uidx)
    mf.set_factors(P, Q)
    sums, count = np.zeros(6, np.float32), np.zeros(1, np.float32)
    f32p, L = capi._f32p, capi.lib()

    def resident(topk):
        return L.gorse_mf_evaluate_resident(mf.h, topk, capi._p(sums, f32p), capi._p(count, f32p), None, None, None)

    assert resident(10) == capi.ERR_INVALID  # nothing resident, as gorse_mf_rank_resident
    assert b"resident" in L.gorse_hip_last_error()
    mf.sample_user_negatives(tptr, tidx, 12, seed=5, fetch=False)
    assert resident(0) == capi.ERR_INVALID
    assert resident(CAP + 1) == capi.ERR_INVALID
    assert b"GORSE_MF_EVAL_MAX_TOPK" in L.gorse_hip_last_error()
    assert resident(CAP) == capi.OK
    one = np.zeros(1, np.int32)
    ptr = np.array([0, 1], np.int64)
    for topk in (0, CAP + 1):
        with pytest.raises(capi.GorseHipError) as e:
            mf.evaluate(one, ptr, one, ptr, one, topk)
        assert e.value.code == capi.ERR_INVALID
    with pytest.raises(capi.GorseHipError) as e:  # gorse_mf_rank's validation
        mf.evaluate(one, ptr, one, ptr, np.array([I], np.int32), 3)
    assert e.value.code == capi.ERR_RANGE
    # a recommend or a rank between two evaluations changes nothing (they share the stage scratch)
    a = mf.evaluate_resident(10, per_user=True, ranks=True)
    mf.recommend(None, 7)
    b = mf.evaluate_resident(10, per_user=True, ranks=True)
    mf.rank(np.arange(U, dtype=np.int32), np.arange(U + 1, dtype=np.int64) * 4, (np.arange(4 * U) % I).astype(np.int32), 3)
    c = mf.evaluate_resident(10, per_user=True, ranks=True)
    for x in (b, c):
        assert_same(x[0], a[0])
        assert x[1] == a[1]
        assert_same(x[2], a[2])
        assert np.array_equal(x[3], a[3]) and np.array_equal(x[4], a[4])
    # after a second sampling the result follows the new lists
    mf.sample_user_negatives(tptr, tidx, 12, seed=6, fetch=False)
    eu, erank, erlen = mf.rank_resident(10)
    d2 = mf.evaluate_resident(10, per_user=True, ranks=True)
    assert np.array_equal(d2[3], erank) and not np.array_equal(d2[3], a[3])
    assert_same(d2[2], host_per_user([test[u] for u in eu], erank, erlen))
    users, cands, ms = mf.evaluate_stats()
    assert users == eu.size and cands == sum(len(test[u]) + 12 for u in eu) and ms > 0
    assert abs(sum(mf.evaluate_stage_times()) - ms) < 1e-9


# ---- Fit through either route --------------------------------------------------------------------------------------------------
def strip_times(log):
    return re.sub(r"[a-z_]*=[0-9.]+ms", "", log)


@pytest.mark.parametrize("preload", [True, False])
@pytest.mark.parametrize("name", ["als", "bpr"])
def test_fit_gives_the_same_log_and_score_through_either_route(name, preload):
    data = synth.synth_cf(300, 200, 6000, seed=7, min_len=3, n_neg=50)
    runs = []
    for host_route in (True, False):
        train, test = cf.datasets_from_synth(data, preload_negatives=preload)
        m = (cf.NewALS({"NFactors": 8, "Reg": 0.015, "NEpochs": 4, "Alpha": 0.05}) if name == "als" else
             cf.NewBPR({"NFactors": 16, "NEpochs": 4, "Lr": 0.05, "InitStdDev": 0.01}))
        m.SetHostEvaluate(host_route)
        s = m.Fit(train, test, cf.NewFitConfig().SetVerbose(1).SetJobs(1))
        runs.append(((s.NDCG, s.Precision, s.Recall), strip_times(m.log)))
    assert "fit %s 4/4" % name in runs[0][1] and runs[0][1].count("NDCG@10=") == 6
    assert "_time=" not in runs[0][1]
    assert runs[0][0] == runs[1][0]
    assert runs[0][1] == runs[1][1]
    assert runs[0][0][0] > 0
