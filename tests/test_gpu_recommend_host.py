"""The host mirror above gorse_mf_recommend.  cf::MatrixFactorization::RecommendUnseen on a small fitted BPR returns what
capi.MF.recommend returns on the model's own factors, training rows and predictable flags, mapped through the dictionaries; a model
whose handle holds no training rows demands the seen lists.  logics::CollaborativeRecommendUnseen (what a worker calls: published item
vectors + user embeddings + exclude sets) returns the first cacheSize entries of CollaborativeRecommendBulk's lists."""
import numpy as np
import pytest

from gorse_amd import capi, cf, synth
from gorse_amd import vectors as V

pytestmark = pytest.mark.gpu


def test_recommend_unseen_on_a_fitted_bpr_equals_the_c_abi():
    data = synth.s_ml100k()
    train, test = cf.datasets_from_synth(data)
    m = cf.NewBPR({"NFactors": 16, "NEpochs": 2, "Lr": 0.05, "InitStdDev": 0.01})
    m.Fit(train, test, cf.NewFitConfig().SetVerbose(1).SetJobs(1))
    P, Q = m.factors()
    ok = np.array([m.IsItemPredictable(i) for i in range(data.I)], np.uint8)
    rng = np.random.default_rng(4)
    users = np.concatenate([np.arange(0, data.U, 7), [3, 3]]).astype(np.int32)
    seen = [rng.integers(0, data.I, int(rng.integers(0, 30))).tolist() for _ in users]
    seen[1] = []
    # ids are the decimal indices (cf.datasets_from_synth); one user the model has never heard of
    ids = [str(u) for u in users] + ["nobody"]
    got_i, got_s, got_c = m.RecommendUnseen(ids, 20, seen + [[]])
    assert m.HandleHoldsTrainingRows()
    assert got_c[-1] == 0 and (got_i[-1] == -1).all()
    mf = capi.MF(data.U, data.I, 16, data.uptr, data.uidx)
    mf.set_factors(P, Q)
    users_idx = np.array([u if m.IsUserPredictable(u) else -1 for u in users], np.int32)
    sp = np.zeros(len(users) + 1, np.int64)
    sp[1:] = np.cumsum([len(s) for s in seen])
    si = np.array([i for s in seen for i in s] or [0], np.int32)
    exp_i, exp_s, exp_c = mf.recommend(users_idx, 20, ok, sp, si)
    assert exp_c.max() == 20
    assert np.array_equal(got_c[:-1], exp_c) and np.array_equal(got_i[:-1], exp_i)
    assert np.array_equal(got_s[:-1].view(np.uint32), exp_s.view(np.uint32))
    # the explicit item filter reaches the device too
    only = np.zeros(data.I, np.uint8)
    only[::50] = 1
    a = m.RecommendUnseen(ids[:5], 20, None, only)
    b = mf.recommend(users_idx[:5], 20, only)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and a[2].max() <= only.sum()


def test_recommend_unseen_on_a_recreated_handle_demands_the_seen_lists():
    """a model restored from bare factors (the equivalent of Unmarshal) has no training rows on its handle: without seen lists the call
    refuses, with them (empty ones included) the seen lists are the whole exclusion"""
    rng = np.random.default_rng(6)
    nu, ni, d = 50, 300, 16
    P = rng.standard_normal((nu, d)).astype(np.float32)
    Q = rng.standard_normal((ni, d)).astype(np.float32)
    m = cf.BPR({"NFactors": d})
    m.load_factors(P, Q)
    ids = [str(u) for u in range(nu)]
    with pytest.raises(cf.HostError, match="holds no training rows"):
        m.RecommendUnseen(ids, 10)
    assert not m.HandleHoldsTrainingRows()
    seen = [rng.choice(ni, int(rng.integers(0, 40)), replace=False).tolist() for _ in range(nu)]
    seen[0] = []
    got = m.RecommendUnseen(ids, 10, seen)
    mf = capi.MF(nu, ni, d, np.zeros(nu + 1, np.int64), np.zeros(1, np.int32))  # no training rows either
    mf.set_factors(P, Q)
    sp = np.zeros(nu + 1, np.int64)
    sp[1:] = np.cumsum([len(r) for r in seen])
    exp = mf.recommend(None, 10, np.ones(ni, np.uint8), sp, np.array([i for r in seen for i in r], np.int32))
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[2], exp[2]) and np.array_equal(got[1].view(np.uint32), exp[1].view(np.uint32))
    assert (got[2] == 10).all() and not any(set(got[0][u]) & set(seen[u]) for u in range(nu))
    # nothing seen, said explicitly: the plain top 10 (user 0's row is the same in both calls)
    plain = m.RecommendUnseen(ids, 10, [[] for _ in ids])
    assert np.array_equal(plain[0][0], got[0][0])
    assert any(set(plain[0][u]) & set(seen[u]) for u in range(nu))


def test_collaborative_recommend_unseen_is_the_prefix_of_the_bulk_lists():
    """inputs without ties at the cut: continuous random factors (the assertion on distinct neighbouring scores checks it)"""
    rng = np.random.default_rng(12)
    n_items, n_users, d, cache_size = 700, 90, 24, 10
    Qf = (rng.standard_normal((n_items, d)) * 0.3).astype(np.float32)
    P = (rng.standard_normal((n_users, d)) * 0.3).astype(np.float32)
    db = V.Open("hip://")
    coll = V.CollaborativeFilteringCollection(1790000000001)
    db.AddCollection(coll, d, V.Dot)
    for start in range(0, n_items, 128):
        db.AddVectors(coll, [V.Vector("i%d" % i, Qf[i], IsHidden=(i % 17 == 0), Categories=["c%d" % (i % 3)])
                             for i in range(start, min(start + 128, n_items))])
    # exclude sets from empty to most of the catalogue (more than the 155 that push the bulk search off the MFMA sweep), an id the
    # collection does not hold, the user's own best items among them
    excludes = []
    for u in range(n_users):
        size = [0, 3, 200, 600][u % 4]
        ex = ["i%d" % i for i in rng.choice(n_items, size, replace=False)]
        if u % 4:
            ex += ["i%d" % i for i in np.argsort(-(Qf @ P[u]))[:4]] + ["nobody"]
        excludes.append(ex)
    bulk = V.CollaborativeRecommendBulk(db, coll, P, excludes, cache_size)
    unseen = V.CollaborativeRecommendUnseen(db, coll, P, excludes, cache_size)
    assert len(unseen) == n_users
    for u in range(n_users):
        head = bulk[u][:cache_size + 1]
        assert all(np.float32(a.Score) != np.float32(b.Score) for a, b in zip(head, head[1:])), u  # no tie at or before the cut
        assert [s.Id for s in unseen[u]] == [s.Id for s in bulk[u][:cache_size]], u
        assert [np.float32(s.Score) for s in unseen[u]] == [np.float32(s.Score) for s in bulk[u][:cache_size]]
        assert [s.Categories for s in unseen[u]] == [s.Categories for s in bulk[u][:cache_size]]
        assert len(unseen[u]) == cache_size and not any(s.Id in excludes[u] for s in unseen[u])
        assert all(int(s.Id[1:]) % 17 != 0 for s in unseen[u])  # hidden items never recommended
