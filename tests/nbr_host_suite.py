"""Shared by test_nbr_cpu.py (exact CPU searchers built on the oracle) and test_gpu_nbr_host.py (hip://): the reference's known
answers for recommendItemToItem / recommendUserToUser (tests/golden/neighbour_recommend_kats.json), random worlds for the embedding,
tags and auto kinds, and the restatement of the per-user host calls on top of tests/nbr_ref.py."""
import json
import os

import numpy as np

import nbr_ref as R
from gorse_amd import vectors as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TS = 1_790_000_000_000


def cpu_db(oracle):
    """a vectors.Database whose device searches are the oracle's exact ones (as tests/test_vectors_db_cpu.py builds it)"""
    from oracle import oracle as orc
    oracle.set_isa(orc.ISA_AVX512)

    def searcher(X, n, d, metric, Q, nq, k, idx, dist, cnt):
        Xa = np.ctypeslib.as_array(X, (n, d)).copy()
        Qa = np.ctypeslib.as_array(Q, (nq, d)).copy()
        I, D, Cn = np.ctypeslib.as_array(idx, (nq, k)), np.ctypeslib.as_array(dist, (nq, k)), np.ctypeslib.as_array(cnt, (nq,))
        for t in range(nq):
            ei, ed = oracle.search_vector(Xa, metric, Qa[t], k)
            I[t, :ei.size], D[t, :ei.size], Cn[t] = ei, ed, ei.size
        return 0

    def sparse_searcher(n, indptr, indices, values, admissible, nq, q_indptr, q_indices, q_values, k, idx, score, cnt):
        ptr = np.ctypeslib.as_array(indptr, (n + 1,)).copy()
        nnz = int(ptr[-1])
        ind = np.ctypeslib.as_array(indices, (max(nnz, 1),))[:nnz].copy()
        val = np.ctypeslib.as_array(values, (max(nnz, 1),))[:nnz].copy()
        ok = np.ctypeslib.as_array(admissible, (n,)).copy()
        qp = np.ctypeslib.as_array(q_indptr, (nq + 1,)).copy()
        qn = int(qp[-1])
        qi = np.ctypeslib.as_array(q_indices, (max(qn, 1),))[:qn].copy()
        qv = np.ctypeslib.as_array(q_values, (max(qn, 1),))[:qn].copy()
        I, Sc, Cn = np.ctypeslib.as_array(idx, (nq, k)), np.ctypeslib.as_array(score, (nq, k)), np.ctypeslib.as_array(cnt, (nq,))
        for t in range(nq):
            ei, es = oracle.sparse_search(ptr, ind, val, qi[qp[t]:qp[t + 1]], qv[qp[t]:qp[t + 1]], k, admissible=ok)
            I[t, :ei.size], Sc[t, :ei.size], Cn[t] = ei, es, ei.size
        return 0
    return V.Database(searcher=searcher, sparse_searcher=sparse_searcher)


# ---- the restatement: raw neighbour lists (item_to_item.go:64-87 without its arithmetic) -> nbr_ref -------------------------------
def raw_lists(db, coll, kind, ids, categories, n):
    out = {}
    for i in ids:
        v = db.GetVectors(coll, [i])
        res = db.QueryVectors(coll, v[0], categories, n + 1) if v else []
        out[i] = [(s.Id, s.Score) for s in res if s.Id != i and (kind == "embedding" or s.Score > 0)][:n]
    return out


def _transform(kind):
    return (R.RECIP, 1.0) if kind == "embedding" else (R.RAW, 0.5 if kind == "auto" else 1.0)


def _named(items, got):
    return [(items[j], s) for j, s in got]


def ref_item_to_item(db, coll, kind, positives, exclude, categories, n):
    lists = raw_lists(db, coll, kind, sorted(set(positives)), categories, n)
    items = sorted({i for l in lists.values() for i, _ in l})
    num = {i: j for j, i in enumerate(items)}
    src = sorted(lists)
    hop2 = R.Table([[num[i] for i, _ in lists[s]] for s in src], [[w for _, w in lists[s]] for s in src], *_transform(kind))
    hop1 = R.Table([[src.index(p) for p in positives]])
    return _named(items, R.recommend_one(hop1, hop2, 0, n, [num[e] for e in exclude if e in num]))


def ref_user_to_user(db, coll, kind, user, exclude, feedback, n):
    nbs = [(u, w) for u, w in raw_lists(db, coll, kind, [user], None, n)[user] if u in feedback]
    src = sorted({u for u, _ in nbs})
    items = sorted({i for u in src for i in feedback[u]})
    num = {i: j for j, i in enumerate(items)}
    hop2 = R.Table([[num[i] for i in feedback[u]] for u in src])
    hop1 = R.Table([[src.index(u) for u, _ in nbs]], [[w for _, w in nbs]], *_transform(kind))
    return _named(items, R.recommend_one(hop1, hop2, 0, n, [num[e] for e in exclude if e in num]))


def same(got, want, what=""):
    """a host call's Score list against (id, sum) pairs or another Score list: ids in order, sums in every bit"""
    want = [(s.Id, s.Score) if hasattr(s, "Id") else s for s in want]
    assert [s.Id for s in got] == [i for i, _ in want], (what, [s.Id for s in got], [i for i, _ in want])
    a, b = np.array([s.Score for s in got], np.float64), np.array([s for _, s in want], np.float64)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (what, a.tolist(), b.tolist())


# ---- the reference's known answers ------------------------------------------------------------------------------------------
def kats():
    with open(os.path.join(ROOT, "tests", "golden", "neighbour_recommend_kats.json")) as f:
        return json.load(f)["cases"]


def run_kat(db, case, bulk):
    """builds the case's collection in db (once per db) and returns the recommender's list"""
    coll = (V.UserToUserCollection if case["recommender"] == "user_to_user" else V.ItemToItemCollection)(case["name"])
    if coll not in db.ListCollections():
        db.AddCollection(coll, case["dimension"], V.Euclidean if case["kind"] == "embedding" else V.Dot)
        db.AddVectors(coll, [V.Vector(v["Id"], v.get("Values", ()), v.get("Indices", ()), v.get("IsHidden", False),
                                      v.get("Categories", ()), 0) for v in case["vectors"]])
    n = case["cache_size"]
    if case["recommender"] == "item_to_item":
        if bulk:
            return V.ItemToItemRecommendBulk(db, coll, case["kind"], [case["positives"]], [case["exclude"]], case["categories"], n)[0]
        return V.ItemToItemRecommend(db, coll, case["kind"], case["positives"], case["exclude"], case["categories"], n)
    if bulk:
        return V.UserToUserRecommendBulk(db, coll, case["kind"], [case["user"]], [case["exclude"]], case["feedback"], n)[0]
    return V.UserToUserRecommend(db, coll, case["kind"], case["user"], case["exclude"], case["feedback"], n)


def check_kat(case, scores):
    if "store_keeps" in case:  # the data-store filter of recommend.go:317-345 is the caller's
        assert sorted(s.Id for s in scores) == sorted(case["store_keeps"] + list(case["store_drops"]))
        scores = [s for s in scores if s.Id in case["store_keeps"]]
    if "expect_ids_in_order" in case:
        assert [s.Id for s in scores] == case["expect_ids_in_order"], [s.Id for s in scores]
    if "expect_scores" in case:
        assert [s.Id for s in scores] == [e["Id"] for e in case["expect_scores"]]
        assert all(abs(s.Score - e["Score"]) <= case["delta"] for s, e in zip(scores, case["expect_scores"]))
    if "expect_scores_any_order" in case:  # ElementsMatch: exact equality of the scores
        assert sorted((s.Id, s.Score) for s in scores) == sorted((e["Id"], e["Score"]) for e in case["expect_scores_any_order"])


# ---- random worlds ------------------------------------------------------------------------------------------------------------
def world(db, kind, seed, n=240, n_users=24):
    """a collection of n entities "e000".. of the kind (some hidden, two categories), and n_users users: positives (with repeats
    and an unknown id), exclude sets (reached, unreached and unknown ids), and a feedback map over the entities as users"""
    rng = np.random.default_rng(seed)
    ids = ["e%03d" % i for i in range(n)]
    coll = "nbr_%s_%d" % (kind, seed)
    hidden = rng.random(n) < 0.05
    cats = [["a"] if rng.random() < 0.7 else ["a", "b"] for _ in range(n)]
    if kind == "embedding":
        w = V.EmbeddingItemToItem("x", TS, db, collection=coll)
        X = rng.normal(0, 1, (n, 8)).astype(np.float32)
        for i in range(n):
            w.Add(ids[i], X[i], bool(hidden[i]), cats[i])
    else:
        tags_idf, fb_idf = rng.uniform(0.2, 3.0, 40).astype(np.float32), rng.uniform(0.2, 3.0, 60).astype(np.float32)
        w = V.SparseSimilarity(kind, coll, TS, db, tags_idf=tags_idf, feedback_idf=fb_idf if kind == "auto" else None)
        for i in range(n):
            w.Add(ids[i], tags=rng.choice(40, int(rng.integers(1, 6)), replace=False),
                  feedback=rng.choice(60, int(rng.integers(0, 5)), replace=False) if kind == "auto" else (),
                  is_hidden=bool(hidden[i]), categories=cats[i])
    w.Clean()
    positives, excludes = [], []
    for t in range(n_users):
        p = list(rng.choice(ids, int(rng.choice([0, 1, 3, 12])))) + (["no-such-item"] if t % 5 == 0 else [])
        positives.append(p + p[:1])
        excludes.append(list(rng.choice(ids, min(int(rng.choice([0, 5, 60])), n // 2), replace=False)) + (["other"] if t % 3 == 0 else []) + p[:2])
    feedback = {ids[i]: ["item%02d" % j for j in rng.integers(0, 50, int(rng.integers(0, 30)))] for i in range(n) if i % 7}
    for t in range(n_users):
        if t % 4 == 1:
            excludes[t] = ["item%02d" % j for j in rng.choice(50, 20, replace=False)]
    return coll, ids, positives, excludes, feedback
