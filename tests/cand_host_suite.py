"""Shared by test_cand_cpu.py (exact CPU searchers built on the oracle) and test_gpu_cand_host.py (hip://): the reference's known
answers for the single list recommenders (tests/golden/recommend_sequential_kats.json), a random world with all four kinds of stage,
and tests/cand_ref.py driven by the per-user host calls on string ids."""
import json
import os

import numpy as np

import cand_ref as R
import nbr_host_suite as S
from gorse_amd import vectors as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kats():
    with open(os.path.join(ROOT, "tests", "golden", "recommend_sequential_kats.json")) as f:
        return json.load(f)["cases"]


def kat_stage(case, query):
    """what the store hands the recommender: the CacheSize best entries that carry the queried category, descending"""
    rows = [s for s in case["scores"] if not query["categories"] or set(query["categories"]) & set(s["Categories"])]
    rows = sorted(rows, key=lambda s: -s["Score"])[:case["cache_size"]]
    lst = [V.Score(s["Id"], s["Score"], s["Categories"]) for s in rows]
    return V.SeqStage(case["recommender"], case["cache_size"], lists=lst if case["recommender"] == "shared" else [lst])


def check_kat(query, scores):
    assert [(s.Id, s.Score) for s in scores] == [(e["Id"], e["Score"]) for e in query["expect"]]


def world(db, seed, n_users=24):
    """an embedding collection, users with positives and exclude sets (nbr_host_suite.world), and four stages: a cached list per
    user, item-to-item, user-to-user over the same collection, and a shared list; ids overlap between all of them"""
    coll, ids, positives, excludes, feedback = S.world(db, "embedding", seed, n=120, n_users=n_users)
    rng = np.random.default_rng(seed + 100)
    pool = ids + ["item%02d" % j for j in range(50)]
    users = [ids[int(i)] for i in rng.choice(len(ids), n_users, replace=False)]

    def scored(n):
        picked = [pool[int(i)] for i in rng.integers(0, len(pool), n)]  # repeats allowed
        return [V.Score(i, float(s), []) for i, s in zip(picked, np.sort(rng.normal(0, 1, n))[::-1])]

    cached = [scored(int(rng.choice([0, 3, 12, 30]))) for _ in range(n_users)]
    stages = [V.SeqStage("lists", 10, lists=cached),
              V.SeqStage("item_to_item", 7, collection=coll, type="embedding", categories=None),
              V.SeqStage("user_to_user", 9, collection=coll, type="embedding", feedback=feedback),
              V.SeqStage("shared", 5, lists=scored(40))]
    return users, positives, excludes, stages


def for_user(stages, t):
    """the stages as the per-user call takes them: a "lists" stage holds user t's list alone"""
    return [V.SeqStage(s.kind, s.cache_size, [s.lists[t]], s.collection, s.type, s.categories, s.feedback) if s.kind == "lists" else s
            for s in stages]


def per_user(db, users, positives, excludes, stages):
    return [V.RecommendSequential(db, users[t], positives[t], excludes[t], for_user(stages, t)) for t in range(len(users))]


def restatement(db, users, positives, excludes, stages):
    """tests/cand_ref.py over one numbering of every id, its neighbourhood lists from the per-user public calls under the
    concatenated exclusion rows; returns one [(id, score bits)] list per user"""
    out_names = {}

    def num(i):
        return out_names.setdefault(i, len(out_names))

    for e in excludes:
        for i in e:
            num(i)
    ref = R.Chain(len(users), [[num(i) for i in e] for e in excludes])
    back = lambda: {v: k for k, v in out_names.items()}  # noqa: E731
    for st in stages:
        if st.kind == "lists":
            lists = [[(num(s.Id), s.Score) for s in l] for l in st.lists]
        elif st.kind == "shared":
            lists = [[(num(s.Id), s.Score) for s in st.lists]] * len(users)
        else:
            names_now = back()
            lists = []
            for t in range(len(users)):
                cur = [names_now[j] for j in ref.cur[t]]
                got = (V.ItemToItemRecommend(db, st.collection, st.type, positives[t], cur, st.categories, st.cache_size)
                       if st.kind == "item_to_item" else
                       V.UserToUserRecommend(db, st.collection, st.type, users[t], cur, st.feedback, st.cache_size))
                lists.append([(num(s.Id), s.Score) for s in got])
        ref.add(lists, st.cache_size)
    names_now = back()
    return [[(names_now[c[0]], c[1]) for c in row] for row in ref.cand]


def same_lists(got, want, what=""):
    """Score lists against [(id, score bits)] or other Score lists"""
    for t, (g, w) in enumerate(zip(got, want)):
        w = [(s.Id, R.bits(s.Score)) if hasattr(s, "Id") else s for s in w]
        assert [(s.Id, R.bits(s.Score)) for s in g] == w, (what, t)
    assert len(got) == len(want)
