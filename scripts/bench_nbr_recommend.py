#!/usr/bin/env python3
"""Item-to-item and user-to-user recommendation lists for many users: gorse_nbr_recommend (csrc/nbr_recommend.hip) at the size of the
sparse item-to-item leg, and the per-user host calls it replaces.  What is timed, each on its own:
  device    capi.NbrRecommender.recommend, k = 100, host to host, on tables set once (device_ms = its own event time), for both
            table shapes:
              item_to_item  hop 1 = the users' positive rows (S-big's log-normal lengths), hop 2 = 100 weighted neighbours per item
              user_to_user  hop 1 = 100 weighted neighbours per user, hop 2 = the users' positive rows
            with each user's own positives as the seen row
  per_user / bulk   the product's two host routes through a hip:// database of --db-items embedding vectors, for the first
            --host-users users: logics::ItemToItemRecommend per user (one search per positive, a std::map per user) and
            logics::ItemToItemRecommendBulk (one bulk search, one gorse_nbr_recommend); the lists are asserted equal.  There is no
            parent-commit device time to compare with: the path is new.
Every route runs once to warm up, then --reps times, the routes ALTERNATING inside a repetition; median, min and max are reported.
gather_bytes_per_s = the bytes of the hop-2 rows a call reads (4 per index + 4 per weight) over the device time: what the walk asks
of the memory system, cache hits included -- not an HBM figure.
NOT measured: which of accumulation, probing and selection holds the device time (that takes a kernel trace with counters, or builds
that leave one stage out), and the share of the global-table queries in it.
usage: bench_nbr_recommend.py [--users 100000] [--reps 5] [--host-users 2048] [--db-items 20000] [--out profiles/nbr_recommend_bench.json]"""
import argparse
import functools
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gorse_amd import capi, synth  # noqa: E402

K = 100
NEIGHBOURS = 100


def stats(ts):
    return {"median_s": float(np.median(ts)), "min_s": float(np.min(ts)), "max_s": float(np.max(ts)), "reps": len(ts)}


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def neighbour_table(rng, n_rows, n_targets):
    """NEIGHBOURS distinct targets per row, similarities in (0, 1) descending as a search returns them"""
    idx = np.empty((n_rows, NEIGHBOURS), np.int32)
    step = 1 << 14
    for r0 in range(0, n_rows, step):  # distinct within a row: a random start and positive steps that add up to less than n_targets
        r1 = min(n_rows, r0 + step)
        base = rng.integers(0, n_targets, (r1 - r0, 1))
        off = np.cumsum(rng.integers(1, max(2, n_targets // (2 * NEIGHBOURS)), (r1 - r0, NEIGHBOURS)), axis=1)
        idx[r0:r1] = (base + off) % n_targets
    w = np.sort(rng.random((n_rows, NEIGHBOURS), dtype=np.float32), axis=1)[:, ::-1]
    ptr = np.arange(n_rows + 1, dtype=np.int64) * NEIGHBOURS
    return ptr, idx.reshape(-1), np.ascontiguousarray(w).reshape(-1)


@functools.lru_cache(maxsize=None)
def shard():
    return synth.s_big_shard(0, 8)  # one rank's 125,000 users of the 1M x 200K x 100M set


def device_routes(n_users, reps):
    data = shard()
    uptr, uidx = np.asarray(data.uptr[:n_users + 1], np.int64), np.asarray(data.uidx[:data.uptr[n_users]], np.int32)
    rng = np.random.default_rng(1)
    lens = np.diff(uptr)
    shapes = {}
    iptr, iidx, iw = neighbour_table(rng, data.I, data.I)
    i2i = capi.NbrRecommender(data.I)
    i2i.set_table(capi.NBR_HOP1, uptr, uidx)
    i2i.set_table(capi.NBR_HOP2, iptr, iidx, iw, capi.NBR_RECIP, 1.0)
    shapes["item_to_item"] = (i2i, int(lens.sum()) * NEIGHBOURS * 8)
    nptr, nidx, nw = neighbour_table(rng, n_users, n_users)
    u2u = capi.NbrRecommender(data.I)
    u2u.set_table(capi.NBR_HOP1, nptr, nidx, nw, capi.NBR_RECIP, 1.0)
    u2u.set_table(capi.NBR_HOP2, uptr, uidx)
    shapes["user_to_user"] = (u2u, int(lens[nidx].sum()) * 4)
    times = {s: [] for s in shapes}
    dev = {s: [] for s in shapes}
    split, last = {}, {}
    for rep in range(reps + 1):  # repetition 0 warms up
        for s, (h, _) in shapes.items():
            t, out = timed(lambda: h.recommend(n_users, K, uptr, uidx))
            print("device rep %d %s %.4f s" % (rep, s, t), file=sys.stderr, flush=True)
            if rep:
                times[s].append(t)
                nl, ng, ms = h.recommend_stats()
                dev[s].append(ms * 1e-3)
                split[s] = (nl, ng)
                assert all(np.array_equal(a, b) for a, b in zip(out, last[s])), "two calls on the same inputs differ"
            last[s] = out
    res = {"users": n_users, "items": int(data.I), "neighbours": NEIGHBOURS, "k": K, "hop1_entries_positives": int(lens.sum()), "shapes": {}}
    for s, (_, gathered) in shapes.items():
        d = stats(dev[s])
        res["shapes"][s] = {"host_to_host": stats(times[s]), "device": d, "users_per_s": n_users / float(np.median(times[s])),
                            "n_lds": split[s][0], "n_global": split[s][1], "hop2_bytes_gathered": gathered,
                            "gather_bytes_per_s": gathered / d["median_s"],
                            "lists_full": float(np.mean(last[s][2] == K))}
    return res


def host_routes(n_users, n_items, reps):
    from gorse_amd import vectors as V
    data = shard()
    rng = np.random.default_rng(2)
    db = V.Open("hip://")
    coll = V.ItemToItemCollection("bench")
    db.AddCollection(coll, 16, V.Euclidean)
    X = rng.normal(0, 1, (n_items, 16)).astype(np.float32)
    for s in range(0, n_items, 1024):
        db.AddVectors(coll, [V.Vector(str(i), X[i]) for i in range(s, min(s + 1024, n_items))])
    positives = [[str(int(i) % n_items) for i in data.uidx[data.uptr[t]:data.uptr[t + 1]]] for t in range(n_users)]
    routes = {"bulk": lambda: V.ItemToItemRecommendBulk(db, coll, "embedding", positives, positives, None, K),
              "per_user": lambda: [V.ItemToItemRecommend(db, coll, "embedding", positives[t], positives[t], None, K) for t in range(n_users)]}
    times, last = {r: [] for r in routes}, {}
    for rep in range(reps + 1):
        for r, fn in routes.items():
            t, last[r] = timed(fn)
            print("host rep %d %s %.4f s" % (rep, r, t), file=sys.stderr, flush=True)
            if rep:
                times[r].append(t)
    key = lambda lists: [[(s.Id, np.float64(s.Score).view(np.uint64)) for s in l] for l in lists]  # noqa: E731
    assert key(last["bulk"]) == key(last["per_user"]), "the bulk lists differ from the per-user lists"
    med = {r: float(np.median(ts)) for r, ts in times.items()}
    return {"users": n_users, "db_items": n_items, "k": K, "positives": int(sum(map(len, positives))),
            "routes": {r: stats(ts) for r, ts in times.items()}, "lists_equal": True,
            "users_per_s": {r: n_users / med[r] for r in med}, "ratio_per_user_over_bulk": med["per_user"] / med["bulk"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-users", type=int, default=2048, help="users the per-user host route is run on (0: skip)")
    ap.add_argument("--db-items", type=int, default=20000, help="vectors of the database the host routes search")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nbr_recommend_bench.json"))
    a = ap.parse_args()
    res = {"device": device_routes(a.users, a.reps)}
    print(json.dumps(res["device"]), flush=True)
    if a.host_users:
        res["host"] = host_routes(a.host_users, a.db_items, a.reps)
        print(json.dumps(res["host"]), flush=True)
    res["not_measured"] = "which of accumulation, probing and selection holds the device time; the global-table queries' share of it"
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
