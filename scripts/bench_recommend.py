#!/usr/bin/env python3
"""Recommending every user's 100 best unseen items: gorse_mf_recommend (exclusion on the device, csrc/recommend.hip) against the
over-fetch route it replaces, on the same inputs in the same run.  What is timed, each on its own:
  new       capi.MF.recommend, k = 100, host to host (device_ms = its own event time)
  search    the over-fetch route's device part alone: TopK.search_vector on the item factors with k = 100 + the longest training row
            of the batch, host to host (the call returns after its copies: synchronised)
  filter    a numpy stand-in for that route's host filter over the search's result (the first 100 + |row| entries minus the row):
            NOT the product's code, reported only to show the part that is missing from `search`
  bulk / unseen (--compiled, ml1m, the first --compiled-users users)  the product's two worker calls through the hip:// database, both
            compiled C++ with the same string-id plumbing: logics::CollaborativeRecommendBulk (search + std::find filter) and
            logics::CollaborativeRecommendUnseen.  The C entry alone is timed, as a cgo caller meets it: the exclude sets are encoded
            before and the staged result is read out (once, to compare the lists) after the timed repetitions
Every route runs once to warm up, then --reps times, the routes ALTERNATING inside a repetition; median, min and max are reported.
Workloads: ml1m = the S-ml1m shape, nFactors 64, all 6040 users; c3 = one rank's shard (125,000 users, all 200,000 items) of the 1M x 200K x 100M set, nFactors 128, its first 65,536 users
for `new`; the over-fetch route there needs k = 100 + the longest row of a batch (thousands), so it is run on the first
--old-users users only and `new` is run on those same users as well (new_subset): the ratio is taken on equal inputs.
usage: bench_recommend.py [--workloads ml1m,c3] [--reps 5] [--compiled [--compiled-users 1024]] [--out profiles/recommend_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gorse_amd import capi, synth  # noqa: E402

K = 100
PEAK_FP32_VALU = 157.3e12  # MI355X vector fp32 peak, flop/s (256 CUs x 128 lanes x 2 x 2.4 GHz)


def stats(ts):
    return {"median_s": float(np.median(ts)), "min_s": float(np.min(ts)), "max_s": float(np.max(ts)), "reps": len(ts)}


def search_batches(topk, P, uptr, n_users, max_entries=1 << 27):
    """the over-fetch searches: batches sized so that batch x k result entries stay below max_entries"""
    out = []
    b0 = 0
    while b0 < n_users:
        b1 = min(n_users, b0 + 8192)
        while True:
            k = K + int(np.diff(uptr[b0:b1 + 1]).max())
            if (b1 - b0) * k <= max_entries or b1 - b0 == 1:
                break
            b1 = b0 + max(1, (b1 - b0) // 2)
        k = min(k, topk.N)
        idx, _, cnt = topk.search_vector(P[b0:b1], k)
        out.append((b0, b1, idx, cnt))
        b0 = b1
    return out


def host_filter(batches, uptr, uidx, n_users):
    items = np.full((n_users, K), -1, np.int32)
    for b0, b1, idx, cnt in batches:
        for t in range(b0, b1):
            row = uidx[uptr[t]:uptr[t + 1]]
            got = idx[t - b0, :min(cnt[t - b0], K + row.size)]
            keep = got[~np.isin(got, row)][:K]
            items[t, :keep.size] = keep
    return items


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def run(name, data, d, n_new, n_old, reps, n_compiled):
    P, Q = synth.init_factors(data.U, data.I, d, 0.0, 0.1, 1)
    uptr, uidx = np.asarray(data.uptr), np.asarray(data.uidx)
    mf = capi.MF(data.U, data.I, d, uptr, uidx)
    mf.set_factors(P, Q)
    ok = np.ones(data.I, np.uint8)  # the over-fetch route searches every stored item
    topk = capi.TopK(Q, capi.METRIC_NEG_DOT)
    routes = {"new": lambda: mf.recommend(n_new, K, ok), "search": lambda: search_batches(topk, P, uptr, n_old)}
    if n_old != n_new:
        routes["new_subset"] = lambda: mf.recommend(n_old, K, ok)
    if n_compiled:
        import ctypes as C
        from gorse_amd import vectors as V
        db = V.Open("hip://")
        coll = V.CollaborativeFilteringCollection(1)
        db.AddCollection(coll, d, V.Dot)
        for s in range(0, data.I, 1024):
            db.AddVectors(coll, [V.Vector(str(i), Q[i]) for i in range(s, min(s + 1024, data.I))])
        H = V._logics_host()
        Pc = np.ascontiguousarray(P[:n_compiled], np.float32)
        ex = "\x1e".join("\n".join(str(i) for i in uidx[uptr[t]:uptr[t + 1]]) for t in range(n_compiled)).encode()
        args = (db.h, coll.encode(), Pc.ctypes.data_as(C.POINTER(C.c_float)), C.c_int64(n_compiled), d, ex, K)

        def read_out():
            flat = V._scores()
            cuts = [int(H.gh_vdb_result_split(t)) for t in range(n_compiled + 1)]
            return [[s.Id for s in flat[cuts[t]:cuts[t + 1]]] for t in range(n_compiled)]
        routes["bulk"] = lambda: V._ck(H.gh_logics_cf_recommend_bulk(*args))
        routes["unseen"] = lambda: V._ck(H.gh_logics_cf_recommend_unseen(*args))
    times = {r: [] for r in routes}
    times["filter"] = []
    dev, split, last = [], None, {}
    for rep in range(reps + 1):  # repetition 0 warms up
        for r, fn in routes.items():
            t, last[r] = timed(fn)
            print("%s rep %d %s %.4f s" % (name, rep, r, t), file=sys.stderr, flush=True)
            if rep:
                times[r].append(t)
            if r == "new" and rep:
                nf, nl, ms = mf.recommend_stats()
                dev.append(ms)
                split = (nf, nl)
        t, last["filter"] = timed(lambda: host_filter(last["search"], uptr, uidx, n_old))
        if rep:
            times["filter"].append(t)
    new_items = (last["new_subset"] if n_old != n_new else last["new"])[0][:n_old]
    res = {"workload": name, "items": int(data.I), "nFactors": d, "k": K, "users_new": n_new, "users_old_route": n_old,
           "routes": {r: stats(ts) for r, ts in times.items()},
           "new_device_ms": stats(np.asarray(dev) * 1e-3), "n_fast": split[0], "n_literal": split[1],
           "rows_equal_new_vs_search_plus_filter": float(np.mean((new_items == last["filter"]).all(axis=1)))}
    med = {r: res["routes"][r]["median_s"] for r in res["routes"]}
    same = med["new_subset"] if n_old != n_new else med["new"]
    res["users_per_s"] = {"new": n_new / med["new"], "search_alone": n_old / med["search"], "search_plus_numpy_filter": n_old / (med["search"] + med["filter"])}
    res["pairs_per_s_new"] = n_new * float(data.I) / med["new"]
    res["ratio_search_alone_over_new_same_users"] = med["search"] / same
    res["end_to_end_fraction_of_fp32_valu_peak"] = 2.0 * d * n_new * float(data.I) / float(np.median(dev) * 1e-3) / PEAK_FP32_VALU
    if n_compiled:
        res["users_compiled"] = n_compiled
        res["users_per_s"]["bulk"] = n_compiled / med["bulk"]
        res["users_per_s"]["unseen"] = n_compiled / med["unseen"]
        res["ratio_bulk_over_unseen"] = med["bulk"] / med["unseen"]
        routes["bulk"]()
        bulk = read_out()
        routes["unseen"]()
        res["rows_equal_unseen_vs_bulk_prefix"] = float(np.mean([a == b[:K] for a, b in zip(read_out(), bulk)]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="ml1m,c3")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--old-users", type=int, default=2048, help="c3: users the over-fetch route is run on")
    ap.add_argument("--compiled", action="store_true", help="ml1m: also the two compiled worker calls through hip://")
    ap.add_argument("--compiled-users", type=int, default=1024, help="ml1m: users the two compiled calls are run on")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recommend_bench.json"))
    a = ap.parse_args()
    res = []
    if os.path.exists(a.out):  # a workload run on its own replaces its own entry
        res = [r for r in json.load(open(a.out)) if "routes" in r]
    for w in a.workloads.split(","):
        if w == "ml1m":
            data = synth.s_ml1m()
            r = run("S-ml1m", data, 64, data.U, data.U, a.reps, min(a.compiled_users, data.U) if a.compiled else 0)
        else:
            data = synth.s_big_shard(0, 8)  # one rank's 125,000 users of the 1M x 200K x 100M set: the same rows, items and widths
            r = run("C3", data, 128, 65536, a.old_users, a.reps, 0)
        res = [x for x in res if x["workload"] != r["workload"]] + [r]
        print(json.dumps(r), flush=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
