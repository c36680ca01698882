#!/usr/bin/env python3
"""A neighbour table from a similarity search, two routes on the same inputs, at two sizes the other benchmarks use:
  sparse   the 200,000 IDF item vectors of the S-big shard (synth.idf_vectors), n = 100, scores <= 0 skipped
  dense    S-emb: 1,000,000 x 128 bf16, cosine, n = 100
  host     (the yardstick) the public search for every stored row as a query, k = n + 1, to the host (sparse:
           gorse_sparse_all_pairs without its self exclusion, dense: gorse_topk_search_vector on the stored vectors, 131,072 rows per
           call); QueryItemToItem's list rule in numpy; gorse_nbr_set_table
  device   gorse_nbr_set_table_from_sparse / _from_topk (csrc/nbr_build.hip): the lists never cross to the host
Each route runs once to warm up, then --reps times, the routes ALTERNATING inside a repetition; median, min and max are reported.  The
two tables are asserted equal in every bit (gorse_nbr_get_table) in every repetition.  search_device_s = the search's own device
time inside the device route (the index's kernel profile), beside which the rest of the route is the rule, the scan, the compaction
and the row pointer's download.
NOT measured: how the host route's time divides between the copy down, the numpy pass, gorse_nbr_set_table's validation and the copy up.
usage: bench_nbr_from_search.py [--reps 5] [--sparse-rows 200000] [--dense-rows 1000000] [--out profiles/nbr_from_search_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gorse_amd import capi, synth  # noqa: E402

N_LIST = 100
TOPK_CLASSES = 6  # GORSE_PROF_TOPK_NCLASSES


def stats(ts):
    return {"median_s": float(np.median(ts)), "min_s": float(np.min(ts)), "max_s": float(np.max(ts)), "reps": len(ts)}


def rule_numpy(idx, raw, cnt, first_row, n, positive_only):
    """the list rule for the lists of stored rows first_row .. : skip the row itself, skip raw <= 0, stop after n -> (counts, indices, weights)"""
    pos = np.arange(idx.shape[1], dtype=np.int32)[None, :]
    keep = (pos < cnt[:, None]) & (idx != (first_row + np.arange(idx.shape[0], dtype=np.int32))[:, None])
    if positive_only:
        keep &= ~(raw <= 0)
    keep &= np.cumsum(keep, axis=1, dtype=np.int16) <= n
    return keep.sum(axis=1), idx[keep], raw[keep]


def host_table(h, search, N, negate, positive_only, transform, step=1 << 17):
    counts, ix, w = [], [], []
    for r0 in range(0, N, step):
        idx, val, cnt = search(r0, min(N, r0 + step))
        c, i, x = rule_numpy(idx, -val if negate else val, cnt, r0, N_LIST, positive_only)
        counts.append(c), ix.append(i), w.append(x)
    ptr = np.zeros(N + 1, np.int64)
    ptr[1:] = np.cumsum(np.concatenate(counts))
    h.set_table(capi.NBR_HOP2, ptr, np.concatenate(ix), np.concatenate(w), transform, 1.0)


def same_tables(a, b):
    return all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a.get_table(capi.NBR_HOP2), b.get_table(capi.NBR_HOP2)))


def run(name, N, host_route, device_route, search_ms, reps):
    dev, host = capi.NbrRecommender(N), capi.NbrRecommender(N)
    times = {"host": [], "device": []}
    search_s = []
    for rep in range(reps + 1):  # repetition 0 warms up
        for route, fn, h in (("host", host_route, host), ("device", device_route, dev)):
            before = search_ms() if route == "device" else 0.0
            t0 = time.perf_counter()
            fn(h)
            t = time.perf_counter() - t0
            print("%s rep %d %s %.4f s" % (name, rep, route, t), file=sys.stderr, flush=True)
            if rep:
                times[route].append(t)
                if route == "device":
                    search_s.append((search_ms() - before) * 1e-3)
        assert same_tables(dev, host), "the two routes' tables differ"
    rows, nnz, _ = dev.table_info(capi.NBR_HOP2)
    med = {r: float(np.median(ts)) for r, ts in times.items()}
    dev.close()
    host.close()
    return {"rows": rows, "n": N_LIST, "entries": nnz, "host": stats(times["host"]), "device": stats(times["device"]),
            "search_device_s": stats(search_s), "tables_equal": True, "ratio_host_over_device": med["host"] / med["device"]}


def sparse_case(n_rows, reps):
    data = synth.s_big_shard(rank=0, world=8)
    ptr, idx, val = synth.idf_vectors(data.iptr, data.iidx, data.U)
    ptr, idx, val = ptr[:n_rows + 1], idx[:ptr[n_rows]], val[:ptr[n_rows]]
    N = ptr.size - 1
    index = capi.Sparse(ptr, idx, val)
    index.set_profiling(True)

    def search(r0, r1):  # the stored rows r0 .. r1 as queries, the row itself not excluded: no query is uploaded
        return index.all_pairs(N_LIST + 1, r0, r1, exclude_self=False)
    res = run("sparse", N, lambda h: host_table(h, search, N, False, True, capi.NBR_RAW),
              lambda h: h.set_table_from_sparse(capi.NBR_HOP2, index, N_LIST, positive_only=True), lambda: index.get_profile()[1], reps)
    index.close()
    return res


def dense_case(n_rows, reps):
    Xb, _ = synth.s_emb(n_rows, 128, 44)
    Xb = np.ascontiguousarray(Xb[:n_rows])
    index = capi.TopK(Xb, capi.METRIC_COSINE, capi.DTYPE_BF16)
    index.set_profiling(True)

    def search(r0, r1):
        return index.search_vector(Xb[r0:r1], N_LIST + 1)
    res = run("dense", n_rows, lambda h: host_table(h, search, n_rows, True, False, capi.NBR_RECIP),
              lambda h: h.set_table_from_topk(capi.NBR_HOP2, index, N_LIST, transform=capi.NBR_RECIP),
              lambda: sum(index.get_profile(c)[1] for c in range(TOPK_CLASSES)), reps)
    index.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sparse-rows", type=int, default=200000)
    ap.add_argument("--dense-rows", type=int, default=1000000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nbr_from_search_bench.json"))
    a = ap.parse_args()
    res = {}
    if a.sparse_rows:
        res["sparse"] = sparse_case(a.sparse_rows, a.reps)
        print(json.dumps(res["sparse"]), flush=True)
    if a.dense_rows:
        res["dense_bf16_cosine_128"] = dense_case(a.dense_rows, a.reps)
        print(json.dumps(res["dense_bf16_cosine_128"]), flush=True)
    res["not_measured"] = "how the host route divides between the copy down, the numpy pass, gorse_nbr_set_table's validation and the copy up"
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
