#!/usr/bin/env python
"""Times gorse_fm_rank_users against the per-user route it replaces, on the same inputs.

Workload: one handle, nFactors 16, one embedding field of D = 768 and again D = 1536; a catalogue of 100,000 items; 4096 users
with 300 candidates each; batch size 1024; user and item rows of 4 entries (the id entry, lead 1, and three labels).
  new route     one rank_users call with the catalogue resident (set_items is timed separately);
  parent route  per user: materialise the 300 x 8 index / value matrices and gather the 300 x D embedding matrix on the host,
                predict_embeddings, numpy.argsort -- timed with the host materialisation and, from rows prepared beforehand,
                without it.  It runs on the first --parent-users users only (512 by default); the report says so.
Median [min-max] of --reps repetitions after a warm-up, the routes alternating.  The scores of the two routes must be equal in
every bit and the orders identical, or the script fails.  Writes one JSON file."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gorse_amd import capi  # noqa: E402

f32 = np.float32


def to_bf16(x):
    u = np.ascontiguousarray(x, f32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def stat(ts):
    ts = sorted(ts)
    return dict(median_ms=1e3 * ts[len(ts) // 2], min_ms=1e3 * ts[0], max_ms=1e3 * ts[-1])


def run(D, args, rng):
    d, n_items, n_users, n_cand, bs = 16, args.items, args.users, args.candidates, args.batch
    n_labels = 1000
    nf = n_users + n_items + 2 * n_labels
    fm = capi.FM(nf, d, embedding_dims=(D,))
    fm.set_params(f32(0.1), rng.normal(0, 0.1, nf).astype(f32), rng.normal(0, 0.1, (nf, d)).astype(f32))
    b = 1 / np.sqrt(D)
    fm.set_embedding_params(0, rng.normal(0, 0.3, (d, D)).astype(f32), rng.uniform(-b, b, (D, d)).astype(f32),
                            rng.normal(0, 0.1, d).astype(f32), rng.uniform(-b, b, (D, d)).astype(f32),
                            rng.normal(0, 0.1, d).astype(f32))
    # rows: [id, label, label, label], lead 1
    uidx = np.concatenate([np.arange(n_users)[:, None], n_users + n_items + rng.integers(0, n_labels, (n_users, 3))], 1).astype(np.int32)
    iidx = np.concatenate([n_users + np.arange(n_items)[:, None],
                           n_users + n_items + n_labels + rng.integers(0, n_labels, (n_items, 3))], 1).astype(np.int32)
    uval = rng.uniform(0.2, 1.0, uidx.shape).astype(f32)
    ival = rng.uniform(0.2, 1.0, iidx.shape).astype(f32)
    emb = to_bf16(rng.normal(0, 1, (n_items, D)).astype(f32))
    emb[::7] = 0
    cand = rng.integers(0, n_items, (n_users, n_cand)).astype(np.int32)
    uptr, iptr = np.arange(n_users + 1, dtype=np.int64) * 4, np.arange(n_items + 1, dtype=np.int64) * 4
    cptr = np.arange(n_users + 1, dtype=np.int64) * n_cand
    ones_u, ones_i = np.ones(n_users, np.int32), np.ones(n_items, np.int32)

    t0 = time.perf_counter()
    fm.set_items(iptr, iidx, ival, lead=ones_i, embs=[emb])
    t_set = time.perf_counter() - t0

    def new_route():
        return fm.rank_users(uptr, uidx, uval, cptr, cand, bs, user_lead=ones_u)

    def materialise(t):
        c = cand[t]
        it, iv = iidx[c], ival[c]
        ui, uv = np.broadcast_to(uidx[t], (n_cand, 4)), np.broadcast_to(uval[t], (n_cand, 4))
        idx = np.concatenate([ui[:, :1], it[:, :1], ui[:, 1:], it[:, 1:]], 1)
        val = np.concatenate([uv[:, :1], iv[:, :1], uv[:, 1:], iv[:, 1:]], 1)
        return np.ascontiguousarray(idx), np.ascontiguousarray(val), emb[c]

    pu = min(args.parent_users, n_users)

    def parent_route(prepared=None):
        scores, order = np.empty((pu, n_cand), f32), np.empty((pu, n_cand), np.int32)
        for t in range(pu):
            idx, val, e = prepared[t] if prepared is not None else materialise(t)
            scores[t] = fm.predict_embeddings(idx, val, [e], bs)
            order[t] = np.argsort(-scores[t], kind="stable")
        return scores, order

    prepared = [materialise(t) for t in range(pu)]
    new_route()
    parent_route(prepared)
    t_new, t_dev, t_par, t_par_prep = [], [], [], []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        s_new, o_new = new_route()
        t_new.append(time.perf_counter() - t0)
        st = fm.rank_stats()
        t_dev.append(st["device_ms"] * 1e-3)
        t0 = time.perf_counter()
        s_par, o_par = parent_route()
        t_par.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        parent_route(prepared)
        t_par_prep.append(time.perf_counter() - t0)
    head = s_new[:pu * n_cand].reshape(pu, n_cand)
    assert np.array_equal(head.view(np.uint32), s_par.view(np.uint32)), "the two routes' scores differ"
    assert not np.isnan(s_new).any()
    assert np.array_equal(o_new[:pu * n_cand].reshape(pu, n_cand), o_par), "the two routes' orders differ"
    rows = n_users * n_cand
    dev = stat(t_dev)
    # what the three branch launches must move per row: x twice (bf16), s written, read + written, read + written (fp32)
    branch_bytes = rows * (2 * 2 * D + 5 * 4 * D)
    return dict(D=D, d=d, items=n_items, users=n_users, candidates=n_cand, batch_size=bs, rows=rows, stats=st,
                set_items_ms=1e3 * t_set, new_route=stat(t_new), new_route_device=dev,
                new_route_users_per_s=n_users / (stat(t_new)["median_ms"] * 1e-3),
                parent_users=pu, parent_route=stat(t_par), parent_route_prepared_rows=stat(t_par_prep),
                parent_route_users_per_s=pu / (stat(t_par)["median_ms"] * 1e-3),
                parent_route_prepared_users_per_s=pu / (stat(t_par_prep)["median_ms"] * 1e-3),
                device_bytes_per_s_lower_bound=branch_bytes / (dev["median_ms"] * 1e-3),
                scores_bit_equal=True, orders_equal=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=100000)
    ap.add_argument("--users", type=int, default=4096)
    ap.add_argument("--candidates", type=int, default=300)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--parent-users", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dims", type=int, nargs="+", default=[768, 1536])
    ap.add_argument("--out", default=os.path.join("profiles", "fm_rank_bench.json"))
    args = ap.parse_args()
    rng = np.random.default_rng(1)
    res = dict(method="median [min-max] of %d repetitions after a warm-up, routes alternating; the parent route on the first "
                      "%d users only" % (args.reps, args.parent_users), runs=[run(D, args, rng) for D in args.dims])
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
