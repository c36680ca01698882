#!/usr/bin/env python3
"""The offline pass's recommenders chained on the device (gorse_cand, csrc/cand.hip) against the same commit's host route, at the
README's neighbourhood workload: 200,000 items x 100 neighbours, --users users (100,000) with S-big's positives as base exclusion
rows, k = 100, an mf model over the same users / items at nFactors 64.  The pass is
    mf -> item-to-item -> user-to-user -> a 100-entry shared list -> the CTR ranker at nFactors 16 with one field of D = 768.
  chain   CandidateChain: begin, add_mf, add_nbr, add_nbr, add_shared, finish, FM.rank_cand
  host    the public host-to-host calls glued as tests/cand_ref.py glues them, with numpy: MF.recommend under the base rows, every
          list filtered against the user's rows and concatenated into them, NbrRecommender.recommend under the concatenated rows
          (twice), the shared list filtered per user (vectorised), the candidate CSR assembled on the host, FM.rank_users.
          The parent commit has no such path, so there is no parent time.
Every route runs once to warm up, then --reps times, the routes ALTERNATING inside a repetition; median, min and max are reported:
wall time, device time (the calls' own event times added up), stage_ms / chain_ms per stage, and the bytes each route moves
across PCIe, COUNTED FROM THE CODE (the arrays each call copies, written down beside the calls below), not measured; not counted:
the mf search's literal-route rows (k items, k scores and a count per such query, up on the chain route), kernel arguments.
The script fails unless both routes give the same candidates, score bits, stage order, ranker scores and ranker order.
NOT measured: which of the chain's kernels (filter, scan, append, merge) holds chain_ms; the host route's split between numpy and
the calls.
usage: bench_cand_chain.py [--users 100000] [--reps 5] [--batch 1024] [--out profiles/cand_chain_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from gorse_amd import capi, synth  # noqa: E402
from bench_fm_rank import to_bf16  # noqa: E402
from bench_nbr_recommend import neighbour_table  # noqa: E402

K, SHARED, D_MF, D_FM, D_EMB = 100, 100, 64, 16, 768
f32 = np.float32


def stats(ts):
    return {"median_s": float(np.median(ts)), "min_s": float(np.min(ts)), "max_s": float(np.max(ts)), "reps": len(ts)}


class Rows:
    """the host route's exclusion rows: a CSR that lists are concatenated into (row order kept, no sort inside rows)"""

    def __init__(self, ptr, items, n_items):
        self.ptr, self.items, self.I = ptr, items, n_items

    def filter_and_take(self, items, cnt, k, check):
        """the first k entries of every row of `items` (n x width, cnt valid) that are not in the row's exclusion: a mask"""
        n, width = items.shape
        valid = np.arange(width)[None, :] < cnt[:, None]
        if check:
            rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(self.ptr))
            keys = np.arange(n, dtype=np.int64)[:, None] * self.I + items
            valid &= ~np.isin(keys, rows * self.I + self.items)
        valid &= np.cumsum(valid, axis=1) <= k
        return valid

    def append(self, items, valid):
        n = items.shape[0]
        add = valid.sum(axis=1)
        rows = np.concatenate([np.repeat(np.arange(n), np.diff(self.ptr)), np.repeat(np.arange(n), add)])
        order = np.argsort(rows, kind="stable")
        self.items = np.concatenate([self.items, items[valid]])[order]
        self.ptr = self.ptr + np.concatenate([[0], np.cumsum(add)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cand_chain_bench.json"))
    a = ap.parse_args()
    n = a.users
    data = synth.s_big_shard(0, 8)
    I = int(data.I)
    uptr, uidx = np.asarray(data.uptr[:n + 1], np.int64), np.asarray(data.uidx[:data.uptr[n]], np.int32)
    rng = np.random.default_rng(1)

    mf = capi.MF(n, I, D_MF, uptr, uidx)
    mf.set_factors(*synth.init_factors(n, I, D_MF, 0.0, 0.1, 1))
    ok = np.ones(I, np.uint8)
    iptr, iidx, iw = neighbour_table(rng, I, I)
    i2i = capi.NbrRecommender(I)
    i2i.set_table(capi.NBR_HOP1, uptr, uidx)
    i2i.set_table(capi.NBR_HOP2, iptr, iidx, iw, capi.NBR_RECIP, 1.0)
    nptr, nidx, nw = neighbour_table(rng, n, n)
    u2u = capi.NbrRecommender(I)
    u2u.set_table(capi.NBR_HOP1, nptr, nidx, nw, capi.NBR_RECIP, 1.0)
    u2u.set_table(capi.NBR_HOP2, uptr, uidx)
    latest = rng.choice(I, SHARED, replace=False).astype(np.int32)
    latest_scores = np.sort(rng.uniform(1e9, 2e9, SHARED))[::-1].copy()

    n_labels = 1000
    nf = n + I + 2 * n_labels
    fm = capi.FM(nf, D_FM, embedding_dims=(D_EMB,))
    fm.set_params(f32(0.1), rng.normal(0, 0.1, nf).astype(f32), rng.normal(0, 0.1, (nf, D_FM)).astype(f32))
    b = 1 / np.sqrt(D_EMB)
    fm.set_embedding_params(0, rng.normal(0, 0.3, (D_FM, D_EMB)).astype(f32), rng.uniform(-b, b, (D_EMB, D_FM)).astype(f32),
                            rng.normal(0, 0.1, D_FM).astype(f32), rng.uniform(-b, b, (D_EMB, D_FM)).astype(f32),
                            rng.normal(0, 0.1, D_FM).astype(f32))
    fu_idx = np.concatenate([np.arange(n)[:, None], n + I + rng.integers(0, n_labels, (n, 3))], 1).astype(np.int32)
    fi_idx = np.concatenate([n + np.arange(I)[:, None], n + I + n_labels + rng.integers(0, n_labels, (I, 3))], 1).astype(np.int32)
    fu_val, fi_val = rng.uniform(0.2, 1.0, fu_idx.shape).astype(f32), rng.uniform(0.2, 1.0, fi_idx.shape).astype(f32)
    emb = to_bf16(rng.normal(0, 1, (I, D_EMB)).astype(f32))
    fu_ptr, fi_ptr = np.arange(n + 1, dtype=np.int64) * 4, np.arange(I + 1, dtype=np.int64) * 4
    lead_u = np.ones(n, np.int32)
    fm.set_items(fi_ptr, fi_idx, fi_val, lead=np.ones(I, np.int32), embs=[emb])
    chain = capi.CandidateChain(I)

    def chain_route():
        dev, pcie = {}, {}
        chain.begin(n, 4 * K, uptr, uidx)
        pcie["begin"] = 8 * (n + 1) + 4 * uidx.size
        chain.add_mf(mf, None, K, item_ok=ok)
        chain.add_nbr(i2i, None, K)
        chain.add_nbr(u2u, None, K)
        chain.add_shared(latest, latest_scores, K)
        # per stage: the new row pointer back; mf: item_ok up, the literal flags back; nbr: order, capacity, offset per query up
        pcie["stages"] = 4 * 8 * (n + 1) + (I + 4 * n) + 2 * 16 * n + 12 * SHARED
        for s, name in enumerate(("mf", "item_to_item", "user_to_user", "shared")):
            dev[name] = dict(zip(("stage_ms", "chain_ms"), chain.stats(s)))
        chain.finish()
        scores, order = fm.rank_cand(chain, fu_ptr, fu_idx, fu_val, a.batch, user_lead=lead_u)
        total = chain.info()[2]
        dev["rank_ms"] = fm.rank_stats()["device_ms"]
        # finish: the row pointer back; rank: the users' rows, the row pointer and the plan (16 bytes per row) up, scores and order back
        pcie["finish_and_rank"] = 8 * (n + 1) + (8 * (n + 1) + 8 * fu_idx.size + 4 * n) + 8 * (n + 1) + 16 * total + 8 * total
        return dev, pcie, scores, order

    def host_route():
        dev, pcie = {}, {}
        R = Rows(uptr.copy(), uidx.copy(), I)
        cand_items, cand_scores, cand_stage = [], [], []

        def take(stage, items, scores, cnt, check):
            valid = R.filter_and_take(items, cnt, K, check)
            cand_items.append((items, valid))
            cand_scores.append(np.asarray(scores, np.float64))
            cand_stage.append(stage)
            R.append(items, valid)

        it, sc, cnt = mf.recommend(n, K, ok, uptr, uidx)
        dev["mf"] = {"stage_ms": mf.recommend_stats()[2]}
        pcie["mf"] = I + 8 * (n + 1) + 4 * uidx.size + 4 * n + n * K * 8 + 4 * n
        take(0, it, sc, cnt, True)
        for stage, (name, h) in enumerate((("item_to_item", i2i), ("user_to_user", u2u)), 1):
            pcie[name] = 8 * (n + 1) + 4 * R.items.size + 16 * n + n * K * 12 + 4 * n
            it, sc, cnt = h.recommend(n, K, R.ptr, R.items)
            dev[name] = {"stage_ms": h.recommend_stats()[2]}
            take(stage, it, sc, cnt, False)
        take(3, np.broadcast_to(latest, (n, SHARED)), np.broadcast_to(latest_scores, (n, SHARED)), np.full(n, SHARED), True)
        # the candidate CSR: per query the stages' kept entries in stage order
        counts = np.stack([v.sum(axis=1) for _, v in cand_items], axis=1)
        rows = np.concatenate([np.repeat(np.arange(n), c) for c in counts.T])
        order = np.argsort(rows, kind="stable")
        items = np.concatenate([i[v] for i, v in cand_items])[order]
        scores = np.concatenate([s[v] for s, (_, v) in zip(cand_scores, cand_items)])[order]
        stages = np.concatenate([np.full(int(c.sum()), s, np.uint8) for s, c in zip(cand_stage, counts.T)])[order]
        cptr = np.concatenate([[0], np.cumsum(counts.sum(axis=1))]).astype(np.int64)
        r_scores, r_order = fm.rank_users(fu_ptr, fu_idx, fu_val, cptr, items, a.batch, user_lead=lead_u)
        dev["rank_ms"] = fm.rank_stats()["device_ms"]
        total = items.size
        pcie["rank"] = (8 * (n + 1) + 8 * fu_idx.size + 4 * n) + 8 * (n + 1) + 4 * total + 16 * total + 8 * total
        return dev, pcie, (cptr, items, scores, stages), r_scores, r_order

    wall = {"chain": [], "host": []}
    devs = {"chain": [], "host": []}
    for rep in range(a.reps + 1):  # repetition 0 warms up
        t0 = time.perf_counter()
        c_dev, c_pcie, c_scores, c_order = chain_route()
        t1 = time.perf_counter()
        h_dev, h_pcie, h_cand, h_scores, h_order = host_route()
        t2 = time.perf_counter()
        print("rep %d chain %.3f s host %.3f s" % (rep, t1 - t0, t2 - t1), file=sys.stderr, flush=True)
        if rep:
            wall["chain"].append(t1 - t0)
            wall["host"].append(t2 - t1)
            devs["chain"].append(c_dev)
            devs["host"].append(h_dev)
    got = chain.get()
    for x, y, what in zip(got, h_cand, ("row pointer", "items", "scores", "stages")):
        same = np.array_equal(x.view(np.uint64), y.view(np.uint64)) if what == "scores" else np.array_equal(x, y)
        assert same, "the two routes' candidates differ: " + what
    assert np.array_equal(c_scores.view(np.uint32), h_scores.view(np.uint32)), "the two routes' ranker scores differ"
    assert np.array_equal(c_order, h_order), "the two routes' ranker orders differ"

    def device_total(d):
        return sum(v if isinstance(v, float) else sum(v.values()) for v in d.values()) * 1e-3

    def per_stage(ds):
        out = {}
        for name in ds[0]:
            if isinstance(ds[0][name], dict):
                out[name] = {key: float(np.median([d[name][key] for d in ds])) for key in ds[0][name]}
            else:
                out[name] = float(np.median([d[name] for d in ds]))
        return out

    res = {"users": n, "items": I, "neighbours": 100, "k": K, "shared_list": SHARED, "mf_factors": D_MF, "fm_factors": D_FM,
           "embedding_dim": D_EMB, "batch_size": a.batch, "base_exclusion_entries": int(uidx.size), "candidates": int(got[0][-1]),
           "exclusion_entries_at_the_end": int(chain.info()[3]),
           "method": "median [min-max] of %d repetitions after a warm-up, the routes alternating; pcie bytes counted from the code, without "
                     "the mf search's literal-route rows (808 bytes per such query on the chain route) and kernel arguments" % a.reps,
           "same_bits": True, "routes": {}}
    for r, pcie in (("chain", c_pcie), ("host", h_pcie)):
        res["routes"][r] = {"wall": stats(wall[r]), "device": stats([device_total(d) for d in devs[r]]),
                            "device_ms_median": per_stage(devs[r]), "pcie_bytes": pcie, "pcie_bytes_total": int(sum(pcie.values()))}
    res["ratio_host_over_chain_wall"] = res["routes"]["host"]["wall"]["median_s"] / res["routes"]["chain"]["wall"]["median_s"]
    res["not_measured"] = "which of filter, scan, append and merge holds chain_ms; the host route's split between numpy and the calls"
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
