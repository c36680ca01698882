#!/usr/bin/env python3
"""Replacement on the device (gorse_cand_add_replacement + gorse_fm_rank_cand_decayed, csrc/cand_replace.hip) against the same
commit's host route, at scripts/bench_cand_chain.py's workload: --users users (100,000), 200,000 items, k = 100, the CTR ranker at
nFactors 16 with one field of D = 768.  The pass before it is item-to-item -> user-to-user -> a 100-entry shared list -> finish
with S-big's positives as base exclusion rows (the mf search adds candidates of the same kind and four seconds per pass; it is left
out).  The history is the same positives, every tenth entry marked read; one item in a hundred is gone.
  device  CandidateChain.add_replacement, FM.rank_cand_decayed
  host    CandidateChain.get, the set arithmetic in numpy as tests/replace_ref.py does it per user (vectorised over composite
          row * n_items + item keys), FM.rank_users on the rebuilt CSR, the decay and one stable numpy sort under the same rule.
          The parent commit has no such path, so there is no parent time.
A finished pass takes its replacement rows once, so every timed run is preceded by an untimed pass; inside a repetition the routes
ALTERNATE.  One warm-up repetition, then --reps; median, min and max of the wall time are reported, the device times from
gorse_cand_replacement_stats and gorse_fm_rank_stats (and gorse_fm_rank_cand's on the same grown pass beside the decayed call's),
and the bytes each route moves across PCIe, COUNTED FROM THE CODE (the arrays each call copies, written down beside the calls
below), not measured.  The script fails unless both routes give the same grown rows, score bits, decayed doubles and orders.
NOT measured: the split of the device time between the stage's kernels, and of the host route's time between numpy and the calls;
a pass whose history is partly among the candidates (here the base rows exclude all of it, so every existing item is appended).
usage: bench_cand_replace.py [--users 100000] [--reps 5] [--batch 1024] [--out profiles/cand_replace_bench.json]"""
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
from bench_cand_chain import stats  # noqa: E402
from bench_fm_rank import to_bf16  # noqa: E402
from bench_nbr_recommend import neighbour_table  # noqa: E402

K, SHARED, D_FM, D_EMB = 100, 100, 16, 768
PD, RD = 0.8, 0.7
f32 = np.float32


def rank_key(s):
    """fm_rank_order.hpp's key of float32 scores, ascending = ranked first"""
    b = s.view(np.uint32).copy()
    nan = (b & 0x7fffffff) > 0x7f800000
    b[b == 0x80000000] = 0
    asc = np.where(b & 0x80000000, ~b, b | np.uint32(0x80000000))
    return np.where(nan, np.uint32(0xffffffff), ~asc)


def decay_key(f):
    """the same for the decayed doubles"""
    b = f.view(np.uint64).copy()
    sign = np.uint64(1) << np.uint64(63)
    nan = (b & ~sign) > np.uint64(0x7ff0000000000000)
    b[b == sign] = 0
    asc = np.where(b & sign, ~b, b | sign)
    return np.where(nan, ~np.uint64(0), ~asc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cand_replace_bench.json"))
    a = ap.parse_args()
    n = a.users
    data = synth.s_big_shard(0, 8)
    I = int(data.I)
    uptr, uidx = np.asarray(data.uptr[:n + 1], np.int64), np.asarray(data.uidx[:data.uptr[n]], np.int32)
    rng = np.random.default_rng(1)
    kind = np.where(np.arange(uidx.size) % 10 == 9, capi.CAND_KIND_READ, capi.CAND_KIND_POSITIVE).astype(np.uint8)
    exists = (rng.uniform(0, 1, I) > 0.01).astype(np.uint8)

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
    users_bytes = 8 * (n + 1) + 8 * fu_idx.size + 4 * n

    def finished_pass():
        chain.begin(n, 3 * K, uptr, uidx)
        chain.add_nbr(i2i, None, K)
        chain.add_nbr(u2u, None, K)
        chain.add_shared(latest, latest_scores, K)
        chain.finish()

    def device_route():
        t0 = time.perf_counter()
        chain.add_replacement(uptr, uidx, kind, exists)
        scores, final, order = fm.rank_cand_decayed(chain, fu_ptr, fu_idx, fu_val, a.batch, PD, RD, user_lead=lead_u)
        wall = time.perf_counter() - t0
        total = chain.info()[2]
        dev = {"replacement_ms": chain.replacement_stats()[3], "rank_decayed_ms": fm.rank_stats()["device_ms"]}
        # add_replacement: the history pointer, one word per entry and keep up; the grown row pointer, one total and two counts back.
        # rank_cand_decayed: the users' rows, the row pointer and the plan (16 bytes per row) up; scores, decayed scores and order back
        pcie = {"add_replacement": 8 * (n + 1) + 4 * uidx.size + I + 8 * (n + 1) + 24,
                "rank_cand_decayed": users_bytes + 8 * (n + 1) + 16 * total + (4 + 8 + 4) * total}
        return wall, dev, pcie, (scores, final, order)

    def host_route():
        t0 = time.perf_counter()
        cptr, items, scores, stages = chain.get()
        old = items.size
        rows_c = np.repeat(np.arange(n, dtype=np.int64), np.diff(cptr))
        rows_h = np.repeat(np.arange(n, dtype=np.int64), np.diff(uptr))
        # distinct (row, item), positive first; existing items only
        words = np.unique((rows_h * I + uidx) * 2 + (kind == capi.CAND_KIND_READ))
        hkey, hread = words >> 1, (words & 1).astype(bool)
        first = np.concatenate([[True], hkey[1:] != hkey[:-1]])
        first &= exists[hkey % I].astype(bool)
        hkey, hread = hkey[first], hread[first]
        absent = ~np.isin(hkey, rows_c * I + items)
        add_rows, add_items = hkey[absent] // I, (hkey[absent] % I).astype(np.int32)
        place = np.argsort(np.concatenate([rows_c, add_rows]), kind="stable")
        g_items = np.concatenate([items, add_items])[place]
        g_scores = np.concatenate([scores, np.zeros(add_items.size)])[place]
        g_stages = np.concatenate([stages, np.full(add_items.size, capi.CAND_STAGE_REPLACEMENT, np.uint8)])[place]
        g_rows = np.concatenate([rows_c, add_rows])[place]
        g_ptr = np.concatenate([[0], np.cumsum(np.bincount(g_rows, minlength=n))]).astype(np.int64)
        r_scores, _ = fm.rank_users(fu_ptr, fu_idx, fu_val, g_ptr, g_items, a.batch, user_lead=lead_u, order=False)
        rank_ms = fm.rank_stats()["device_ms"]
        # the decay: every candidate's kind by a search in the history keys, one double multiply; then one stable sort
        gkey = g_rows * I + g_items
        at = np.minimum(np.searchsorted(hkey, gkey), hkey.size - 1)
        hit = hkey[at] == gkey
        final = r_scores.astype(np.float64)
        final[hit] = final[hit] * np.where(hread[at[hit]], RD, PD)
        pos = np.arange(g_items.size, dtype=np.int64) - g_ptr[g_rows]
        by = np.lexsort((pos, rank_key(r_scores), decay_key(final), g_rows))
        order = pos[by].astype(np.int32)
        wall = time.perf_counter() - t0
        total = g_items.size
        # get: items, scores and stage bytes back; rank_users: the users' rows, the row pointer, the candidates and the plan up, scores back
        pcie = {"get": (4 + 8 + 1) * old, "rank_users": users_bytes + 8 * (n + 1) + 4 * total + 16 * total + 4 * total}
        return wall, {"rank_users_ms": rank_ms}, pcie, (g_ptr, g_items, g_scores, g_stages, r_scores, final, order)

    walls = {"device": [], "host": []}
    devs = {"device": [], "host": []}
    for rep in range(a.reps + 1):  # repetition 0 warms up
        for route in (("device", "host") if rep % 2 else ("host", "device")):
            finished_pass()
            if route == "device":
                w, d_dev, d_pcie, d_out = device_route()
                d_get = chain.get()
                stats_ = chain.replacement_stats()
                _, want_order = fm.rank_cand(chain, fu_ptr, fu_idx, fu_val, a.batch, user_lead=lead_u)  # on the same grown pass
                d_dev["rank_cand_ms_on_the_same_pass"] = fm.rank_stats()["device_ms"]
                dev = d_dev
            else:
                w, dev, h_pcie, h_out = host_route()
            print("rep %d %s %.3f s" % (rep, route, w), file=sys.stderr, flush=True)
            if rep:
                walls[route].append(w)
                devs[route].append(dev)
    for x, y, what in zip(d_get, h_out[:4], ("row pointer", "items", "scores", "stages")):
        same = np.array_equal(x.view(np.uint64), y.view(np.uint64)) if what == "scores" else np.array_equal(x, y)
        assert same, "the two routes' grown rows differ: " + what
    assert np.array_equal(d_out[0].view(np.uint32), h_out[4].view(np.uint32)), "the two routes' ranker scores differ"
    assert np.array_equal(d_out[1].view(np.uint64), h_out[5].view(np.uint64)), "the two routes' decayed scores differ"
    assert np.array_equal(d_out[2], h_out[6]), "the two routes' orders differ"

    res = {"users": n, "items": I, "k": K, "shared_list": SHARED, "fm_factors": D_FM, "embedding_dim": D_EMB, "batch_size": a.batch,
           "positive_decay": PD, "read_decay": RD, "history_entries": int(uidx.size), "candidates_before": int(h_out[0][-1] - stats_[0]),
           "appended": stats_[0], "replacement_rows_positive": stats_[1], "replacement_rows_read": stats_[2],
           "order_differs_from_the_rankers_in": int(np.sum(d_out[2] != want_order)),
           "method": "median [min-max] of %d repetitions after a warm-up, an untimed pass before every run, the routes alternating; "
                     "pcie bytes counted from the code, without kernel arguments" % a.reps,
           "same_bits": True, "routes": {}}
    for r, pcie in (("device", d_pcie), ("host", h_pcie)):
        res["routes"][r] = {"wall": stats(walls[r]), "device_ms_median": {k: float(np.median([d[k] for d in devs[r]])) for k in devs[r][0]},
                            "pcie_bytes": pcie, "pcie_bytes_total": int(sum(pcie.values()))}
    res["ratio_host_over_device_wall"] = res["routes"]["host"]["wall"]["median_s"] / res["routes"]["device"]["wall"]["median_s"]
    res["not_measured"] = ("the split of replacement_ms between sort, mark, scan and write and of rank_decayed_ms between scoring and the "
                           "decay sort beyond the difference to rank_cand_ms_on_the_same_pass; the host route's split between numpy and "
                           "the calls; a pass whose history is partly among its candidates; the pass with the mf stage in front")
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
