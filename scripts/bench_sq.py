#!/usr/bin/env python3
"""The scalar-quantised index (gorse_sq, csrc/sq.hip) beside the bf16 index (gorse_topk) on the same vectors and commit:
  c4      S-emb 1,000,000 x 128, cosine, k = 100 (BASELINE config C4): every stored row as a query
  ml1m    S-ml1m-sized item factors, 3706 x 64, Dot, k = 100
  sq      SQIndex.search_rows over all rows with the own row left out; the lists come to the host (the ABI has no other form)
  bf16    (the yardstick) TopK(bf16).all_pairs, results fetched to the host as well; bf16_device_only_s = the same call with the
          results left on the device, the form bench.py times
The two calls ALTERNATE inside a repetition after one warm-up each; median [min - max] of --reps host-clock times (both calls end in a
synchronise).  kernels_ms = the sq handle's per-class device-event times of its last repetition.  sweep_share_of_int8_peak = the
algorithmic int8 operations of the sweep (2 N^2 d, the padding not counted) over the sweep class's device time, as a share of the int8
matrix peak taken as twice bench.py's bf16 peak.  recall_at_k = the share of the fp32 exact top-k (TopK fp32, the same vectors) that the
quantised lists hold, over the first --recall-queries rows.
NOT measured: how the sq call's host time outside its kernels divides between the hand-back's flag download and the result copies.
usage: bench_sq.py [--reps 5] [--rows 1000000] [--recall-queries 4096] [--out profiles/sq_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gorse_amd import capi, synth  # noqa: E402

INT8_PEAK_TOPS = 2 * 2500.0  # v_mfma_i32_32x32x32_i8 issues at twice the bf16 rate; bench.py MFMA_BF16_PEAK_TFLOPS


def stats(ts):
    return {"median_s": float(np.median(ts)), "min_s": float(np.min(ts)), "max_s": float(np.max(ts)), "reps": len(ts)}


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def run(name, X32, Xb, metric, k, reps, recall_queries):
    N, d = X32.shape
    sq, bf = capi.SQIndex(X32, metric), capi.TopK(Xb, metric, dtype=capi.DTYPE_BF16)
    sq.set_profiling(True)
    sq_call = lambda: sq.search_rows(k, exclude_self=True)  # noqa: E731
    bf_call = lambda: bf.all_pairs(k)  # noqa: E731
    sq_call(), bf_call()
    ts, tb, td = [], [], []
    for _ in range(reps):
        before = sq.get_profile()
        t, (idx, _, cnt) = timed(sq_call)
        ts.append(t)
        after = sq.get_profile()
        tb.append(timed(bf_call)[0])
        td.append(timed(lambda: (bf.all_pairs(k, fetch=False), bf.synchronize()))[0])
    kernels = {c: after[c][1] - before[c][1] for c in capi.SQ_PROF}
    nq = min(recall_queries, N)
    exact = capi.TopK(X32, metric)
    eidx, _, ecnt = exact.search_index(np.arange(nq), k + 1)
    hit = tot = 0
    for q in range(nq):
        want = [r for r in eidx[q, :ecnt[q]] if r != q][:k]
        hit += np.intersect1d(want, idx[q, :cnt[q]]).size
        tot += len(want)
    res = {"workload": "%s: %d x %d, metric %d, k = %d, every row a query" % (name, N, d, metric, k),
           "sq": stats(ts), "bf16": stats(tb), "bf16_device_only": stats(td), "sq_kernels_ms": kernels,
           "sq_last_stats": dict(zip(("sweep", "scan", "handed_back"), sq.last_stats())),
           "recall_at_k": hit / max(tot, 1), "recall_queries": nq}
    if kernels["sweep"] > 0:
        res["sweep_share_of_int8_peak"] = 2.0 * N * N * d / (kernels["sweep"] * 1e-3) / (INT8_PEAK_TOPS * 1e12)
    print(name, json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--recall-queries", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sq_bench.json"))
    a = ap.parse_args()
    if capi.device_count() < 1:
        raise SystemExit("no MI355X visible: nothing is measured without one")
    out = {}
    _, Q = synth.init_factors(16, 3706, 64, 0.0, 0.1, 1)
    out["ml1m"] = run("ml1m", Q, (Q.view(np.uint32) >> 16).astype(np.uint16), capi.METRIC_NEG_DOT, 100, a.reps, a.recall_queries)
    Xb, X32 = synth.s_emb(a.rows, 128)
    out["c4"] = run("c4", X32, Xb, capi.METRIC_COSINE, 100, a.reps, a.recall_queries)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
