#!/usr/bin/env python3
"""The deep sweep form of the exact top-k (gorse_topk_set_deep_sweep, csrc/topk_deep.hip) beside the scan on ONE handle and commit:
  emb1024   200,000 x 1024 bf16, Euclidean, k = 100, all pairs (the reference's shipped embedding width)
  emb1536   100,000 x 1536 bf16, cosine, k = 100
  f32_768   100,000 x 768 fp32, -dot, k = 100
mode 0 (the yardstick: the parent commit's code path, the vector-ALU scan) is timed on the first --subset queries only -- at 0.2 ms
per query a whole pass is tens of seconds -- and mode 1 on the same queries and on the whole range.  Seeded inputs, one warm-up
of every timed call, the two modes ALTERNATING inside a repetition (the mode is switched outside the timed region), median [min -
max] of --reps host-clock times (every call ends with its results on the host) and the handle's device-event time per profile class
of the last repetition.  The rows of both modes on the subset are asserted equal in every bit.
deep_flops = 2 x padded depth x N x queries over the PROF_TOPK_DEEP time, share_of_bf16_peak against bench.py's dense bf16 MFMA peak;
l2_bytes = N x queries x padded depth x 2 x (1 / 128 + 1 / 256), what the 128 x 256 tiles re-read (topk_deep_plan.hpp), and the
bandwidth that implies over the same time.
--ties 0,1 measures the tie replay of a deep handle instead (gorse_topk_set_deep_tie_replay, csrc/topk_deep_hist.hip): the same three
shapes, EVERY query, mode 1, the setting off (the yardstick: the parent commit's code path, ties to the literal scan) and on
alternating on one handle, a warm-up, median [min - max] of --reps, the rows of the two asserted equal in every bit, the device time
per profile class and gorse_topk_last_stats of both; output to profiles/topk_deep_ties_bench.json.
usage: bench_topk_deep.py [--reps 5] [--subset 8192] [--scale 1.0] [--ties 0,1] [--out profiles/topk_deep_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gorse_amd import capi  # noqa: E402

MFMA_BF16_PEAK_TFLOPS = 2500.0  # bench.py
CLASSES = {"scan_score": capi.PROF_TOPK_SCORE, "scan_select": capi.PROF_TOPK_RESCORE, "deep_sweep": capi.PROF_TOPK_DEEP,
           "rescore": capi.PROF_TOPK_SELECT, "hist_sweep": capi.PROF_TOPK_HIST, "sort_replay": capi.PROF_TOPK_REPLAY}
SHAPES = (("emb1024", 200_000, 1024, capi.DTYPE_BF16, capi.METRIC_EUCLIDEAN), ("emb1536", 100_000, 1536, capi.DTYPE_BF16, capi.METRIC_COSINE),
          ("f32_768", 100_000, 768, capi.DTYPE_F32, capi.METRIC_NEG_DOT))


def stats(ts):
    return {"median_s": float(np.median(ts)), "min_s": float(np.min(ts)), "max_s": float(np.max(ts)), "reps": len(ts)}


def timed(t, fn):
    before = {c: t.get_profile(v)[1] for c, v in CLASSES.items()}
    t0 = time.perf_counter()
    out = fn()
    dt = time.perf_counter() - t0
    return dt, out, {c: t.get_profile(v)[1] - before[c] for c, v in CLASSES.items()}


def run(name, N, d, dtype, metric, k, reps, subset):
    rng = np.random.default_rng(1000 + d)
    Xf = rng.standard_normal((N, d), dtype=np.float32)
    X = (Xf.view(np.uint32) >> 16).astype(np.uint16) if dtype == capi.DTYPE_BF16 else Xf
    del Xf
    t = capi.TopK(X, metric, dtype=dtype)
    t.set_profiling(True)
    nq = min(subset, N)
    kpad = -(-(d if dtype == capi.DTYPE_BF16 else 3 * d) // 64) * 64
    ts = {"mode0_subset": [], "mode1_subset": [], "mode1_all": []}
    ms = {}
    for rep in range(-1, reps):  # rep -1: the warm-up of every call
        t.set_deep_sweep(0)
        dt, (i0, d0), ms["mode0_subset"] = timed(t, lambda: t.all_pairs(k, 0, nq))
        assert t.get_deep_sweep() == (0, 0, 0)
        t.set_deep_sweep(1)
        dt1, (i1, d1), ms["mode1_subset"] = timed(t, lambda: t.all_pairs(k, 0, nq))
        assert t.get_deep_sweep() == (1, 1, 1)
        fb_subset = t.last_stats()[0]
        assert np.array_equal(i0, i1) and np.array_equal(d0.view(np.uint32), d1.view(np.uint32)), "the modes differ"
        dta, _, ms["mode1_all"] = timed(t, lambda: t.all_pairs(k))
        fb_all = t.last_stats()[0]
        if rep >= 0:
            ts["mode0_subset"].append(dt), ts["mode1_subset"].append(dt1), ts["mode1_all"].append(dta)
    res = {"workload": "%s: %d x %d %s, metric %d, k = %d; subset = the first %d queries" % (name, N, d, "bf16" if dtype == capi.DTYPE_BF16 else "fp32", metric, k, nq),
           "padded_depth": kpad, "to_the_scan": {"mode1_subset": fb_subset, "mode1_all": fb_all}, "rows_equal_on_subset": True}
    for c in ts:
        res[c] = dict(stats(ts[c]), device_ms_last_rep=ms[c])
    for c, q in (("mode1_subset", nq), ("mode1_all", N)):
        sec = ms[c]["deep_sweep"] * 1e-3
        flops, l2 = 2.0 * kpad * N * q, float(N) * q * kpad * 2 * (1 / 128 + 1 / 256)
        res[c].update(deep_tflops=flops / sec / 1e12, share_of_bf16_peak=flops / sec / 1e12 / MFMA_BF16_PEAK_TFLOPS, l2_bytes=l2, l2_tb_per_s=l2 / sec / 1e12)
    res["speedup_on_subset"] = res["mode0_subset"]["median_s"] / res["mode1_subset"]["median_s"]
    print(name, json.dumps(res), flush=True)
    return res


def run_ties(name, N, d, dtype, metric, k, reps, settings):
    rng = np.random.default_rng(1000 + d)
    Xf = rng.standard_normal((N, d), dtype=np.float32)
    X = (Xf.view(np.uint32) >> 16).astype(np.uint16) if dtype == capi.DTYPE_BF16 else Xf
    del Xf
    t = capi.TopK(X, metric, dtype=dtype)
    t.set_profiling(True)
    t.set_deep_sweep(1)
    ts, ms, last, rows = {s: [] for s in settings}, {}, {}, {}
    for rep in range(-1, reps):  # rep -1: the warm-up
        for s in settings:  # alternating; the setting is switched outside the timed region
            t.set_deep_tie_replay(s)
            dt, rows[s], ms[s] = timed(t, lambda: t.all_pairs(k))
            assert t.get_deep_sweep() == (1, 1, 1) and t.get_deep_tie_replay()[0] == s
            last[s] = dict(zip(("n_fallback", "n_tie"), t.last_stats()))
            if rep >= 0:
                ts[s].append(dt)
        for s in settings[1:]:
            assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(rows[settings[0]], rows[s])), "the settings differ"
    res = {"workload": "%s: %d x %d %s, metric %d, k = %d, every query, mode 1" % (name, N, d, "bf16" if dtype == capi.DTYPE_BF16 else "fp32", metric, k),
           "rows_equal": len(settings) > 1}
    for s in settings:
        res["ties_%d" % s] = dict(stats(ts[s]), device_ms_last_rep=ms[s], last_stats=last[s])
    if 0 in settings and 1 in settings:
        res["off_over_on"] = res["ties_0"]["median_s"] / res["ties_1"]["median_s"]
    print(name, json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--subset", type=int, default=8192)
    ap.add_argument("--scale", type=float, default=1.0, help="scales every shape's row count (a quick run)")
    ap.add_argument("--ties", default="", help="0,1: measure the deep tie replay off and on instead (every query, mode 1)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if capi.device_count() < 1:
        raise SystemExit("no MI355X visible: nothing is measured without one")
    a.out = a.out or os.path.join(ROOT, "profiles", "topk_deep_ties_bench.json" if a.ties else "topk_deep_bench.json")
    if a.ties:
        settings = [int(s) for s in a.ties.split(",")]
        assert settings and set(settings) <= {0, 1}, "--ties takes 0, 1 or 0,1"
        out = {name: run_ties(name, int(N * a.scale), d, dtype, metric, 100, a.reps, settings) for name, N, d, dtype, metric in SHAPES}
    else:
        out = {name: run(name, int(N * a.scale), d, dtype, metric, 100, a.reps, a.subset) for name, N, d, dtype, metric in SHAPES}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
