#!/usr/bin/env python3
"""ALS epochs at nFactors 192 and 256 in form 0 (the residual recurrence) and form 1 (the Deep Gram form, csrc/als_deep.hip) on the C5
quarter shard (125 000 x 100 000, 12.5 M entries: the shape DESIGN.md section 4 uses for nFactors 128).

Both forms run on ONE handle, alternating, from the same seeded factors: a warm-up epoch of each, then --epochs timed epochs of each;
median [min - max] per form.  An epoch is timed by the host clock around gorse_als_epoch, which returns behind a stream synchronise
(gorse_mf_epoch_times counts BPR's enqueued epochs only); the kernels' own event times (profile classes ALS_SWEEP / ALS_GRAM) of the
same epochs are recorded beside it.  Accuracy: the user half-sweep of each form against a float64 Gram solve on --check-rows rows
(evenly spaced through the side, plus its longest row), as a multiple of the ALS bar 1e-4 |ref| + 5e-5 rowmax |ref|.
Writes profiles/als_deep_bench.json (rewritten after every measurement, so an interrupted run keeps what it has)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gorse_amd import capi, synth  # noqa: E402

W, REG = 0.001, 0.06  # the ALS defaults (model.go:577-586)


def gram_rows_fp64(P, Q, uptr, uidx, iptr, rows):
    Q64 = Q.astype(np.float64)
    has = np.diff(iptr) > 0
    S = Q64[has].T @ Q64[has]
    out = np.empty((len(rows), P.shape[1]))
    for k, u in enumerate(rows):
        Bu = Q64[uidx[uptr[u]:uptr[u + 1]]]
        M, s, p = (1 - W) * (Bu.T @ Bu) + W * S, Bu.sum(axis=0), P[u].astype(np.float64)
        for f in range(p.size):
            p[f] = (s[f] - (M[f] @ p - M[f, f] * p[f])) / (M[f, f] + REG)
        out[k] = p
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=125_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--nnz", type=int, default=12_500_000)
    ap.add_argument("--widths", type=int, nargs="+", default=[192, 256])
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--check-rows", type=int, default=48)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "als_deep_bench.json"))
    a = ap.parse_args()
    assert capi.device_count() >= 1, "no MI355X visible"
    uptr, uidx, iptr, iidx = synth.s_als(a.users, a.items, a.nnz, 45)
    result = {"shape": {"users": a.users, "items": a.items, "entries": int(uptr[-1])}, "weight": W, "reg": REG, "epochs": a.epochs, "widths": {}}

    def save():
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")

    rows = np.unique(np.concatenate([np.linspace(0, a.users - 1, a.check_rows).astype(np.int64), [int(np.diff(uptr).argmax())]]))
    for d in a.widths:
        P, Q = synth.init_factors(a.users, a.items, d, 0.0, 0.1, 1)
        mf = capi.MF(a.users, a.items, d, uptr, uidx, iptr, iidx)
        r = result["widths"][str(d)] = {"form0_ms": [], "form1_ms": [], "form0_kernels_ms": [], "form1_kernels_ms": []}
        ref = gram_rows_fp64(P, Q, uptr, uidx, iptr, rows)
        bar = 1e-4 * np.abs(ref) + 5e-5 * np.abs(ref).max(axis=1, keepdims=True)
        mf.set_profiling(True)
        for form in (1, 0):  # warm-up (allocations, code objects) and accuracy: one user half-sweep, then one whole epoch
            mf.set_als_form(form)
            mf.set_factors(P, Q)
            mf.als_half_epoch(0, W, REG)
            got = mf.get_factors()[0][rows].astype(np.float64)
            r["form%d_family" % form] = mf.als_form()[1]
            r["form%d_worst_over_bar" % form] = float((np.abs(got - ref) / bar).max())
            mf.set_factors(P, Q)
            t0 = time.perf_counter()
            mf.als_epoch(W, REG)
            r["form%d_warmup_ms" % form] = (time.perf_counter() - t0) * 1e3
            print("nFactors %d form %d: family %d, worst error / bar %.3f, warm-up epoch %.2f ms" % (
                d, form, r["form%d_family" % form], r["form%d_worst_over_bar" % form], r["form%d_warmup_ms" % form]), flush=True)
            save()
        for _ in range(a.epochs):
            for form in (0, 1):
                mf.set_als_form(form)
                mf.set_factors(P, Q)
                mf.reset_profile()
                t0 = time.perf_counter()
                mf.als_epoch(W, REG)
                r["form%d_ms" % form].append((time.perf_counter() - t0) * 1e3)
                r["form%d_kernels_ms" % form].append(mf.get_profile(capi.PROF_ALS_SWEEP)[1] + mf.get_profile(capi.PROF_ALS_GRAM)[1])
                save()
        for form in (0, 1):
            ms = np.array(r["form%d_ms" % form])
            r["form%d_median_min_max_ms" % form] = [float(np.median(ms)), float(ms.min()), float(ms.max())]
        r["form0_over_form1"] = r["form0_median_min_max_ms"][0] / r["form1_median_min_max_ms"][0]
        print("nFactors %d: form 0 %.2f [%.2f - %.2f] ms, form 1 %.2f [%.2f - %.2f] ms, ratio %.2f" % (
            (d,) + tuple(r["form0_median_min_max_ms"]) + tuple(r["form1_median_min_max_ms"]) + (r["form0_over_form1"],)), flush=True)
        save()
        mf.close()


if __name__ == "__main__":
    main()
