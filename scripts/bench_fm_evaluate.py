#!/usr/bin/env python
"""Times the evaluation of the FM ranker from a resident test split against the host route it replaces inside Fit.

Workload: nFactors 16, one embedding field of D = 768 and again D = 1536; 200,000 test rows of width 8, about half of them
positive; batch size 1024.  The model is a ctr.FM after a short Fit on a training set of --train rows of the same shape.
  route A   FM.EvaluateResident() on the split FM.SetTest(test) made resident (SetTest is timed separately, once);
  route B   FM.Evaluate(test): partition, gather and pad on the host, upload, download the logits, std::sort.
Median [min-max] of --reps repetitions after a warm-up, the routes alternating.  The two routes' Scores must be equal in every
bit, or the script fails.  The device time of route A comes from gorse_fm_evaluate_stats on a capi.FM handle that holds the same
parameters and the same split, its split by stage (scoring | keys, sort and counts | the float32 chain) from the handle's events.
A Fit of --epochs epochs at Verbose 1 is timed with either route, and the evaluations' share of its wall time is reported.
Writes one JSON file."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gorse_amd import capi, ctr  # noqa: E402

f32 = np.float32


def to_bf16(x):
    u = np.ascontiguousarray(x, f32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def stat(ts):
    ts = sorted(ts)
    return dict(median_ms=1e3 * ts[len(ts) // 2], min_ms=1e3 * ts[0], max_ms=1e3 * ts[-1])


def rows(rng, n, nf, D, width=8):
    """n rows of `width` distinct-enough features with values in (0.2, 1), +-1 targets about half and half, and embeddings drawn
    from a pool of 4096 rows ~ Normal(0, 1) (every seventh pool row all zero: a sample without an embedding)"""
    idx = rng.integers(0, nf, (n, width)).astype(np.int32)
    val = rng.uniform(0.2, 1.0, (n, width)).astype(f32)
    tgt = np.where(rng.random(n) < 0.5, 1.0, -1.0).astype(f32)
    pool = to_bf16(rng.normal(0, 1, (4096, D)).astype(f32))
    pool[::7] = 0
    return idx, val, tgt, pool[rng.integers(0, 4096, n)]


def dataset(idx, val, tgt, emb, nf):
    n, w = idx.shape
    ds = ctr.Dataset(nf, (np.arange(n + 1, dtype=np.int64) * w, idx.reshape(-1), val.reshape(-1), tgt))
    ds.set_embeddings([emb])
    return ds


def run(D, args, rng):
    d, nf, bs = 16, 50000, args.batch
    tr, te = rows(rng, args.train, nf, D), rows(rng, args.rows, nf, D)
    train, test = dataset(*tr, nf), dataset(*te, nf)

    def fit(host_route):
        m = ctr.FM(nFactors=d, nEpochs=args.epochs, batchSize=bs, lr=0.001, reg=0.0, optimizer=ctr.Adam, seed=1)
        m.SetHostEvaluate(host_route)
        t0 = time.perf_counter()
        s = m.Fit(train, test, Verbose=1)
        return m, s, time.perf_counter() - t0, m.log()

    fit(False)  # warm-up: the library's first launches
    m_b, s_b, t_fit_b, lg_b = fit(True)
    m, s_a, t_fit_a, lg_a = fit(False)
    assert s_a == s_b and lg_a == lg_b, "the two Fits differ"
    n_evals = len(lg_a)

    t0 = time.perf_counter()
    m.SetTest(test)
    t_set = time.perf_counter() - t0
    m.EvaluateResident()
    m.Evaluate(test)
    t_a, t_b = [], []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        sa = m.EvaluateResident()
        t_a.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        sb = m.Evaluate(test)
        t_b.append(time.perf_counter() - t0)
        assert sa == sb, "the two routes' Scores differ: %r %r" % (sa, sb)
    assert not np.isnan(sa.AUC)

    # the same parameters and split on a bare handle, for the device's own clock
    fm = capi.FM(nf, d, embedding_dims=(D,))
    fm.set_params(*m.params())
    fm.set_embedding_params(0, *m.field_params(0))
    fm.set_test(te[0], te[1], te[2], [te[3]])
    fm.evaluate(bs)
    dev, stages = [], []
    for _ in range(args.reps):
        counts, auc_sum = fm.evaluate(bs)
        dev.append(fm.evaluate_stats()["device_ms"] * 1e-3)
        ms3 = (C.c_double * 3)()
        capi.check(capi.lib().gorse_hip_test_fm_evaluate_times(fm.h, ms3))
        stages.append([x * 1e-3 for x in ms3])
    st = fm.evaluate_stats()
    auc = f32(auc_sum) / f32(counts["n_pos"] * counts["n_neg"])
    assert f32(sa.AUC) == auc, "the bare handle's AUC differs: %r %r" % (sa.AUC, auc)
    fm.close()
    a, b = stat(t_a), stat(t_b)
    by_stage = {k: stat([s[i] for s in stages]) for i, k in enumerate(("scoring", "keys_sort_count", "chain"))}
    return dict(D=D, d=d, rows=args.rows, width=8, batch_size=bs, counts=counts, auc=float(auc), stats=st,
                set_test_ms=1e3 * t_set, route_a_resident=a, route_b_host=b, route_a_device=stat(dev), route_a_device_stages=by_stage,
                chain_share_of_device=by_stage["chain"]["median_ms"] / stat(dev)["median_ms"],
                uploaded_bytes_per_host_evaluation=args.rows * (2 * D + 8 * 8),
                fit=dict(train_rows=args.train, epochs=args.epochs, evaluations=n_evals,
                         wall_ms_host_route=1e3 * t_fit_b, wall_ms_resident=1e3 * t_fit_a,
                         evaluation_share_host_route=n_evals * b["median_ms"] / (1e3 * t_fit_b),
                         evaluation_share_resident=n_evals * a["median_ms"] / (1e3 * t_fit_a)),
                scores_bit_equal=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200000)
    ap.add_argument("--train", type=int, default=200000)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dims", type=int, nargs="+", default=[768, 1536])
    ap.add_argument("--out", default=os.path.join("profiles", "fm_evaluate_bench.json"))
    args = ap.parse_args()
    rng = np.random.default_rng(1)
    res = dict(method="median [min-max] of %d repetitions after a warm-up, routes alternating; Fit timed once per route after a "
                      "warm-up Fit; the evaluations' share of a Fit = evaluations x median evaluation / Fit wall time" % args.reps,
               runs=[run(D, args, rng) for D in args.dims])
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
