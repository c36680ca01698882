#!/usr/bin/env python
"""Times cf.Evaluate's device route (gorse_mf_evaluate_resident: rank lists, metrics and user-order sums on the device) against the
host route it replaces inside Fit (gorse_mf_rank_resident, then a set per user and the metrics on the host).

Workload: S-ml1m (6040 users x 3706 items, synthetic), one test item per user, 100 sampled negatives, topK 10, nFactors 16 and 64.
  evaluate   one model after a one-epoch BPR Fit of a production split: its handle holds the training set and the candidate lists,
             so cf.Evaluate ranks the resident lists as it does between the epochs of a Fit.  SetHostEvaluate(True / False) picks the
             route; the routes alternate, one warm-up each, then --reps repetitions: median [min-max] wall time.  Both routes must
             return the same bits, or the script fails.
  stages     the device route's own clock on a bare handle with the same lists: gorse_mf_evaluate_stats, split by the handle's
             events into the per-user kernel and the sum chain.
  fit        the 30-epoch Verbose 10 BPR Fit through the C++ twin, three runs per route after a warm-up, on the production split
             (resident lists) and on the NCF layout with preloaded negatives (lists uploaded per evaluation, what bench.py's fit leg
             runs): wall time, and the evaluations' share of it from the log's eval_time.
  large      200,000 evaluated users at nFactors 128 on a bare handle: evaluate_resident against rank_resident alone (the host
             route without its host half), the rank lists compared and the sums checked against the numpy chain; the chain's share.
Writes one JSON file."""
import argparse
import json
import os
import re
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gorse_amd import capi, cf, synth  # noqa: E402

f32 = np.float32


def stat(ts):
    ts = sorted(ts)
    return dict(median_ms=1e3 * ts[len(ts) // 2], min_ms=1e3 * ts[0], max_ms=1e3 * ts[-1])


def same_bits(a, b):
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a.view(np.uint32)[~np.isnan(a)], b.view(np.uint32)[~np.isnan(b)])


def evaluate_leg(data, d, reps):
    train, test = cf.datasets_from_synth(data, preload_negatives=False)
    m = cf.NewBPR({"NFactors": d, "Reg": 0.01, "Lr": 0.05, "NEpochs": 1, "InitMean": 0, "InitStdDev": 0.1})
    m.Fit(train, test, cf.NewFitConfig().SetJobs(1))  # leaves the handle with the training set and this split's lists resident
    six = (cf.NDCG, cf.Precision, cf.Recall, cf.HR, cf.MAP, cf.MRR)

    def once(host_route, scorers):
        m.SetHostEvaluate(host_route)
        t0 = time.perf_counter()
        s = cf.Evaluate(m, test, train, 10, 100, 1, *scorers)
        return time.perf_counter() - t0, s

    assert same_bits(once(True, six)[1], once(False, six)[1]), "the two routes differ (six metrics)"
    t_host, t_dev = [], []
    for _ in range(reps):
        th, sh = once(True, six[:3])  # Fit's three scorers
        td, sd = once(False, six[:3])
        assert same_bits(sh, sd), "the two routes differ: %r %r" % (sh, sd)
        t_host.append(th)
        t_dev.append(td)
    P, Q = m.factors()
    # the same lists and factors on a bare handle, for the device's own clock
    mf = capi.MF(data.U, data.I, d, data.uptr, data.uidx)
    mf.set_factors(P, Q)
    mf.sample_user_negatives(data.test_ptr, data.test_idx, 100, seed=0, fetch=False)
    sums, count = mf.evaluate_resident(10)
    assert same_bits((sums * (f32(1) / count))[:3], sd), "the bare handle's result differs"
    dev, stages, rank_only = [], [], []
    for _ in range(reps):
        mf.evaluate_resident(10)
        dev.append(mf.evaluate_stats()[2] * 1e-3)
        stages.append([x * 1e-3 for x in mf.evaluate_stage_times()])
        t0 = time.perf_counter()
        mf.rank_resident(10)
        rank_only.append(time.perf_counter() - t0)
    users, cands, _ = mf.evaluate_stats()
    mf.close()
    h, dv = stat(t_host), stat(t_dev)
    return dict(nFactors=d, users=users, candidates=cands, topK=10, ndcg=float(sd[0]), host_route=h, device_route=dv,
                device_range_below_host_range=dv["max_ms"] < h["min_ms"], rank_resident_alone=stat(rank_only),
                device_ms=stat(dev), device_ms_user_kernel=stat([s[0] for s in stages]), device_ms_chain=stat([s[1] for s in stages]),
                bits_equal=True)


def fit_leg(data, d, preload, runs):
    train, test = cf.datasets_from_synth(data, preload_negatives=preload)
    jobs = max(2, min(16, os.cpu_count() or 2))

    def fit(host_route, state):
        m = cf.NewBPR({"NFactors": d, "Reg": 0.01, "Lr": 0.05, "NEpochs": 30, "InitMean": 0, "InitStdDev": 0.001, "RandomState": state})
        m.SetHostEvaluate(host_route)
        t0 = time.perf_counter()
        s = m.Fit(train, test, cf.NewFitConfig().SetJobs(jobs))
        wall = time.perf_counter() - t0
        ev = [float(x) for x in re.findall(r"eval_time=([0-9.]+)ms", m.log)]
        return wall, ev, s.NDCG

    fit(False, 0)  # warm-up: code objects, buffers, the first sampling of this split
    fit(True, 0)
    out = {}
    for name, host_route in (("host_route", True), ("device_route", False)):
        out[name] = []
    for r in range(runs):  # the routes alternate
        for name, host_route in (("host_route", True), ("device_route", False)):
            wall, ev, ndcg = fit(host_route, 1 + r)
            # the first evaluation of a production split also samples the negatives: reported apart
            out[name].append(dict(wall_ms=1e3 * wall, evaluations=len(ev), eval_ms_first=ev[0], eval_ms_later_mean=float(np.mean(ev[1:])),
                                  eval_share_of_wall=sum(ev) / (1e3 * wall), ndcg=ndcg))
    for name in ("host_route", "device_route"):
        out[name + "_wall"] = stat([x["wall_ms"] * 1e-3 for x in out[name]])
    return dict(nFactors=d, preloaded_negatives=preload, jobs=jobs, **out)


def large_leg(U, I, d, reps):
    rng = np.random.default_rng(3)
    uptr = np.arange(U + 1, dtype=np.int64)
    uidx = rng.integers(0, I, U).astype(np.int32)
    tidx = ((uidx + 1 + rng.integers(0, I - 1, U)) % I).astype(np.int32)  # one test item per user, not the training item
    P, Q = synth.init_factors(U, I, d, 0.0, 0.1, 9)
    mf = capi.MF(U, I, d, uptr, uidx)
    mf.set_factors(P, Q)
    mf.sample_user_negatives(uptr, tidx, 100, seed=0, fetch=False)
    sums, count, per_user, rank, rlen = mf.evaluate_resident(10, per_user=True, ranks=True)
    eu, erank, erlen = mf.rank_resident(10)
    assert np.array_equal(rank, erank) and np.array_equal(rlen, erlen), "rank lists differ"
    assert same_bits(sums, np.cumsum(per_user, axis=1, dtype=f32)[:, -1]), "sums differ from the user-order chain"
    t_dev, t_rank, dev, stages = [], [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        mf.evaluate_resident(10)
        t_dev.append(time.perf_counter() - t0)
        dev.append(mf.evaluate_stats()[2] * 1e-3)
        stages.append([x * 1e-3 for x in mf.evaluate_stage_times()])
        t0 = time.perf_counter()
        mf.rank_resident(10)
        t_rank.append(time.perf_counter() - t0)
    mf.close()
    chain = stat([s[1] for s in stages])
    return dict(users=U, items=I, nFactors=d, candidates_per_user=101, topK=10, device_route=stat(t_dev), rank_resident_alone=stat(t_rank),
                device_ms=stat(dev), device_ms_user_kernel=stat([s[0] for s in stages]), device_ms_chain=chain,
                chain_ns_per_user=1e6 * chain["median_ms"] / U, chain_share_of_device=chain["median_ms"] / stat(dev)["median_ms"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fit-runs", type=int, default=3)
    ap.add_argument("--large-users", type=int, default=200000)
    ap.add_argument("--out", default=os.path.join("profiles", "mf_evaluate_bench.json"))
    args = ap.parse_args()
    data = synth.s_ml1m()
    res = dict(method="evaluate: median [min-max] of %d repetitions after a warm-up, host and device route alternating on one model's "
                      "handle, wall time around cf.Evaluate; device_ms from events on the handle's stream; fit: %d runs per route after a "
                      "warm-up, alternating" % (args.reps, args.fit_runs),
               evaluate=[evaluate_leg(data, d, args.reps) for d in (16, 64)],
               fit=[fit_leg(data, 16, preload, args.fit_runs) for preload in (False, True)],
               large=large_leg(args.large_users, 20000, 128, args.reps))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
