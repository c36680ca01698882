#!/usr/bin/env python
"""Times training and evaluating the FM ranker from (user, item) samples against the padded route on the materialised rows.

Workload (the README's FM configuration): nFactors 16, one embedding field of D = 768 and again D = 1536, 100,000 items,
50,000 users, --train (1M) training samples and --rows (200,000) test samples, batch size 1024.  A user row is its id entry and
3 labels, an item row its id entry and 4 labels, so a composed row holds 9 entries.
  padded route   set_train + set_train_embeddings + set_test on the rows and per-sample embeddings materialised on the host;
  sample route   set_items + set_train_samples + set_test_samples: the catalogue once, per sample three numbers.
Both routes run on the same data, alternating; every figure is the median [min-max] of --reps repetitions after a warm-up.
Measured: the set-up's wall time, the bytes it uploads (counted from the arrays handed over) and the device memory it holds
(hipMemGetInfo before and after, and again after the first epoch and evaluation, when the plans exist); the wall time of an Adam
epoch with the stream drained; the device time of an evaluation (gorse_fm_evaluate_stats); a --epochs (3) epoch Fit at Verbose 1
end to end through ctr.FM.Fit on the Materialise()d sets and through ctr.FM.FitSamples.  The script fails unless costs,
parameters, counts, logits and Scores of the two routes are equal in every bit.  Writes one JSON file."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gorse_amd import capi, ctr  # noqa: E402

f32, u32 = np.float32, np.uint32
N_USERS, N_ITEMS, N_UL, N_IL, K_UL, K_IL = 50000, 100000, 1000, 1000, 3, 4


def to_bf16(x):
    u = np.ascontiguousarray(x, f32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def stat(ts):
    ts = sorted(ts)
    return dict(median_ms=1e3 * ts[len(ts) // 2], min_ms=1e3 * ts[0], max_ms=1e3 * ts[-1])


def say(*a):
    print(*a, flush=True)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, f32).view(u32), np.asarray(b, f32).view(u32))


def free_bytes():
    hip = C.CDLL("libamdhip64.so")
    free, total = C.c_size_t(0), C.c_size_t(0)
    if hip.hipMemGetInfo(C.byref(free), C.byref(total)) != 0:
        raise RuntimeError("hipMemGetInfo failed")
    return int(free.value)


class World:
    """feature indices follow the unified index: users | items | user labels | item labels"""

    def __init__(self, rng, D, n_train, n_test, n_users=N_USERS, n_items=N_ITEMS):
        self.D, self.n_users, self.n_items = D, n_users, n_items
        base = n_users + n_items
        self.nf = base + N_UL + N_IL
        self.u_lab = base + rng.integers(0, N_UL, (n_users, K_UL)).astype(np.int32)
        self.i_lab = base + N_UL + rng.integers(0, N_IL, (n_items, K_IL)).astype(np.int32)
        self.u_val = rng.uniform(0.2, 1.0, (n_users, K_UL)).astype(f32)
        self.i_val = rng.uniform(0.2, 1.0, (n_items, K_IL)).astype(f32)
        pool = to_bf16(rng.normal(0, 1, (4096, D)).astype(f32))
        pool[::7] = 0  # an item without an embedding carries an all-zero row
        self.table = np.ascontiguousarray(pool[rng.integers(0, 4096, n_items)])
        self.train = self._samples(rng, n_train)
        self.test = self._samples(rng, n_test)

    def _samples(self, rng, n):
        return (rng.integers(0, self.n_users, n).astype(np.int32), rng.integers(0, self.n_items, n).astype(np.int32),
                np.where(rng.random(n) < 0.5, 1.0, -1.0).astype(f32))

    def side(self, ids, lab, val):
        """one side as the CSR set_items / rank_users take: the id entry (lead 1), then the labels"""
        n, k = lab.shape
        idx = np.concatenate([ids[:, None], lab], 1).astype(np.int32)
        v = np.concatenate([np.ones((n, 1), f32), val], 1)
        return np.arange(n + 1, dtype=np.int64) * (k + 1), idx.reshape(-1), v.reshape(-1), np.ones(n, np.int32)

    def users(self):
        return self.side(np.arange(self.n_users, dtype=np.int32), self.u_lab, self.u_val)

    def items(self):
        return self.side(self.n_users + np.arange(self.n_items, dtype=np.int32), self.i_lab, self.i_val)

    def materialise(self, samples):
        """the rows Dataset.Get composes (user id | item id | user labels | item labels) and the embeddings gathered per sample"""
        u, c, t = samples
        one = np.ones((u.size, 1), f32)
        idx = np.concatenate([u[:, None], (self.n_users + c)[:, None], self.u_lab[u], self.i_lab[c]], 1).astype(np.int32)
        val = np.concatenate([one, one, self.u_val[u], self.i_val[c]], 1).astype(f32)
        return np.ascontiguousarray(idx), np.ascontiguousarray(val), t, self.table[c]

    def label_rows(self):
        mk = lambda lab, val: [list(zip(a, b)) for a, b in zip(lab.tolist(), val.tolist())]  # noqa: E731
        return (np.arange(self.n_users, dtype=np.int32), mk(self.u_lab, self.u_val),
                self.n_users + np.arange(self.n_items, dtype=np.int32), mk(self.i_lab, self.i_val))


def nbytes(*arrs):
    return int(sum(a.nbytes for a in arrs))


def run(D, args, rng):
    d, bs = 16, args.batch
    t0 = time.perf_counter()
    w = World(rng, D, args.train, args.rows)
    tr, te = w.materialise(w.train), w.materialise(w.test)
    t_mat = time.perf_counter() - t0
    say("D=%d: world and materialised rows built on the host in %.1f s" % (D, t_mat))
    uptr, uidx, uval, ulead = w.users()
    iptr, iidx, ival, ilead = w.items()
    B, W, V = f32(0), rng.normal(0, 0.01, w.nf).astype(f32), rng.normal(0, 0.01, (w.nf, d)).astype(f32)
    bound = 1.0 / np.sqrt(D)
    field = (rng.normal(0, 0.01, (d, D)).astype(f32), rng.uniform(-bound, bound, (D, d)).astype(f32), np.zeros(d, f32),
             rng.uniform(-bound, bound, (D, d)).astype(f32), np.zeros(d, f32))

    def handle():
        fm = capi.FM(w.nf, d, embedding_dims=(D,))
        fm.set_params(B, W, V)
        fm.set_embedding_params(0, *field)
        return fm

    def setup_padded(fm):
        fm.set_train(tr[0], tr[1], tr[2])
        fm.set_train_embeddings(0, tr[3])
        fm.set_test(te[0], te[1], te[2], [te[3]])

    def setup_samples(fm):
        fm.set_items(iptr, iidx, ival, lead=ilead, embs=[w.table])
        fm.set_train_samples(uptr, uidx, uval, *w.train, user_lead=ulead)
        fm.set_test_samples(uptr, uidx, uval, *w.test, user_lead=ulead)

    up_padded = nbytes(tr[0], tr[1], tr[2], tr[3], te[0], te[1], te[3])
    up_samples = nbytes(iptr, iidx, ival, ilead, w.table) + 2 * nbytes(uptr, uidx, uval, ulead) + nbytes(*w.train) + nbytes(*w.test[:2])

    a, b = handle(), handle()
    held = {}
    for name, fm, setup in (("padded", a, setup_padded), ("samples", b, setup_samples)):
        f0 = free_bytes()
        setup(fm)  # the warm-up of the set-up timing as well
        held[name] = dict(after_setup=f0 - free_bytes())
        fm.epoch(bs, capi.OPT_ADAM, 0.001, 0.0)
        fm.evaluate(bs)
        held[name]["after_first_epoch_and_evaluation"] = f0 - free_bytes()
    say("D=%d: device memory held %s" % (D, held))
    for fm in (a, b):  # the same start for both
        fm.set_params(B, W, V)
        fm.set_embedding_params(0, *field)

    t_set = {"padded": [], "samples": []}
    for _ in range(args.reps):
        for name, fm, setup in (("padded", a, setup_padded), ("samples", b, setup_samples)):
            t0 = time.perf_counter()
            setup(fm)
            t_set[name].append(time.perf_counter() - t0)
    say("D=%d: set-up %s" % (D, {k: stat(v) for k, v in t_set.items()}))

    t_ep = {"padded": [], "samples": []}
    for rep in range(args.reps + 1):  # the first builds the plans: a warm-up
        costs = {}
        for name, fm in (("padded", a), ("samples", b)):
            t0 = time.perf_counter()
            costs[name] = fm.epoch(bs, capi.OPT_ADAM, 0.001, 0.0)
            if rep:
                t_ep[name].append(time.perf_counter() - t0)
        assert np.isfinite(costs["padded"]) and same_bits(costs["padded"], costs["samples"]), "the epoch costs differ: %r" % costs
    pa, pb = a.get_params(), b.get_params()
    assert all(same_bits(x, y) for x, y in zip(pa, pb)), "B, W, V differ"
    assert all(same_bits(x, y) for x, y in zip(a.get_embedding_params(0), b.get_embedding_params(0))), "the field's tensors differ"
    say("D=%d: epoch %s" % (D, {k: stat(v) for k, v in t_ep.items()}))

    t_ev = {"padded": [], "samples": []}
    for rep in range(args.reps + 1):
        outs = {}
        for name, fm in (("padded", a), ("samples", b)):
            outs[name] = fm.evaluate(bs, logits=rep == 0)
            if rep:
                t_ev[name].append(fm.evaluate_stats()["device_ms"] * 1e-3)
        assert outs["padded"][0] == outs["samples"][0] and same_bits(outs["padded"][1], outs["samples"][1]), "the evaluations differ"
        if rep == 0:
            assert same_bits(outs["padded"][2], outs["samples"][2]), "the logits differ"
    counts = outs["padded"][0]
    say("D=%d: evaluation %s" % (D, {k: stat(v) for k, v in t_ev.items()}))
    a.close()
    b.close()

    # Fit end to end, both ways
    sides = w.label_rows()
    strain = ctr.SampleDataset(w.nf, *sides, embs=[w.table], samples=w.train)
    stest = ctr.SampleDataset(w.nf, *sides, embs=[w.table], samples=w.test)
    t0 = time.perf_counter()
    mtrain, mtest = strain.Materialise(), stest.Materialise()
    t_host_mat = time.perf_counter() - t0
    t_fit = {"padded": [], "samples": []}
    kw = dict(nFactors=d, nEpochs=args.epochs, batchSize=bs, lr=0.001, reg=0.0, optimizer=ctr.Adam, seed=1)
    for rep in range(args.fit_reps + 1):
        res = {}
        for name in ("padded", "samples"):
            m = ctr.FM(**kw)
            t0 = time.perf_counter()
            s = m.Fit(mtrain, mtest, Verbose=1) if name == "padded" else m.FitSamples(strain, stest, Verbose=1)
            if rep:
                t_fit[name].append(time.perf_counter() - t0)
            res[name] = (s, m.log(), m.params(), m.field_params(0))
        (sa, la, pa, fa), (sb, lb, pb, fb) = res["padded"], res["samples"]
        assert sa == sb and la == lb, "the two Fits differ: %r %r" % (la, lb)
        assert all(same_bits(x, y) for x, y in zip(pa, pb)) and all(same_bits(x, y) for x, y in zip(fa, fb)), "the Fits' parameters differ"
    say("D=%d: Fit %s" % (D, {k: stat(v) for k, v in t_fit.items()}))
    ep = {k: stat(v) for k, v in t_ep.items()}
    return dict(D=D, d=d, n_users=w.n_users, n_items=w.n_items, n_features=w.nf, train_rows=args.train, test_rows=args.rows,
                row_entries=2 + K_UL + K_IL, batch_size=bs, counts=counts, measured=True,
                host_materialise_numpy_s=t_mat, host_materialise_mirror_s=t_host_mat,
                setup_wall={k: stat(v) for k, v in t_set.items()},
                uploaded_bytes=dict(padded=up_padded, samples=up_samples), device_bytes_held=held,
                adam_epoch_wall=ep, evaluation_device={k: stat(v) for k, v in t_ev.items()},
                sample_epoch_median_within_or_below_padded_range=bool(ep["samples"]["median_ms"] <= ep["padded"]["max_ms"]),
                fit=dict(epochs=args.epochs, verbose=1, wall={k: stat(v) for k, v in t_fit.items()}, score_auc=res["padded"][0].AUC),
                costs_parameters_scores_bit_equal=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200000)
    ap.add_argument("--train", type=int, default=1000000)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fit-reps", type=int, default=5)
    ap.add_argument("--dims", type=int, nargs="+", default=[768, 1536])
    ap.add_argument("--out", default=os.path.join("profiles", "fm_samples_bench.json"))
    args = ap.parse_args()
    rng = np.random.default_rng(1)
    res = dict(method="median [min-max] of %d repetitions (Fit: %d) after a warm-up, the two routes alternating on the same data; "
                      "epoch = wall time of gorse_fm_epoch (it returns with the stream drained); evaluation = the device time "
                      "gorse_fm_evaluate_stats reports; uploaded bytes counted from the arrays handed over; device bytes = "
                      "hipMemGetInfo before minus after" % (args.reps, args.fit_reps),
               runs=[run(D, args, rng) for D in args.dims])
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
