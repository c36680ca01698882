"""Probe of the accumulated tier's fold interval (csrc/bpr_fold.hpp kDefaultAccFoldEvery) on S-ml1m: for nFactors 8 / 16 / 64 and the tier
off / folded every 2 / 4 / 8 fold periods -- device milliseconds per epoch (15 epochs enqueued back to back, after 3) and NDCG@10 after
30 epochs of the production mode on three sampler seeds (the fixtures of tests/test_gpu_bpr_positive_series.py; the sequential oracle's
figures for the same streams are printed by tests/test_gpu_bpr_acc_rows.py).  usage: python scripts/gpu_probe_bpr_acc_rows.py [out.txt]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gorse_amd import capi, synth  # noqa: E402
from oracle import oracle as orc  # noqa: E402


def main():
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()

    L = capi.lib()
    o = orc.Oracle()
    o.set_exp(0)
    L.gorse_hip_test_set_exact_exp(0)
    data = synth.s_ml1m()
    lr, reg, epochs = 0.05, 0.01, 30
    say("S-ml1m, lr %g reg %g; ms = device time per epoch (15 enqueued, after 3); NDCG@10 after %d epochs, seeds 2024 / 7 / 99" % (lr, reg, epochs))
    say("%8s %6s %9s %9s  %s" % ("nFactors", "tier", "ms/epoch", "NDCG mean", "NDCG per seed, finite"))
    for d in (8, 16, 64):
        P0, Q0 = synth.init_factors(data.U, data.I, d, 0.0, 0.001, 1)
        for every in (0, 2, 4, 8):
            L.gorse_hip_test_set_bpr_acc_rows(1 if every else 0)
            L.gorse_hip_test_set_bpr_acc_fold_every(every)
            try:
                got, fin, ms = [], True, None
                for seed in (2024, 7, 99):
                    mf = capi.MF(data.U, data.I, d, data.uptr, data.uidx)
                    mf.set_factors(P0, Q0)
                    if ms is None:
                        for ep in range(1, 4):
                            mf.bpr_epoch_enqueue(data.n_train, lr, reg, seed, 100 + ep)
                        mf.synchronize()
                        mf.epoch_times(reset=True)
                        for ep in range(4, 19):
                            mf.bpr_epoch_enqueue(data.n_train, lr, reg, seed, 100 + ep)
                        mf.synchronize()
                        n, tot, _ = mf.epoch_times()
                        ms = tot / max(n, 1)
                        mf.set_factors(P0, Q0)
                    for ep in range(1, epochs + 1):
                        mf.bpr_epoch(data.n_train, lr, reg, seed, ep, mode=capi.BPR_HOGWILD_STORES)
                    gP, gQ = mf.get_factors()
                    mf.close()
                    fin = fin and bool(np.isfinite(gP).all() and np.isfinite(gQ).all())
                    got.append(float(o.evaluate(gP, gQ, data.test_ptr, data.test_idx, data.neg_ptr, data.neg_idx, 10)[0]) if fin else float("nan"))
                say("%8d %6s %9.4f %9.4f  %s %s" % (d, "off" if not every else "k=%d" % every, ms, float(np.mean(got)),
                                                  " ".join("%.4f" % g for g in got), fin))
            finally:
                L.gorse_hip_test_set_bpr_acc_rows(-1)
                L.gorse_hip_test_set_bpr_acc_fold_every(0)


if __name__ == "__main__":
    main()
