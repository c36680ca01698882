"""Wall-clock time of gorse_fm_epoch at 1M features x nFactors 16 (17.0M parameters), 1M rows of width 8, batch 1024 = 977
steps: `epochs` epochs with Adam, then with SGD.  The first epoch of a training set also sorts the batches' (feature, position)
lists.  Under `rocprofv3 --kernel-trace --stats -- python scripts/gpu_fm_epoch_time.py 1` it gives the per-kernel times of
DESIGN.md section 4 ("Factorization machine")."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from gorse_amd import capi  # noqa: E402

nf, d, n, w = 1_000_000, 16, 1_000_000, 8
epochs = int(sys.argv[1]) if len(sys.argv) > 1 else 3
rng = np.random.default_rng(0)
idx = rng.integers(0, nf, (n, w), dtype=np.int32)
val = np.ones((n, w), np.float32)
tgt = np.where(rng.random(n) < 0.5, 1, -1).astype(np.float32)
fm = capi.FM(nf, d)
fm.set_params(0.0, rng.normal(0, 0.01, nf).astype(np.float32), rng.normal(0, 0.01, (nf, d)).astype(np.float32))
fm.set_train(idx, val, tgt)
for opt in (capi.OPT_ADAM, capi.OPT_SGD):
    for e in range(epochs):
        t = time.perf_counter()
        c = fm.epoch(1024, opt, 0.01, 1e-4)
        print("opt %d epoch %d: %.2f ms cost %.4f" % (opt, e, (time.perf_counter() - t) * 1e3, c), flush=True)
print("steps/epoch", -(-n // 1024), "params", nf * (d + 1) + 1)
