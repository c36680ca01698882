"""Wall-clock time of gorse_fm_epoch at 1M features x nFactors 16 (17.0M parameters), 1M rows of width 8, batch 1024 = 977
steps: `epochs` epochs with Adam, then with SGD.  The first epoch of a training set also sorts the batches' (feature, position)
lists.  Under `rocprofv3 --kernel-trace --stats -- python scripts/gpu_fm_epoch_time.py 1` it gives the per-kernel times of
DESIGN.md section 4 ("Factorization machine").  A second argument D > 0 adds one item-embedding field of that dimension
(n x D bf16 on the device: 1.5 GB at D = 768, 3.1 GB at 1536), which runs the attention branch in every step.  The rows'
embeddings are drawn from a pool of 4096 normal vectors (a million distinct draws cost more host time than the epochs)."""
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
D = int(sys.argv[2]) if len(sys.argv) > 2 else 0
fm = capi.FM(nf, d, embedding_dims=(D,) if D else None)
fm.set_params(0.0, rng.normal(0, 0.01, nf).astype(np.float32), rng.normal(0, 0.01, (nf, d)).astype(np.float32))
fm.set_train(idx, val, tgt)
if D:
    b = 1 / np.sqrt(D)
    fm.set_embedding_params(0, rng.normal(0, 0.01, (d, D)), rng.uniform(-b, b, (D, d)), np.zeros(d), rng.uniform(-b, b, (D, d)),
                            np.zeros(d))
    pool = rng.normal(0, 1, (4096, D)).astype(np.float32).view(np.uint32)
    pool = ((pool + 0x7FFF + ((pool >> 16) & 1)) >> 16).astype(np.uint16)  # bf16, round to nearest even
    fm.set_train_embeddings(0, pool[rng.integers(0, 4096, n)])
for opt in (capi.OPT_ADAM, capi.OPT_SGD):
    for e in range(epochs):
        t = time.perf_counter()
        c = fm.epoch(1024, opt, 0.01, 1e-4)
        print("opt %d epoch %d: %.2f ms cost %.4f" % (opt, e, (time.perf_counter() - t) * 1e3, c), flush=True)
print("steps/epoch", -(-n // 1024), "params", nf * (d + 1) + 1, "embedding dim", D)
