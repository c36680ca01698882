#!/usr/bin/env python3
"""Generate tests/golden/ref_live_vectors.npz: the reference's own dot / euclidean kernels (AVX and AVX512) on the
seeded vectors of tests/test_oracle_golden.py::test_bit_equal_to_live_reference_kernels, inputs + outputs.

Needs oracle/_ref/libgorse_ref.so (oracle/Makefile `ref`) and an AVX512 host; the test then checks the oracle against
these recorded outputs on hosts without them, and against the live kernels (and this file) where they exist.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import oracle as orc  # noqa: E402

orc.build(force=False)
ref = orc.load_ref()
assert ref is not None, "needs oracle/_ref/libgorse_ref.so and an AVX512 host"

rng = np.random.default_rng(7)
sizes = list(range(1, 140)) + [255, 256, 257]
A, B = [], []
res = {k: [] for k in ("dot256", "dot512", "euc256", "euc512")}
for n in sizes:
    a = rng.standard_normal(n).astype(np.float32)
    b = rng.standard_normal(n).astype(np.float32)
    A.append(a)
    B.append(b)
    for isa, tag in ((orc.ISA_AVX, "256"), (orc.ISA_AVX512, "512")):
        res["dot" + tag].append(ref.dot(isa, a, b))
        res["euc" + tag].append(ref.euclidean(isa, a, b))
out = {"sizes": np.array(sizes, np.int64), "a": np.concatenate(A), "b": np.concatenate(B)}
out.update({k: np.array(v, np.float32) for k, v in res.items()})
path = os.path.join(ROOT, "tests", "golden", "ref_live_vectors.npz")
np.savez_compressed(path, **out)
print("wrote", path, os.path.getsize(path), "bytes")
