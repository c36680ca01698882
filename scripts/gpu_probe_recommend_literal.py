#!/usr/bin/env python3
"""One gorse_mf_recommend call per literal mode on one handle, the C3 shard's first 8192 users, nFactors 128, k 100 (after a warm-up
call of each): the command a kernel trace of the literal path profiles
(rocprofv3 --kernel-trace --stats -- python scripts/gpu_probe_recommend_literal.py [schedule])."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gorse_amd import capi, synth  # noqa: E402

schedule = int(sys.argv[1]) if len(sys.argv) > 1 else 0
data = synth.s_big_shard(0, 8)
P, Q = synth.init_factors(data.U, data.I, 128, 0.0, 0.1, 1)
mf = capi.MF(data.U, data.I, 128, np.asarray(data.uptr), np.asarray(data.uidx))
mf.set_factors(P, Q)
mf.set_recommend_schedule(schedule)
ok = np.ones(data.I, np.uint8)
rows = {}
for rep in range(2):
    for mode in (0, 1):
        mf.set_recommend_literal(mode)
        rows[mode] = mf.recommend(8192, 100, ok)
        print("rep", rep, "mode", mode, "stats", mf.recommend_stats(), "literal", mf.recommend_literal_stats(), flush=True)
assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(rows[0], rows[1]))
