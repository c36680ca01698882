#!/usr/bin/env python3
"""C4 (1M x 128 bf16, cosine, k = 100) on the device: the all-pairs pass with its stage times, a few rows checked against the
oracle, and the switches of the tie path (row slices of the history sweep, the replay's shortcut).  usage: gpu_probe_topk_c4.py [n_queries]"""
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from gorse_amd import capi, synth  # noqa: E402
from oracle import oracle as orc  # noqa: E402


def run(t, k, q0, q1, label, reps=2):
    t.all_pairs(k, q0, q1, fetch=False)
    t.synchronize()
    classes = (capi.PROF_TOPK_SWEEP, capi.PROF_TOPK_SELECT, capi.PROF_TOPK_HIST, capi.PROF_TOPK_REPLAY)
    t.set_profiling(True)
    before = [t.get_profile(c) for c in classes]  # the counters are cumulative
    t0 = time.perf_counter()
    for _ in range(reps):
        t.all_pairs(k, q0, q1, fetch=False)
    t.synchronize()
    dt = (time.perf_counter() - t0) / reps
    stages = [(a[0] - b[0], a[1] - b[1]) for a, b in zip([t.get_profile(c) for c in classes], before)]
    t.set_profiling(False)
    n_fb, n_tie = t.last_stats()
    print("%-34s %8.2f ms per pass | sweep %.2f rescore %.2f history %.2f replay %.2f ms | tie queries %d, to the scan %d"
          % (label, dt * 1e3, *(ms / max(reps, 1) for _, ms in stages), n_tie, n_fb), flush=True)


def main():
    nq = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 1_000_000
    N, d, k = 1_000_000, 128, 100
    Xb, Xe = synth.s_emb(N, d, 44)
    t = capi.TopK(Xb, capi.METRIC_COSINE, dtype=capi.DTYPE_BF16)
    L = capi.lib()
    run(t, k, 0, nq, "default")
    # parity of a few rows (the GPU tests and bench.py check more)
    o = orc.Oracle()
    o.set_isa(orc.ISA_AVX512)
    idx, dist = t.all_pairs(k, 500_000, 500_016)
    for r in range(16):
        ei, ed = o.search_index(Xe, orc.METRIC_COSINE, 500_000 + r, k)
        assert np.array_equal(idx[r], ei) and np.array_equal(dist[r].view(np.uint32), ed.view(np.uint32)), r
    print("16 rows equal the oracle's", flush=True)
    if "quick" in sys.argv[1:]:
        return
    if "sym" in sys.argv[1:]:  # the symmetric form of the sweep against the square one: stage times, then EVERY row of both passes
        SYM_OFF = capi.TOPK_SYM_OFF
        for rep in range(2):
            for v, label in ((0, "symmetric sweep (default)"), (SYM_OFF, "square sweep (TOPK_SYM_OFF)")):
                L.gorse_hip_test_set_topk_variant(v)
                run(t, k, 0, nq, label, reps=2)
                print("   main sweep symmetric: %s" % t.last_symmetric(), flush=True)
        L.gorse_hip_test_set_topk_variant(0)
        i_sy, d_sy = t.all_pairs(k, 0, nq)
        st = t.last_stats()
        print("symmetric: tie queries %d, to the scan %d, warm starts swept again %d" % (st[1], st[0], t.resweeps()), flush=True)
        L.gorse_hip_test_set_topk_variant(SYM_OFF)
        i_sq, d_sq = t.all_pairs(k, 0, nq)
        st = t.last_stats()
        print("square:    tie queries %d, to the scan %d, warm starts swept again %d" % (st[1], st[0], t.resweeps()), flush=True)
        L.gorse_hip_test_set_topk_variant(0)
        same_i = np.array_equal(i_sy, i_sq)
        same_d = np.array_equal(d_sy.view(np.uint32), d_sq.view(np.uint32))
        print("all %d rows of the two passes equal: indices %s, distance bits %s" % (nq, same_i, same_d), flush=True)
        if not (same_i and same_d):
            bad = np.argwhere((i_sy != i_sq).any(1) | (d_sy.view(np.uint32) != d_sq.view(np.uint32)).any(1)).ravel()
            print("  %d rows differ, first: %s" % (bad.size, bad[:20]), flush=True)
            for q in bad[:3]:
                ei, ed = o.search_index(Xe, orc.METRIC_COSINE, int(q), k)
                print("  row %d: symmetric equals the oracle %s, square equals the oracle %s" % (q, np.array_equal(i_sy[q], ei), np.array_equal(i_sq[q], ei)))
        # a query range inside the index (what a rank of a sharded refresh runs): symmetric only inside its own square
        for (a, b) in ((250_112, 500_096), (0, 131_072)):
            L.gorse_hip_test_set_topk_variant(0)
            i1, d1 = t.all_pairs(k, a, b)
            sym = t.last_symmetric()
            print("   range [%d, %d) symmetric %s: equal to the full pass's rows: %s" % (a, b, sym, np.array_equal(i1, i_sq[a:b]) and
                  np.array_equal(d1.view(np.uint32), d_sq[a:b].view(np.uint32))), flush=True)
            run(t, k, a, b, "range [%d, %d) symmetric" % (a, b), reps=2)
            L.gorse_hip_test_set_topk_variant(SYM_OFF)
            run(t, k, a, b, "range [%d, %d) square" % (a, b), reps=2)
        L.gorse_hip_test_set_topk_variant(0)
        return
    if "replay" in sys.argv[1:]:  # the tie replay's counters
        L.gorse_hip_test_set_topk_variant(capi.TOPK_REPLAY_COUNTERS)
        run(t, k, 0, nq, "instrumented", reps=1)
        c = t.sweep_profile()
        q = max(c[3], 1)
        print("  replay: %d queries, ticks per query mean %.0f max %d; entries mean %.0f max %d; pushes %.0f, T^gap calls %.0f of which not the identity %.0f, literal T %.0f (max %d) per query; undecided %d"
              % (c[3], c[0] / q, c[1], c[2] / q, c[9], c[4] / q, c[5] / q, c[6] / q, c[7] / q, c[8], c[10]), flush=True)
        L.gorse_hip_test_set_topk_variant(0)
        return
    if "lanes" in sys.argv[1:]:  # the tie replay: queries per wave chosen by the launch's size (default) against always 64
        for v, label in ((0, "queries per replay wave by launch size"), (capi.TOPK_REPLAY_WAVE64, "64 queries per replay wave"),
                         (0, "by launch size again"), (capi.TOPK_REPLAY_WAVE64, "64 again")):
            L.gorse_hip_test_set_topk_variant(v)
            run(t, k, 0, nq, label, reps=2)
        L.gorse_hip_test_set_topk_variant(0)
        return
    if "warm" in sys.argv[1:]:  # round 6: the history sweep's slices started from the bounds the main sweep's lists prove (default) against cold
        COLD = capi.TOPK_COLD_SLICES
        for rep in range(2):
            for v, label in ((0, "history slices warm (default)"), (COLD, "history slices cold (TOPK_COLD_SLICES)")):
                L.gorse_hip_test_set_topk_variant(v)
                run(t, k, 0, nq, label, reps=2)
        L.gorse_hip_test_set_topk_variant(0)
        i_a, d_a = t.all_pairs(k, 0, nq)
        st_a = t.last_stats()
        L.gorse_hip_test_set_topk_variant(COLD)
        i_b, d_b = t.all_pairs(k, 0, nq)
        st_b = t.last_stats()
        L.gorse_hip_test_set_topk_variant(0)
        same = np.array_equal(i_a, i_b) and np.array_equal(d_a.view(np.uint32), d_b.view(np.uint32))
        print("warm: tie queries %d, to the scan %d; cold: %d, %d" % (st_a[1], st_a[0], st_b[1], st_b[0]), flush=True)
        print("all %d rows with warm-started history slices equal the cold form's: %s" % (nq, same), flush=True)
        assert same
        return
    for v, label in ((capi.TOPK_SLICE1, "history sweep in one slice"), (capi.TOPK_WARM_OFF, "no warm start"), (capi.TOPK_COARSE_OFF, "no block-level scale bound")):
        L.gorse_hip_test_set_topk_variant(v)
        run(t, k, 0, nq, label, reps=1)
    L.gorse_hip_test_set_topk_variant(0)


if __name__ == "__main__":
    main()
