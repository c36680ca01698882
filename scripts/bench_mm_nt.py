#!/usr/bin/env python
"""Times floats.MM's NT case (C = A B^T in floats.Dot's bits) as tiles on the matrix cores (csrc/sgemm_nt.hip sgemm_nt_mfma_kernel,
gorse_hip_test_set_sgemm_nt mode 2) against the one-dot-per-element kernels it replaces for large results (mode 1: sgemm_nt_kernel /
sgemm_nt_long_kernel, unchanged, the baseline).

Per shape: operands resident on the device, one warm-up call per mode, then --reps repetitions with the modes alternating; the time is
the kernel's own (gorse_hip_test_sgemm_last_ms: events around the launch), for shapes under 1 GFLOP the mean of ten calls per
repetition.  Median [min-max].  The two results must be equal in every bit in every repetition, or the script fails.  TFLOP/s counts
2 m n k; the fraction of peak is against the 157.3 TFLOP/s of the fp32 MFMA (the NN kernel reaches 0.72-0.74 of it at 4096^3).
Writes one JSON file."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gorse_amd import capi  # noqa: E402

PEAK_TFLOPS = 157.3
SHAPES = [("4096^3, the twin of the NN headline", 4096, 4096, 4096), ("short k", 8192, 8192, 64), ("long k", 1024, 1024, 8192),
          ("the threshold of the automatic rule", 512, 512, 64)]
MODES = {1: ("per_element", lambda k: capi.SGEMM_NT | (capi.SGEMM_NT_LONG if k > 512 else 0)),
         2: ("mfma_tiles", lambda k: capi.SGEMM_NT | capi.SGEMM_NT_MFMA)}


def stat(ts, flops):
    ts = sorted(ts)
    med = ts[len(ts) // 2]
    return dict(median_ms=med, min_ms=ts[0], max_ms=ts[-1], tflops=flops / (med * 1e9))


def shape_leg(L, what, m, n, k, reps, pad=0):
    """pad: floats past k in every row of A and B (the leading dimension is k + pad)"""
    g = torch.Generator(device="cuda").manual_seed(m + n + k)
    a = torch.randn(m, k + pad, device="cuda", generator=g)
    b = torch.randn(n, k + pad, device="cuda", generator=g)
    c = {mode: torch.full((m, n), float("nan"), device="cuda") for mode in MODES}
    flops = 2.0 * m * n * k
    inner = 10 if flops < 1e9 else 1

    def once(mode):
        L.gorse_hip_test_set_sgemm_nt(mode)
        ms = 0.0
        for _ in range(inner):
            capi.sgemm_device(0, 1, m, n, k, a.data_ptr(), k + pad, b.data_ptr(), k + pad, c[mode].data_ptr(), n)
            assert L.gorse_hip_test_sgemm_last_form() == MODES[mode][1](k), (mode, L.gorse_hip_test_sgemm_last_form())
            ms += L.gorse_hip_test_sgemm_last_ms()
        return ms / inner

    times = {mode: [] for mode in MODES}
    for rep in range(-1, reps):  # (-1: the warm-up)
        for mode in MODES:
            t = once(mode)
            if rep >= 0:
                times[mode].append(t)
        assert torch.equal(c[1].view(torch.int32), c[2].view(torch.int32)), "the two forms differ at %s" % what
        for t in c.values():
            t.fill_(float("nan"))
    out = {MODES[mode][0]: stat(times[mode], flops) for mode in MODES}
    new, old = out["mfma_tiles"], out["per_element"]
    return dict(shape=what, m=m, n=n, k=k, lda=k + pad, ldb=k + pad, calls_per_repetition=inner, bits_equal=True, **out,
                speedup=old["median_ms"] / new["median_ms"], mfma_tiles_fraction_of_fp32_mfma_peak=new["tflops"] / PEAK_TFLOPS,
                ranges_disjoint=new["max_ms"] < old["min_ms"] or old["max_ms"] < new["min_ms"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "mm_nt_bench.json"))
    args = ap.parse_args()
    assert capi.device_count() >= 1, "no MI355X visible"
    L = capi.lib()
    try:
        legs = [shape_leg(L, *s, args.reps) for s in SHAPES]
        # rows 16 KB apart (k = 4096, 8192) against rows 32 floats further apart: the same work, other addresses
        legs += [shape_leg(L, what + ", leading dimensions k + 32", m, n, k, args.reps, 32) for what, m, n, k in SHAPES[:1] + SHAPES[2:3]]
    finally:
        L.gorse_hip_test_set_sgemm_nt(0)
    res = dict(method="median [min-max] of %d repetitions after a warm-up, hook modes 1 and 2 alternating on resident operands, kernel "
                      "time from events around the launch; every repetition's two results compared bit for bit" % args.reps,
               peak_tflops_fp32_mfma=PEAK_TFLOPS, nn_kernel_fraction_of_peak="0.72-0.74 (README, bench.py mm)", shapes=legs)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
