"""Helpers and bars shared by the matrix-factorisation GPU parity tests (tests/test_gpu_cf_parity.py,
tests/test_gpu_cf_factor_widths.py).  Nothing here touches the device at import time."""
import numpy as np

from gorse_amd import capi, synth


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def report_elementwise(label, pairs):
    """prints, next to whichever bar the test applies, the PLAIN element-wise relative error |got - ref| / |ref| (max and the
    99.9th percentile over the elements with |ref| > 0): the figure "1e-4 relative" would mean with no floor at all"""
    for name, got, ref in pairs:
        got, ref = np.asarray(got, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
        nz = ref != 0
        rel = np.abs(got[nz] - ref[nz]) / np.abs(ref[nz])
        print("%s %s: element-wise relative error max %.2e, 99.9th percentile %.2e; max |error| / max |ref| %.2e"
              % (label, name, rel.max(), np.quantile(rel, 0.999), np.abs(got - ref).max() / np.abs(ref).max()))


ALS_RTOL, ALS_ATOL_ROW = 1e-4, 5e-5


def assert_als_close(got, ref, label=""):
    """The ALS bar, stated: |got - ref| <= 1e-4 |ref| + 5e-5 * (largest |ref| of the same row), element by element.
    "1e-4 relative"  on its own cannot hold for the elements that are differences of large terms: the
    rounding error of a row's d x d solve scales with the row, not with the element (the plain element-wise figure is
    printed by report_elementwise); the absolute term is therefore tied to the row's own scale and written down here."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    bound = ALS_RTOL * np.abs(ref) + ALS_ATOL_ROW * np.abs(ref).max(axis=1, keepdims=True)
    worst = float((np.abs(got - ref) / np.maximum(bound, 1e-300)).max())
    assert worst <= 1.0, "%s: |err| reaches %.2f x (1e-4 |ref| + 5e-5 rowmax|ref|)" % (label, worst)
    return worst


def als_half_fp64(A, B, ptr, idx, bptr, w, reg, rows):
    """The reference's user half-sweep (model.go:645-690) for the given rows of A in float64: the same recurrence, every sum
    in double precision -- the value both float32 forms (the reference's residual recurrence, the device's Gram form) round."""
    A = np.asarray(A, np.float64).copy()
    B = np.asarray(B, np.float64)
    d = A.shape[1]
    has = np.diff(bptr) > 0
    S = B[has].T @ B[has]
    for u in rows:
        fb = idx[ptr[u]:ptr[u + 1]]
        Bu = B[fb]
        pu = A[u]
        pred = Bu @ pu
        for f in range(d):
            q = Bu[:, f]
            res = pred - pu[f] * q
            a = ((1 - (1 - w) * res) * q).sum()
            c = ((1 - w) * q * q).sum()
            b = w * (pu @ S[:, f] - pu[f] * S[f, f])
            pu[f] = (a - b) / (c + w * S[f, f] + reg)
            pred = res + pu[f] * q
    return A[rows]


# What ONE grid of each capped matrix-factorisation launch holds before its kernel's grid-stride loop takes a second step.  The tests of
# tests/test_gpu_cf_past_one_grid.py size their inputs from these literals; tests/test_mf_grid_caps_cpu.py holds every one of them
# against the launcher's own text, so a cap raised later fails a test instead of leaving the strided iterations unvisited again.
GRID_USER_RUNS = 65_536       # bpr_launch_update_users (bpr_plan.hpp bpr_user_run_workers): 256 * 16 workgroups x 16 groups, one user run each (nFactors 8: two per group)
GRID_USER_RUNS_D8 = 131_072
GRID_SAMPLES = 65_536         # launch_update_mode (bpr_plan.hpp bpr_sample_workers): 256 * 16 workgroups x 16 groups, one sample each
GRID_SCORE_PAIRS = 131_072    # mf_score_device: 256 * 32 workgroups x 16 groups, one pair each
GRID_RANK_LISTS = 4_096       # mf_rank_device: expand_users_kernel, one workgroup per list
GRID_DELTA_FLOATS = 2_097_152  # mf_delta_export_async / _import_async: 2048 workgroups x 256 threads x one float4
GRID_SORT_SAMPLES = 524_288   # launch_user_sort (bpr_rank_kernel, bpr_scatter_by_kernel): 256 * 8 workgroups x 256 threads
GRID_FOLD_ELEMENTS = 131_072  # bpr_fold_kernel behind a per-sample launch: 512 workgroups x 256 threads, one row element each
SCAN_ONE_WORKGROUP = 32_768   # exclusive_scan_i32: up to 16 tiles of 2048 counters by scan_small_kernel, three kernels beyond


def rel_err(a, b):
    """Largest element error relative to max(|reference element|, rms of the reference matrix):
    plain element-wise relative error, except that elements far below the matrix scale are
    measured against that scale (their relative error is pure cancellation noise)."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    floor = max(float(np.sqrt(np.mean(b * b))), 1e-12)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), floor)))


def make_mf(data, d, seed=3, std=0.1, with_items=True):
    mf = capi.MF(data.U, data.I, d, data.uptr, data.uidx, data.iptr if with_items else None,
                 data.iidx if with_items else None)
    P, Q = synth.init_factors(data.U, data.I, d, 0.0, std, seed)
    mf.set_factors(P, Q)
    return mf, P, Q
