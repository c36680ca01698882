"""Shapes and inputs of the exact top-k's depth and wide-row tests (tests/test_gpu_topk_depths.py, tests/test_gpu_topk_wide_rows.py),
kept apart from the GPU modules so that tests/test_topk_depth_table_cpu.py can hold the tables against the kernels' sources, and
so that the inputs can be examined with the oracle alone.

Path B (csrc/topk_mfma.hip) instantiates its sweep per operand depth KP: ceil(d / 16) k-steps for a bf16 index, ceil(3 d / 16) for an
fp32 index (hi | lo | hi split), rounded up to the next supported depth.  Path A (csrc/topk.hip) takes 16, 8, 4, 2 or 1 sixteen-lane
groups per workgroup as the row width grows (scan_groups)."""
import numpy as np

from gorse_amd import capi

F32, BF16 = capi.DTYPE_F32, capi.DTYPE_BF16
SUPPORTED_KP = (1, 2, 3, 4, 6, 8, 12, 16, 24)  # kSupportedKP of csrc/topk_mfma.hip (test_topk_depth_table_cpu.py compares)
METRICS = (capi.METRIC_NEG_DOT, capi.METRIC_COSINE, capi.METRIC_EUCLIDEAN)


def expected_kp(dtype, d):
    """topk_mfma_prepare: the operand depth of an index, None when it is too deep for path B"""
    need = -(-(d if dtype == BF16 else 3 * d) // 16)
    return next((c for c in SUPPORTED_KP if c >= need), None)


def operand_form(dtype, d):
    """'aliased': a bf16 index of d == 16 KP is its own operand matrix; 'full': split fp32 operands without a pad column;
    'padded': pad_bf16_kernel / split_f32_kernel leave zero columns behind the row"""
    kp = expected_kp(dtype, d)
    if dtype == BF16:
        return "aliased" if d == 16 * kp else "padded"
    return "full" if 3 * d == 16 * kp else "padded"


# (dtype, d): every supported depth in both dtypes; bf16 in the aliased and in the padded form at the depths that are a row width;
# the padded rows are the narrowest of their depth, so that the most k-steps are zeros
DEPTH_CASES = (
    (BF16, 16), (BF16, 9), (F32, 5),                          # KP 1
    (BF16, 32), (BF16, 17), (F32, 10),                        # KP 2
    (BF16, 48), (BF16, 33), (F32, 16),                        # KP 3
    (BF16, 64), (BF16, 49), (F32, 21),                        # KP 4
    (BF16, 96), (BF16, 65), (F32, 32), (F32, 22),             # KP 6
    (BF16, 97), (F32, 33),                                    # KP 8
    (BF16, 192), (BF16, 129), (F32, 43),                      # KP 12
    (BF16, 256), (BF16, 193), (F32, 85), (F32, 65),           # KP 16
    (BF16, 384), (BF16, 257), (F32, 86),                      # KP 24
)
DEPTH_N, DEPTH_K = 2500, 25
# (dtype, d, metric, k) -> which seed of the case's series is used (0 where not listed): the first one with which no sampled query of
# the three calls has two equal distances among its k + 1 best in the reference's own arithmetic (found and checked with the oracle
# alone; fp32 distances of Gaussian rows collide by chance, the Euclidean ones of wide rows at k = 100 most often)
DEPTH_SEED_TRY = {
    (F32, 33, 1, 25): 1,
    (BF16, 48, 1, 25): 1,
    (BF16, 49, 1, 25): 1,
    (BF16, 64, 1, 25): 1,
    (BF16, 64, 2, 25): 1,
    (F32, 85, 1, 100): 39,
    (F32, 86, 1, 25): 2,
    (BF16, 97, 1, 25): 1,
    (BF16, 97, 2, 25): 1,
    (BF16, 129, 1, 25): 2,
    (BF16, 129, 2, 25): 1,
    (BF16, 192, 0, 100): 1,
    (BF16, 192, 1, 25): 5,
    (BF16, 192, 1, 100): 67,
    (BF16, 192, 2, 100): 5,
    (BF16, 256, 1, 25): 2,
    (BF16, 257, 1, 100): 3202,
    (BF16, 257, 2, 100): 7,
    (BF16, 384, 1, 25): 1,
}
DEPTH_K100 = ((BF16, 192), (F32, 85), (BF16, 257))  # one case per KP >= 12 also with k = 100
# the tie path (history sweep + heap replay) at the depths whose history sweep is not the main sweep's LDS-DMA form
TIE_CASES = ((BF16, 48), (F32, 22), (BF16, 129), (F32, 85), (BF16, 384))
# the 64-row-tile variant of the register-staged main sweep (RB = 2) at KP 3 and KP 6
TILE64_CASES = ((BF16, 33), (F32, 32))
# one column past KP 24: no path B
TOO_DEEP_CASES = ((BF16, 385), (F32, 129))

# Path A.  Both sides of every edge of scan_groups ((1 + g) * d * 4 <= 144 KB), the widths users configure, 16-chunk tails with an
# 8-tail and a scalar tail (d % 16 in 9..15), the same tails without a full chunk or with one
WIDE_WIDTHS = (1024, 1536, 2168, 2169, 3072, 4096, 4097, 7372, 7373, 12288, 12289, 16384, 1031, 1033, 1039, 9, 15, 17, 31)
WIDE_BF16_ORDER_WIDTHS = (1024, 7373, 16384)  # METRIC_EUCLIDEAN_BF16: 16, 2 and 1 sixteen-lane groups
TOPK_MAX_DIM = 16384
SCAN_LDS_BYTES = 144 * 1024


def scan_groups(d):
    """csrc/topk.hip scan_groups restated"""
    g = 16
    while g > 1 and (1 + g) * d * 4 > SCAN_LDS_BYTES:
        g >>= 1
    return g


def to_bf16(Xf):
    return (np.ascontiguousarray(Xf, np.float32).view(np.uint32) >> 16).astype(np.uint16)


def from_bf16(Xb):
    return (Xb.astype(np.uint32) << 16).view(np.float32)


def as_index(Xf, dtype):
    """(what the handle is given, the same rows as the fp32 values the reference computes with)"""
    if dtype == BF16:
        X = to_bf16(Xf)
        return X, from_bf16(X)
    Xf = np.ascontiguousarray(Xf, np.float32)
    return Xf, Xf


def depth_inputs(dtype, d, metric, k=DEPTH_K, N=DEPTH_N):
    """Gaussian rows with skewed norms (the -dot bound uses the largest norm), an unordered query list with repeats and 70 query
    vectors: (X, Xe, qs, qv, qe)"""
    rng = np.random.default_rng(7000 + 1000 * d + 10 * metric + dtype + 1_000_000 * DEPTH_SEED_TRY.get((dtype, d, metric, k), 0))
    Xf = rng.standard_normal((N, d)).astype(np.float32)
    Xf *= rng.uniform(0.2, 3.0, (N, 1)).astype(np.float32)
    X, Xe = as_index(Xf, dtype)
    qs = np.concatenate([rng.integers(0, N, 150), [5, 5, N - 1, 0]]).astype(np.int64)
    qv, qe = as_index(rng.standard_normal((70, d)).astype(np.float32), dtype)
    return X, Xe, qs, qv, qe


DEPTH_SAMPLE = 9  # every 9th row of a call is compared with the oracle
