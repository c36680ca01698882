"""Shapes and inputs of the exact top-k's depth and wide-row tests (tests/test_gpu_topk_depths.py, tests/test_gpu_topk_wide_rows.py),
kept apart from the GPU modules so that tests/test_topk_depth_table_cpu.py can hold the tables against the kernels' sources, and
so that the inputs can be examined with the oracle alone.

Path B (csrc/topk_mfma.hip; the sweep: csrc/topk_sweep.hip) instantiates its sweep per operand depth KP: ceil(d / 16) k-steps for a bf16 index, ceil(3 d / 16) for an
fp32 index (hi | lo | hi split), rounded up to the next supported depth.  Path A (csrc/topk.hip) takes 16, 8, 4, 2 or 1 sixteen-lane
groups per workgroup as the row width grows (scan_groups)."""
import numpy as np

from gorse_amd import capi

F32, BF16 = capi.DTYPE_F32, capi.DTYPE_BF16
SUPPORTED_KP = (1, 2, 3, 4, 6, 8, 12, 16, 24)  # kSupportedKP of csrc/topk_plan.hpp (test_topk_depth_table_cpu.py compares)
METRICS = (capi.METRIC_NEG_DOT, capi.METRIC_COSINE, capi.METRIC_EUCLIDEAN)


def expected_kp(dtype, d):
    """topk_mfma_prepare (operand_depth of csrc/topk_plan.hpp): the operand depth of an index, None when it is too deep for path B"""
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


# ---- the scan's selection (csrc/topk.hip select_fast_kernel): tests/test_gpu_topk_scan_select.py, examined by
# tests/test_topk_scan_cases_cpu.py ----
# 1024 threads stride a query's row of distances and keep their 4 smallest keys each; the (k + 1)-th smallest kept key bounds the
# true (k + 1)-th smallest from above; the rows up to that bound are collected into 2048 slots, sorted and checked for ties.  A
# NaN, k + 1 > 1024 or more than 2048 rows at the bound leave the query to the literal kernel.
SEL_THREADS, SEL_KEEP, SEL_CAP = 1024, 4, 2048
SEL_D = 4
SEL_Q = np.array([1.0, 2.0, -1.0, 0.5], np.float32)  # |q|^2 = 6.25: the -dot distances of its multiples are exact
SEL_KS = (5, 20)
SEL_STRIDE_AT = 5  # the planted rows of the one-stride cases sit at indices = 5 (mod 1024)
NEG_DOT, EUCLIDEAN, COSINE = capi.METRIC_NEG_DOT, capi.METRIC_EUCLIDEAN, capi.METRIC_COSINE


def sel_queries():
    """the query direction and two vectors within 1e-3 of it (the planted rows keep their order)"""
    rng = np.random.default_rng(515)
    return np.stack([SEL_Q, SEL_Q + rng.uniform(-1e-3, 1e-3, SEL_D).astype(np.float32),
                     SEL_Q + rng.uniform(-1e-3, 1e-3, SEL_D).astype(np.float32)]).astype(np.float32)


def sel_planted(metric, n):
    """n rows with pairwise distinct distances to SEL_Q, every one far better than a background or plateau row: -dot = distinct
    positive multiples of the query direction, Euclidean = the query plus distinct offsets, cosine = distinct small rotations"""
    P = np.tile(SEL_Q, (n, 1)).astype(np.float32)
    j = np.arange(n, dtype=np.float32)
    if metric == NEG_DOT:
        P *= (3.0 + j)[:, None]
    elif metric == EUCLIDEAN:
        P[:, 0] += (j + 1.0) / 64.0
    else:
        th = (j + 1.0) * 0.01
        P[:, 0] = SEL_Q[0] * np.cos(th) - SEL_Q[1] * np.sin(th)
        P[:, 1] = SEL_Q[0] * np.sin(th) + SEL_Q[1] * np.cos(th)
    return np.ascontiguousarray(P, np.float32)


def sel_rows(k):
    return (k + 8) * SEL_THREADS + 6


def _plant(X, metric, k, one_stride, seed):
    n = k + 6
    at = SEL_STRIDE_AT + SEL_THREADS * np.arange(n) if one_stride else np.arange(n)
    at = np.random.default_rng(seed).permutation(at)  # the ranks in no order of the indices
    X[at] = sel_planted(metric, n)
    return np.sort(at).astype(np.int64)


def concentrated_case(metric, k):
    """(X, planted ids): Gaussian background rows around -4 q -- a positive -dot, a cosine distance above 1, a Euclidean distance
    of 5 |q| or so -- and the k + 6 best rows in ONE thread's stride: that thread keeps 4 of them, so the bound comes from the
    other threads' background rows and the second pass must fetch planted rows no thread kept"""
    N = sel_rows(k)
    rng = np.random.default_rng(9000 + 10 * k + metric)
    X = (rng.standard_normal((N, SEL_D)) - 4.0 * SEL_Q).astype(np.float32)
    return X, _plant(X, metric, k, True, 77 + k)


def plateau_row(metric):
    return -SEL_Q if metric == COSINE else np.zeros(SEL_D, np.float32)


def plateau_case(metric, k, variant):
    """(X, planted ids): the planted rows, every other row ONE row (more than 2048 of them).  Variant 'A': planted in one stride --
    the bound lands on the plateau, the collection overflows its 2048 slots, the query goes literal.  Variant 'B': planted at
    0 .. k + 5, one per stride -- the bound is the exact (k + 1)-th smallest and the fast kernel answers."""
    N = sel_rows(k)
    X = np.tile(plateau_row(metric), (N, 1)).astype(np.float32)
    return X, _plant(X, metric, k, variant == "A", 78 + k)


def signed_zero_cases():
    """-dot of an orthogonal pair is -0.0 (logics/cf.go:33).  (X6, query vector, k) and (X40, query index, k): in both the query
    (1, 0, 0, 0) has exactly one orthogonal row among its k best and pairwise distinct distances among its k + 1 best; every value
    is a bf16 value"""
    X6 = np.array([[0, 1, 2, 3], [1, 0, 0, 0], [2, 1, 1, 1], [-1, 5, 5, 5], [3, 0, 0, 0], [-2, 0, 0, 0]], np.float32)
    rng = np.random.default_rng(40)
    X40 = np.empty((40, 4), np.float32)
    X40[:6] = X6
    X40[6:, 0] = -(1.5 + 0.25 * np.arange(34))
    X40[6:, 1:] = rng.integers(-3, 4, (34, 3))
    return (X6, np.array([1, 0, 0, 0], np.float32), 5), (X40, 1, 5)


STRIDE_NS = (1, 2, 1023, 1024, 1025, 2047, 2048, 2049, 4096, 4097)
STRIDE_KS = (1, 7)


def stride_case(N, metric):
    """(X, a dozen query ids with 0 and N - 1, 4 query vectors)"""
    rng = np.random.default_rng(6000 + 10 * N + metric)
    X = rng.standard_normal((N, 5)).astype(np.float32)
    qs = np.unique(np.concatenate([rng.integers(0, N, 10), [0, N - 1]])).astype(np.int64)
    return X, rng.permutation(qs), rng.standard_normal((4, 5)).astype(np.float32)


# k at the buffer rule: k + 1 == 1024 == SEL_CAP / 2 is the last k the fast kernel answers
KCAP_N, KCAP_D = 1500, 8
KCAP_KS = (1023, 1024, KCAP_N + 3)
# (metric, k) -> the seed of the series that is used (0 where not listed): the first one with which no checked query has two equal
# distances among its k + 1 best in the reference's own arithmetic (tests/test_topk_scan_cases_cpu.py verifies it)
KCAP_SEED_TRY = {
    (EUCLIDEAN, 1023): 2,
    (EUCLIDEAN, 1024): 2,
    (EUCLIDEAN, KCAP_N + 3): 1,
    (COSINE, KCAP_N + 3): 1,
}


def kcap_case(metric, k, seed_try=None):
    """(X, 6 query ids, 4 query vectors)"""
    s = KCAP_SEED_TRY.get((metric, k), 0) if seed_try is None else seed_try
    rng = np.random.default_rng(8100 + 10 * metric + k + 100_000 * s)
    X = rng.standard_normal((KCAP_N, KCAP_D)).astype(np.float32)
    X *= rng.uniform(0.5, 2.0, (KCAP_N, 1)).astype(np.float32)
    qs = np.concatenate([rng.integers(0, KCAP_N, 4), [0, KCAP_N - 1]]).astype(np.int64)
    return X, qs, rng.standard_normal((4, KCAP_D)).astype(np.float32)


MASK_N, MASK_D, MASK_K = 8 * SEL_THREADS, 6, 10
MASK_NAMES = ("one_stride", "two_strides", "k_minus_1", "k", "k_plus_1", "none", "random")


def mask_case():
    """(X, 4 query vectors, {name: mask}, a row every mask hides): A = 8 < k in one stride; A = 16 >= k + 1 in two strides,
    where the 8 kept keys never reach k + 1 and the bound saturates; exactly k - 1, k and k + 1 rows; no row; 60 % of the rows"""
    rng = np.random.default_rng(8192)
    X = rng.standard_normal((MASK_N, MASK_D)).astype(np.float32)
    i = np.arange(MASK_N)
    masks = {"one_stride": i % SEL_THREADS == 3, "two_strides": (i % SEL_THREADS == 3) | (i % SEL_THREADS == 4)}
    for name, n in (("k_minus_1", MASK_K - 1), ("k", MASK_K), ("k_plus_1", MASK_K + 1)):
        masks[name] = np.isin(i, rng.choice(MASK_N, n, replace=False))
    masks["none"] = np.zeros(MASK_N, bool)
    masks["random"] = rng.random(MASK_N) < 0.6
    hidden = int(np.nonzero(~np.any(list(masks.values()), axis=0))[0][7])  # a row no mask admits
    return X, rng.standard_normal((4, MASK_D)).astype(np.float32), {n: m.astype(np.uint8) for n, m in masks.items()}, hidden


NONFINITE_K = 15
NONFINITE_ROWS = (5, 77, 300)  # a NaN, a +inf and a -inf entry


def nonfinite_case():
    """(X, 5 query ids, 4 query vectors, {name: mask}): an 800 x 12 index with a NaN, a +inf and a -inf entry in three rows.  The
    query vectors and rows have positive entries against the two infinite ones, so that -dot sees one -inf and one +inf distance.
    'nan_hidden' hides row 5 alone (the cosine distance to an infinite row is still NaN), 'all_hidden' the three rows."""
    rng = np.random.default_rng(21)
    X = rng.standard_normal((800, 12)).astype(np.float32)
    X[5, 3], X[77, 0], X[300, 1] = np.nan, np.inf, -np.inf
    qv = rng.standard_normal((4, 12)).astype(np.float32)
    qv[:, :2] = np.abs(qv[:, :2])
    ok = np.nonzero((X[:, 0] > 0) & (X[:, 1] > 0) & np.isfinite(X).all(1))[0]
    qs = ok[[0, 9, 3, 30, 3]].astype(np.int64)
    masks = {"nan_hidden": np.ones(800, np.uint8), "all_hidden": np.ones(800, np.uint8)}
    masks["nan_hidden"][5] = 0
    masks["all_hidden"][list(NONFINITE_ROWS)] = 0
    return X, qs, qv, masks


def distinct_best(dist, k):
    """no NaN among the distances and no equal pair among the k + 1 smallest (-0 = +0): the fast kernel's own condition, on the
    oracle's ascending list of ALL of a query's distances"""
    d = np.asarray(dist, np.float32) + np.float32(0)
    return not np.isnan(d).any() and np.unique(d[:k + 1]).size == min(k + 1, d.size)


REROUTE_N, REROUTE_D, REROUTE_K = 300, 8, 15
BLOCK_N, BLOCK_D, BLOCK_K, BLOCK_QUERIES = 300, 6, 10, 7
GRID_Y = 65535  # queries of a scan block at most (dist_kernel's grid y)


def reroute_case():
    """small-integer rows: most queries have equal distances among their k + 1 best"""
    rng = np.random.default_rng(4)
    X = rng.integers(-2, 3, (REROUTE_N, REROUTE_D)).astype(np.float32)
    return X, np.arange(40, dtype=np.int64), (rng.random(REROUTE_N) < 0.7).astype(np.uint8)


def block_case(dtype):
    """(X, Xe, 100 unordered query ids with repeats, 50 query vectors as given, the same as fp32)"""
    rng = np.random.default_rng(4300 + dtype)
    X, Xe = as_index(rng.standard_normal((BLOCK_N, BLOCK_D)).astype(np.float32), dtype)
    qs = np.concatenate([rng.integers(0, BLOCK_N, 96), [5, 5, BLOCK_N - 1, 0]]).astype(np.int64)
    qv, qe = as_index(rng.standard_normal((50, BLOCK_D)).astype(np.float32), dtype)
    return X, Xe, qs, qv, qe
