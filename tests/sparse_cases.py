"""Inputs and the oracle comparison of the sparse top-k GPU parity tests (tests/test_gpu_vectors_sparse.py,
tests/test_gpu_sparse_sym.py, tests/test_gpu_sparse_long_rows.py)."""
import numpy as np


def random_csr(rng, rows, dims, lo, hi, neg=False, zipf=False):
    """rows sparse vectors over `dims` indices with lo..hi entries each, indices strictly ascending"""
    ptr = [0]
    idx, val = [], []
    pop = None
    if zipf:
        pop = 1.0 / np.arange(1, dims + 1)
        pop = pop / pop.sum()
    for _ in range(rows):
        n = min(int(rng.integers(lo, hi + 1)), dims)
        ids = np.sort(rng.choice(dims, size=n, replace=False, p=pop)).astype(np.uint32)
        v = rng.random(n).astype(np.float32) + np.float32(0.05)
        if neg:
            v *= rng.choice(np.array([-1, 1], dtype=np.float32), size=n)
        idx.append(ids)
        val.append(v)
        ptr.append(ptr[-1] + n)
    return (np.array(ptr, dtype=np.int64), np.concatenate(idx) if idx else np.zeros(0, np.uint32),
            np.concatenate(val) if val else np.zeros(0, np.float32))


def rows_with_lengths(rng, dims, lengths, wide=False):
    """A CSR whose row r has exactly lengths[r] strictly ascending indices below `dims`.  Values are signed; with `wide` their
    magnitudes are exp(uniform(-14, 14)), so that the float32 sum of a row's products depends on the order of its terms."""
    lengths = np.asarray(lengths, dtype=np.int64)
    assert lengths.min(initial=0) >= 0 and lengths.max(initial=0) <= dims
    ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    idx = np.empty(int(ptr[-1]), np.uint32)
    for r, n in enumerate(lengths):
        idx[ptr[r]:ptr[r + 1]] = np.arange(dims) if n == dims else np.sort(rng.choice(dims, size=int(n), replace=False))
    sign = rng.choice(np.array([-1.0, 1.0]), size=idx.size)
    mag = np.exp(rng.uniform(-14, 14, idx.size)) if wide else rng.random(idx.size) + 0.05
    return ptr, idx, (mag * sign).astype(np.float32)


# ---- the collections of tests/test_gpu_sparse_long_rows.py (their properties: tests/test_sparse_long_cases_cpu.py) ------------------
# L: stored rows on both sides of the 1024 entries from which sparse_rows_kernel walks a row with the whole wave, 64 entries per step:
# lengths 0, 1 and 63 mod 64, one row that holds every index, two pairs of equal lengths
L_DIMS = 4096
L_LONG = [1024, 1025, 1026, 1087, 1088, 1089, 1500, 2049, 3000, 4096, 1025, 1088]
L_QUERY_LENGTHS = [30, 50, 300, 1050, 2000, 4096]  # ~ 0.5 (x), 0.8, 5, 16, 31 and 64 matches per 64-entry step of a long row
L_THRESHOLD = 40  # split = heavy threshold of the searches over L: every query above but the first is heavy


def long_rows_case(long_row_last=False):
    """(ptr, idx, val, rows of the twelve long rows in the order of L_LONG): 600 rows over 4096 dims, wide values, the others with
    0..40 entries (empty ones among them), row order shuffled; with long_row_last the CSR ends with a long row"""
    rng = np.random.default_rng(1024)
    short = rng.integers(0, 41, 588)
    short[:5] = 0
    lengths = np.concatenate([L_LONG, short])
    while True:
        order = rng.permutation(lengths.size)
        if (order[-1] < len(L_LONG)) == long_row_last:
            break
    ptr, idx, val = rows_with_lengths(rng, L_DIMS, lengths[order], wide=True)
    where = np.empty(lengths.size, np.int64)
    where[order] = np.arange(lengths.size)
    return ptr, idx, val, [int(r) for r in where[:len(L_LONG)]]


def step_matches(row_idx, q_idx):
    """matches of the query per step of 64 consecutive entries of the stored row"""
    hit = np.isin(row_idx, q_idx)
    return [int(hit[s:s + 64].sum()) for s in range(0, row_idx.size, 64)]


def long_rows_queries(ptr, idx, val, long_rows):
    """(qp, qi, qv) of the searches over L: one query per L_QUERY_LENGTHS, then the hand-built one against the 1089-entry row: 16
    matches in the row's first 64 entries (the per-match sum), 17 in the second (the all-lanes sum), all 64 of the third, none of
    the fourth, random shares of the others, the single entry of the last step; and 40 indices that the row lacks"""
    rng = np.random.default_rng(2049)
    qp, qi, qv = rows_with_lengths(rng, L_DIMS, L_QUERY_LENGTHS, wide=True)
    r = long_rows[L_LONG.index(1089)]
    row = idx[ptr[r]:ptr[r + 1]]
    take = [rng.choice(row[0:64], 16, replace=False), rng.choice(row[64:128], 17, replace=False), row[128:192], row[1088:]]
    for s in range(256, 1088, 64):
        take.append(rng.choice(row[s:s + 64], int(rng.integers(0, 65)), replace=False))
    take.append(rng.choice(np.setdiff1d(np.arange(L_DIMS, dtype=np.uint32), row), 40, replace=False))
    hand = np.sort(np.concatenate(take)).astype(np.uint32)
    hv = (np.exp(rng.uniform(-14, 14, hand.size)) * rng.choice(np.array([-1.0, 1.0]), hand.size)).astype(np.float32)
    return np.concatenate([qp, [qp[-1] + hand.size]]).astype(np.int64), np.concatenate([qi, hand]), np.concatenate([qv, hv])


# B: rows past the thresholds in force without any hook (heavy 16384, split 2048, the whole-wave walk's 1024)
B_DIMS = 20000
B_HEAVY = [16384, 16385, 16386, 16449, 16450, 17000, 17777, 18000, 19000, 19999, 20000, 16385]
B_SPLIT = [2048, 2049, 2050]
B_MIDDLE = [1024, 1025, 1500, 2000]


def production_thresholds_case():
    """(ptr, idx, val): ~2150 rows over 20,000 dims, ~375,000 entries, row order shuffled: B_HEAVY (eleven past 16384), B_SPLIT and
    thirty rows of 2049..6000 (44 rows past 2048), B_MIDDLE, 2100 rows of 0..30"""
    rng = np.random.default_rng(16384)
    lengths = np.concatenate([B_HEAVY, B_SPLIT, rng.integers(2049, 6001, 30), B_MIDDLE, rng.integers(0, 31, 2100)])
    return rows_with_lengths(rng, B_DIMS, rng.permutation(lengths))


# W: more distinct indices x row groups than one workgroup of the directory scan takes with one chunk sum per thread (1024 x 8192
# cells), and more rows past 20 entries than a launch round holds dense copies for (2^30 bytes / 8 / distinct indices)
W_ROWS, W_SPACE, W_SHARED = 12000, 400000, 300
W_LONG = 20  # the split threshold of the several-round calls


def dense_copy_bound(distinct):
    return (1 << 30) // (distinct * 8)


def launch_round_bound(distinct, groups, n_ranges, k):
    """long queries per launch round (csrc/sparse.hip, per_launch): 2 GiB of partial rankings -- one of KP >= k keys per row group, or
    per row range of the heavy-query kernel where those are more --, 1 GiB of dense copies, a grid dimension"""
    kp = next(p for p in (128, 256, 512, 1024) if k <= p)
    return max(1, min((2 << 30) // (max(groups, n_ranges) * kp * 8), dense_copy_bound(distinct), 32768))


def wide_directory_case():
    """(ptr, idx, val, shared indices): 12,000 rows; 14..19 private indices each (3000 rows 8 more), dealt from one permutation of
    the index space (so each is distinct, with gaps between them), and 0..4 of 300 shared indices"""
    rng = np.random.default_rng(8388608)
    perm = rng.permutation(W_SPACE).astype(np.uint32)
    shared, at = np.sort(perm[:W_SHARED]), W_SHARED
    n_private = rng.integers(14, 20, W_ROWS)
    n_private[rng.choice(W_ROWS, 3000, replace=False)] += 8
    rows = []
    for n in n_private:
        rows.append(np.sort(np.concatenate([perm[at:at + n], rng.choice(shared, int(rng.integers(0, 5)), replace=False)])))
        at += n
    ptr = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int64)
    idx = np.concatenate(rows).astype(np.uint32)
    val = ((rng.random(idx.size) + 0.05) * rng.choice(np.array([-1.0, 1.0]), idx.size)).astype(np.float32)
    return ptr, idx, val, shared


def rows_of(ptr, idx, val, rows):
    return [(idx[ptr[r]:ptr[r + 1]], val[ptr[r]:ptr[r + 1]]) for r in rows]


def check_against_oracle(o, ptr, idx, val, k, got, queries, excludes, mask=None):
    """got = (idx nq x k, score nq x k, cnt nq): rows, score BITS, counts and padding equal the oracle's"""
    out_idx, out_sc, out_cnt = got[0], got[1], got[2]
    for t, (qi, qv) in enumerate(queries):
        ei, es = o.sparse_search(ptr, idx, val, qi, qv, k, exclude=excludes[t], admissible=mask)
        assert out_cnt[t] == ei.size, (t, out_cnt[t], ei.size)
        assert np.array_equal(out_idx[t, :ei.size], ei), t
        assert np.array_equal(out_sc[t, :ei.size].view(np.uint32), es.view(np.uint32)), t
        assert (out_idx[t, ei.size:] == -1).all() and np.isneginf(out_sc[t, ei.size:]).all(), t


# rows with equal scores, products that cancel to +-0, an empty row, a row of explicit zeros, negative scores
TIE_ROWS = [([1, 4], [1.0, 1.0]), ([1, 4], [1.0, 1.0]), ([4], [2.0]), ([1, 9], [3.0, 1.0]), ([1, 4], [1.0, -1.0]),
            ([2], [5.0]), ([], []), ([1, 4], [-1.0, 1.0]), ([4, 9], [0.0, 0.0]), ([1], [-4.0]), ([1, 4], [1.0, 1.0]),
            ([4], [-4.0])]
# query 0 = {1: 1, 4: 1} with row 0 excluded and row 2 masked: scores 3 (row 3), 2 (rows 1 and 10: a tie, ascending row),
# -4 (rows 9 and 11), and six zero-score rows (4, 7, 8 cancel or multiply zeros; 5, 6 share nothing) -- the reference
# ranks all ten admissible rows, cuts to k and drops the zeros, so a negative row needs k > 3 + 5
TIE_EXPECT = {3: [3, 1, 10], 8: [3, 1, 10], 9: [3, 1, 10, 9], 10: [3, 1, 10, 9, 11], 20: [3, 1, 10, 9, 11]}


def tie_case():
    ptr = np.array([0] + list(np.cumsum([len(r[0]) for r in TIE_ROWS])), dtype=np.int64)
    idx = np.array([i for r in TIE_ROWS for i in r[0]], dtype=np.uint32)
    val = np.array([v for r in TIE_ROWS for v in r[1]], dtype=np.float32)
    qp = np.array([0, 2, 2, 3], dtype=np.int64)
    qi = np.array([1, 4, 77], dtype=np.uint32)  # query 1 is empty, query 2 only has an index nobody stored
    qv = np.array([1.0, 1.0, 1.0], dtype=np.float32)
    mask = np.ones(len(TIE_ROWS), dtype=np.uint8)
    mask[2] = 0
    excl = np.array([0, -1, -1], dtype=np.int64)
    return ptr, idx, val, (qp, qi, qv), mask, excl
