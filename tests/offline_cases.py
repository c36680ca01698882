"""Shapes and references of tests/test_gpu_offline_past_one_grid.py: the caps of the offline pass's launchers as literals
(tests/test_offline_grid_caps_cpu.py holds them against the sources), and restatements of the candidate chain's stage rule and of a
neighbour table's rows over padded numpy arrays, for passes of millions of queries that the per-query Python of tests/cand_ref.py
and tests/nbr_build_ref.py cannot walk in a test's time.  The restatements are held against those two on small shapes, and on a
sample of the big pass's own queries, by the CPU test before any device result is compared with them."""
import numpy as np

import cand_ref as R

# ---- what one step of every loop holds (csrc/cand.hip, csrc/nbr_build.hip, csrc/csr_scan.hpp, csrc/recommend.hip) -------------
GRID = 1 << 20                   # kMaxGrid of cand.hip and nbr_build.hip: workgroups of one launch at most
CAND_WAVES = RULE_WAVES = 4      # queries / rows per workgroup of the wave-per-row kernels
BLOCK_GRID_QUERIES = GRID        # cand_sort_kernel, cand_merge_kernel
WAVE_GRID_QUERIES = 4 * GRID     # cand_filter_kernel, cand_append_kernel, cand_compact_kernel
ROW_GRID_ROWS = 4 * GRID         # nbr_rule_kernel, nbr_compact_kernel, nbr_bound_kernel
SCAN_TILE = 2048                 # counts per workgroup of csr_exclusive_scan
SCAN_TOP = 256                   # workgroup sums per pass of nbr_scan_top_kernel
SCAN_ONE_TOP_PASS = SCAN_TILE * SCAN_TOP  # 524,288 counts
REC_HOOK = (8, 8192)             # gorse_hip_test_set_recommend(slices, buffer, 0) ...
REC_HOOK_K = 10                  # ... at this k ...
REC_HOOK_CHUNK = 240             # ... gives launches of this many queries (recomputed from recommend.hip by the CPU test)
REC_MAX_SLICES = 8

PAD = np.iinfo(np.int32).max     # behind a padded row's entries; no item is this large (n_items <= 2^31 - 1)


def stride_step(t):
    """where query t falls in the strided loops: the message of a failed comparison"""
    return "query %d: step %d of the workgroup-per-query kernels, step %d of the wave-per-query kernels" % (
        t, t // BLOCK_GRID_QUERIES, t // WAVE_GRID_QUERIES)


# ---- the candidate chain over padded arrays -------------------------------------------------------------------------------------

class VChain:
    """cand_ref.Chain for rows that fit padded arrays: row t's entries are base[t, :base_len[t]], a stage's list of query t is
    items[t, :lens[t]].  Same rule: the exclusion set is the row at the start of the stage, a list's repeated item stays twice."""

    def __init__(self, base, base_len, capacity):
        base, base_len = np.asarray(base, np.int32), np.asarray(base_len, np.int64)
        n = base.shape[0]
        assert base.max(initial=0) < PAD
        self.cur = sort_rows(np.where(np.arange(base.shape[1]) < base_len[:, None], base, PAD))
        self.cur_len = base_len.copy()
        self.items = np.full((n, capacity), -1, np.int32)
        self.scores = np.zeros((n, capacity), np.uint64)
        self.stages = np.zeros((n, capacity), np.uint8)
        self.cnt = np.zeros(n, np.int64)
        self.stage = 0

    def add(self, items, scores, lens, k, keep=None):
        """items / scores: (n, L), or (L,) for one list shared by every query; entries past lens[t] must still be item numbers"""
        n = self.cur.shape[0]
        items = np.asarray(items, np.int32)
        L = items.shape[-1]
        ok = np.arange(L, dtype=np.int16) < np.asarray(lens, np.int16)[:, None]
        if keep is not None:
            ok &= np.asarray(keep)[items] != 0
        items = np.broadcast_to(items, (n, L))
        bits = np.broadcast_to(np.ascontiguousarray(scores, np.float64).view(np.uint64), (n, L))
        for w in range(self.cur.shape[1]):
            ok &= items != self.cur[:, w:w + 1]
        pos = np.cumsum(ok, axis=1, dtype=np.int16)
        pos -= 1
        ok &= pos < k
        rows, cols = np.nonzero(ok)
        at = pos[rows, cols]
        dst = self.cnt[rows] + at  # (int64: the index of a column)
        assert dst.max(initial=0) < self.items.shape[1]
        self.items[rows, dst] = items[rows, cols]
        self.scores[rows, dst] = bits[rows, cols]
        self.stages[rows, dst] = self.stage
        new = np.full((n, min(k, L)), PAD, np.int32)
        new[rows, at] = items[rows, cols]
        kept = ok.sum(axis=1, dtype=np.int64)
        self.cnt += kept
        self.cur = sort_rows(np.concatenate([self.cur, new], axis=1))
        self.cur_len += kept
        self.stage += 1

    def exclusion(self):
        mask = np.arange(self.cur.shape[1]) < self.cur_len[:, None]
        return ptr_of(self.cur_len), self.cur[mask]

    def finished(self, keep=None):
        ok = np.arange(self.items.shape[1]) < self.cnt[:, None]
        if keep is not None:
            ok &= np.asarray(keep)[np.where(ok, self.items, 0)] != 0
        return ptr_of(ok.sum(axis=1)), self.items[ok], self.scores[ok], self.stages[ok]


def sort_rows(a):
    """every row ascending.  The rows are a few entries wide and there are millions of them: an odd-even transposition network
    over the columns, where a sort per row would spend its time between the rows"""
    if a.shape[1] > 16:
        return np.sort(a, axis=1)
    cols = [a[:, c].copy() for c in range(a.shape[1])]
    for step in range(len(cols)):
        for c in range(step % 2, len(cols) - 1, 2):
            lo, hi = np.minimum(cols[c], cols[c + 1]), np.maximum(cols[c], cols[c + 1])
            cols[c], cols[c + 1] = lo, hi
    return np.stack(cols, axis=1)


def ptr_of(lens):
    ptr = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=ptr[1:])
    return ptr


def splice(bulk, at, rows):
    """the CSR `bulk` = (ptr, flat arrays ...) with its rows `at` (ascending; empty in bulk) replaced by the rows of the CSR `rows`"""
    ptr, rptr = bulk[0], np.asarray(rows[0], np.int64)
    lens, rl = np.diff(ptr), np.diff(rptr)
    assert len(at) == len(rl) and not lens[at].any()
    where = np.repeat(ptr[at], rl)
    lens[at] = rl
    return (ptr_of(lens),) + tuple(np.insert(a, where, np.asarray(r).astype(a.dtype)) for a, r in zip(bulk[1:], rows[1:]))


class ChainCase:
    """one pass: begin(base rows), add_lists(k_lists), add_shared(k_shared, keep_shared), finish(keep_finish).  base_of(t) ->
    (items (n, W), lengths) and lists_of(t) -> (items (n, L), float64 scores (n, L), lengths) give the rows of the queries t (an
    int64 array) that padded arrays hold; marked[t] = (base row, [(item, score), ...]) are the queries they cannot."""

    def __init__(self, nq, n_items, capacity, k_lists, k_shared, base_of, lists_of, shared, keep_shared, keep_finish, marked=None):
        self.nq, self.n_items, self.capacity, self.k_lists, self.k_shared = nq, n_items, capacity, k_lists, k_shared
        self.base_of, self.lists_of = base_of, lists_of
        self.shared_items, self.shared_scores = np.asarray(shared[0], np.int32), np.asarray(shared[1], np.float64)
        self.keep_shared, self.keep_finish = keep_shared, keep_finish
        self.marked = marked or {}
        self.marked_at = np.array(sorted(self.marked), np.int64)

    def is_marked(self, q):
        return np.isin(q, self.marked_at)

    def base_csr(self, q=None):
        """the base rows of the queries q as gorse_cand_begin takes them (unsorted)"""
        q = np.arange(self.nq, dtype=np.int64) if q is None else np.asarray(q, np.int64)
        items, lens = self.base_of(q)
        mk = self.is_marked(q)
        lens = np.where(mk, 0, lens)
        bulk = (ptr_of(lens), np.asarray(items, np.int32)[np.arange(items.shape[1]) < lens[:, None]])
        return splice(bulk, np.flatnonzero(mk), R.csr([self.marked[int(t)][0] for t in q[mk]]))

    def lists_csr(self, q=None):
        q = np.arange(self.nq, dtype=np.int64) if q is None else np.asarray(q, np.int64)
        items, scores, lens = self.lists_of(q)
        mk = self.is_marked(q)
        lens = np.where(mk, 0, lens)
        m = np.arange(items.shape[1]) < lens[:, None]
        bulk = (ptr_of(lens), np.asarray(items, np.int32)[m], np.asarray(scores, np.float64)[m])
        lists = [self.marked[int(t)][1] for t in q[mk]]
        ptr, li = R.csr([[e[0] for e in l] for l in lists])
        return splice(bulk, np.flatnonzero(mk), (ptr, li, R.csr([[e[1] for e in l] for l in lists], np.float64)[1]))


class ChainResult:
    """excl[s] = the exclusion CSR after begin (s = 0) and after stage s - 1; info[s] likewise; finished = (ptr, items, score
    bits, stages); info_finished"""


def expected_chain(case, q=None):
    """the pass of `case` over the queries q (all of them by default): padded arrays for the bulk, cand_ref.Chain for the marked"""
    q = np.arange(case.nq, dtype=np.int64) if q is None else np.asarray(q, np.int64)
    mk = case.is_marked(q)
    at = np.flatnonzero(mk)
    marked = [case.marked[int(t)] for t in q[at]]
    base, blen = case.base_of(q)
    v = VChain(base, np.where(mk, 0, blen), case.capacity)
    ref = R.Chain(len(at), [m[0] for m in marked])
    out = ChainResult()
    out.excl, out.info = [], []

    def snapshot():
        out.excl.append(splice(v.exclusion(), at, ref.exclusion()))
        out.info.append((len(q), v.stage, int(v.cnt.sum()) + sum(len(r) for r in ref.cand), int(out.excl[-1][0][-1])))

    snapshot()
    items, scores, lens = case.lists_of(q)
    v.add(items, scores, np.where(mk, 0, lens), case.k_lists)
    ref.add([m[1] for m in marked], case.k_lists)
    snapshot()
    v.add(case.shared_items, case.shared_scores, np.where(mk, 0, case.shared_items.size), case.k_shared, case.keep_shared)
    ref.add_shared(case.shared_items.tolist(), case.shared_scores.tolist(), case.k_shared, case.keep_shared)
    snapshot()
    out.finished = splice(v.finished(case.keep_finish), at, ref.finished(case.keep_finish))
    out.info_finished = out.info[-1][:2] + (int(out.finished[0][-1]), out.info[-1][3])
    return out


def chain_by_reference(case, q):
    """the same pass through cand_ref.Chain alone, query by query"""
    q = np.asarray(q, np.int64)
    mk = case.is_marked(q)
    base, blen = case.base_of(q)
    items, scores, lens = case.lists_of(q)
    rows, lists = [], []
    for r, t in enumerate(q):
        if mk[r]:
            rows.append(case.marked[int(t)][0])
            lists.append(case.marked[int(t)][1])
        else:
            rows.append(base[r, :blen[r]].tolist())
            lists.append([(int(i), float(s)) for i, s in zip(items[r, :lens[r]], scores[r, :lens[r]])])
    ref = R.Chain(len(q), rows)
    out = ChainResult()
    out.excl = [ref.exclusion()]
    ref.add(lists, case.k_lists)
    out.excl.append(ref.exclusion())
    ref.add_shared(case.shared_items.tolist(), case.shared_scores.tolist(), case.k_shared, case.keep_shared)
    out.excl.append(ref.exclusion())
    out.finished = ref.finished(case.keep_finish)
    return out


def first_difference(got, want, ptr=None):
    """None when the arrays are equal; else the first differing position, as a query number when ptr (a row pointer) is given"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return -1
    bad = np.flatnonzero(got != want)
    if bad.size == 0:
        return None
    return int(bad[0]) if ptr is None else int(np.searchsorted(ptr, bad[0], side="right") - 1)


def assert_csr(got, want, names, what):
    """got / want = (ptr, flat arrays ...); the message names the first differing query and its stride steps"""
    t = first_difference(got[0], want[0])
    assert t is None, (what, names[0], stride_step(max(t - 1, 0)))
    for g, w, name in zip(got[1:], want[1:], names[1:]):
        t = first_difference(g, w, want[0])
        assert t is None, (what, name, stride_step(t))


def _mix(t, salt):
    """a fixed 64-bit mix of the query number: the bulk rows are a function of t alone"""
    x = (np.asarray(t).astype(np.uint64) + np.uint64(salt)) * np.uint64(0x9E3779B97F4A7C15)
    x ^= x >> np.uint64(29)
    x *= np.uint64(0xBF58476D1CE4E5B9)
    x ^= x >> np.uint64(32)
    return x


BULK_ITEMS = 12  # the bulk's rows and lists draw from items 0 .. 11, so that lists meet base rows, each other and the shared list


def bulk_base(t):
    """0 .. 2 items, in either order when 2, now and then the same item twice"""
    h = _mix(t, 1)
    a, b = (h % np.uint64(BULK_ITEMS)).astype(np.int32), ((h >> np.uint64(8)) % np.uint64(BULK_ITEMS)).astype(np.int32)
    return np.stack([a, b], axis=1), ((h >> np.uint64(16)) % np.uint64(3)).astype(np.int64)


def bulk_lists(t):
    """0 .. 3 distinct items: start + i * step modulo 12 with a step coprime to 12; the score names the query and the entry"""
    h = _mix(t, 2)
    start = (h % np.uint64(BULK_ITEMS)).astype(np.int32)
    step = np.array([1, 5, 7, 11], np.int32)[((h >> np.uint64(8)) % np.uint64(4)).astype(np.int64)]
    e = np.arange(3, dtype=np.int32)
    items = (start[:, None] + e * step[:, None]) % np.int32(BULK_ITEMS)
    scores = np.asarray(t, np.float64)[:, None] * 0.25 - e
    return items, scores, ((h >> np.uint64(16)) % np.uint64(4)).astype(np.int64)


BIG_NQ = WAVE_GRID_QUERIES + 37
BIG_N_ITEMS = 20000
MARKED_LENGTHS = (65, 300, 4097)  # an LDS sort of one pass, of several, and a sort in global memory (more than 4096 entries)


def big_chain_case():
    """4 * 2^20 + 37 queries: past the 2^20 workgroups of cand_sort_kernel / cand_merge_kernel four times over, past the 4 * 2^20
    waves of the filter, append and compact kernels once, and 2049 workgroup sums for nbr_scan_top_kernel (nine passes).  About
    200 marked queries -- both sides of every multiple of 2^20 that matters, the ends, and random others -- carry long unsorted
    base rows with repeats and lists that interleave with them; query 1 (4097 entries, sorted in global memory) comes directly
    before query 2^20 + 1 (300 entries, sorted in LDS) in the stride of workgroup 1."""
    rng = np.random.default_rng(41)
    nq = BIG_NQ
    fixed = [0, 1, GRID - 1, GRID, GRID + 1, 2 * GRID, 4 * GRID - 1, 4 * GRID, 4 * GRID + 1, nq - 1]
    at = sorted(set(fixed) | set(rng.choice(nq, 190, replace=False).tolist()))
    length = {t: MARKED_LENGTHS[i % 3] for i, t in enumerate(at)}
    length[1], length[GRID + 1] = 4097, 300
    length[0], length[4 * GRID] = 300, 4097      # and the other order in the stride of workgroup 0 (through 2^20, 2 * 2^20, ...)
    marked = {}
    for i, t in enumerate(at):
        base = rng.integers(BULK_ITEMS, BIG_N_ITEMS, length[t]).tolist()
        base[5], base[-1] = base[40], base[0]    # repeats, away from their first copies
        fresh = np.setdiff1d(np.arange(BIG_N_ITEMS), base)
        n_list = (256, 0, 1, 3, 256, 2)[i % 6]
        # the list opens with items of the base row (the walk passes them), then items between the row's entries
        lst = (base[7:7 + (i % 4)] + rng.choice(fresh, 256, replace=False).tolist())[:n_list]
        marked[t] = (base, [(int(j), float(t) * 0.25 - e) for e, j in enumerate(lst)])
    keep_shared = np.ones(BIG_N_ITEMS, np.uint8)
    keep_shared[[7, 4]] = 0
    keep_finish = (np.arange(BIG_N_ITEMS) % 5 != 0).astype(np.uint8)
    shared = ([3, 7, 0, 4, 11, 5, 9, 13], [8.0, 7.0, 6.0, 5.0, 4.0, 3.0, 2.0, 1.0])
    return ChainCase(nq, BIG_N_ITEMS, 4, 2, 2, bulk_base, bulk_lists, shared, keep_shared, keep_finish, marked)


def tiny_rows_case(nq):
    """test_many_queries_with_tiny_rows of tests/test_gpu_cand.py as arrays: 97 items, base rows of 0 .. 3 entries, lists of 0 .. 5
    (repeats allowed) cut at 3, a shared list of 4 cut at 2, capacity 5, every fifth item dropped by finish"""
    rng = np.random.default_rng(nq)
    n_items = 97
    base, base_len = rng.integers(0, n_items, (nq, 3)).astype(np.int32), rng.integers(0, 4, nq)
    items, lens = rng.integers(0, n_items, (nq, 5)).astype(np.int32), rng.integers(0, 6, nq)
    scores = rng.normal(0, 1, (nq, 5))
    keep = (np.arange(n_items) % 5 != 0).astype(np.uint8)
    return ChainCase(nq, n_items, 5, 3, 2, lambda t: (base[t], base_len[t]), lambda t: (items[t], scores[t], lens[t]),
                     ([5, 96, 0, 33], [1.0, 2.0, 3.0, 4.0]), None, keep)


# ---- neighbour tables ---------------------------------------------------------------------------------------------------------

def expand_table(ptr, idx, w, sources):
    """the table whose row r is row sources[r] of the CSR (ptr, idx, w), or empty where sources[r] < 0: a neighbour list depends
    on its source alone, so a table over repeated sources is the stored rows' table expanded"""
    src = np.asarray(sources, np.int64)
    lens = np.where(src >= 0, np.diff(ptr)[np.maximum(src, 0)], 0)
    out = ptr_of(lens)
    take = np.repeat(ptr[np.maximum(src, 0)] - out[:-1], lens) + np.arange(out[-1])
    return out, idx[take], w[take]


def edge_sources(n_rows, index_n, n_valid=300, seed=0):
    """about n_valid valid sources among n_rows, the rest -1: valid at row 0, at the last row and on both sides of every multiple
    of the scan's 2048 below n_rows"""
    rng = np.random.default_rng(seed + n_rows)
    src = np.full(n_rows, -1, np.int64)
    at = {0, n_rows - 1}
    for m in range(SCAN_TILE, n_rows, SCAN_TILE):
        at |= {m - 1, m}
    at |= set(rng.choice(n_rows, n_valid - len(at), replace=False).tolist())
    at = np.array(sorted(at))
    src[at] = rng.integers(0, index_n, at.size)
    return src


BIG_ROWS = ROW_GRID_ROWS + 101


def big_sources(index_n):
    """4 * 2^20 + 101 rows over the index's rows, a stride of 7 apart (row r and the row r + 4 of the next wave name different
    stored rows), with 64 rows of -1: row 1, the last row, both sides of row 4 * 2^20, and others at fixed places"""
    r = np.arange(BIG_ROWS, dtype=np.int64)
    src = (7 * r + 3) % index_n
    none = [1, BIG_ROWS - 1, ROW_GRID_ROWS - 2, ROW_GRID_ROWS - 1, ROW_GRID_ROWS, ROW_GRID_ROWS + 2, ROW_GRID_ROWS + 50]
    none += [1000 + 65537 * i for i in range(64 - len(none))]
    assert len(set(none)) == 64 and max(none) < BIG_ROWS
    src[none] = -1
    return src


def big_sample_rows():
    """about 40 rows of the big table to recommend from: the ends, both sides of 2^22, rows without a source, and others"""
    rows = [0, 1, 2, 3, ROW_GRID_ROWS - 3, ROW_GRID_ROWS - 2, ROW_GRID_ROWS - 1, ROW_GRID_ROWS, ROW_GRID_ROWS + 1, ROW_GRID_ROWS + 2,
            ROW_GRID_ROWS + 3, ROW_GRID_ROWS + 99, ROW_GRID_ROWS + 100, 1000, 1000 + 65537, GRID - 1, GRID, 2 * GRID, 3 * GRID + 5]
    rows += np.random.default_rng(6).choice(BIG_ROWS, 21, replace=False).tolist()
    return np.array(rows, np.int64)


# ---- recommend ------------------------------------------------------------------------------------------------------------------

def ties_world(n_users=40, n_items=1031, d=24):
    """equal item rows among everybody's best (users 0 .. 19 score items 100, 101 and 900 highest, and equally) and all-zero user
    rows (users 20 .. 29: every score is a zero): queries of these users are tied at every k"""
    rng = np.random.default_rng(23)
    P = rng.standard_normal((n_users, d)).astype(np.float32)
    Q = rng.standard_normal((n_items, d)).astype(np.float32)
    sign = np.where(rng.random(d) < 0.5, -1.0, 1.0).astype(np.float32)
    Q[100] = Q[101] = Q[900] = 4.0 * sign
    P[:20] = np.abs(P[:20]) * sign
    P[20:30] = 0.0
    rows = [np.setdiff1d(rng.choice(n_items, int(rng.integers(0, 300)), replace=False), [100, 101, 900]).astype(np.int32)
            for _ in range(n_users)]
    return P, Q, rows
