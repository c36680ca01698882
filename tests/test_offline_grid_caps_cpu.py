"""The caps that tests/test_gpu_offline_past_one_grid.py sizes its inputs from (the literals of tests/offline_cases.py), held against
the launchers' own text (no GPU): a cap raised later fails here instead of silently leaving a strided loop's second step unvisited
again.  And the restatements over padded arrays that the big comparisons rest on, held against tests/cand_ref.py and
tests/nbr_build_ref.py.

Every loop of the offline pass's device modules that walks more than one launch, grid or scan workgroup holds:

  launcher (kernel)                                       one step holds                      crossed by
  mf_recommend_core, the launch loop (rec_fast_kernel,    kRecScratchBytes / per_query        test_recommend_all_users_in_two_launches,
    rec_finish_kernel, the literal queries' numbers,        rounded down to 16: 240 queries   test_recommend_user_list_in_three_launches,
    the device rows at q0 * k)                              under the hook (8, 8192) at k 10  test_recommend_ties_past_the_first_launch,
                                                                                              test_chain_mf_stage_in_three_launches
  rec_fast_kernel's item slices                           min(slices, I) slices of            test_recommend_tiny_catalogues
                                                            ceil(I / slices) items
  csr_exclusive_scan of nbr_build.hip                     2048 counts per workgroup           test_table_scan_past_one_workgroup_dense,
                                                                                              test_table_scan_past_one_workgroup_sparse
  csr_exclusive_scan of cand.hip, nbr_scan_top_kernel     256 workgroup sums per pass:        test_chain_scan_top_pass_edges (256 and 257 sums),
                                                            524,288 counts                    test_chain_past_both_grids (2049 sums)
  cand_sort_kernel, cand_merge_kernel (block_grid)        2^20 queries, a workgroup each      test_chain_past_both_grids
  cand_filter_kernel, cand_append_kernel,                 4 * 2^20 queries, a wave each       test_chain_past_both_grids
    cand_compact_kernel, both passes (wave_grid)
  nbr_rule_kernel, nbr_compact_kernel,                    4 * 2^20 rows, a wave each          test_table_past_one_grid
    nbr_bound_kernel (row_grid)

(csr_exclusive_scan's kernels are compiled into either translation unit; test_table_past_one_grid runs the copy of nbr_build.hip
through nine passes of its top kernel as well.)"""
import re

import numpy as np

import nbr_build_ref as B
import offline_cases as oc
from test_mf_grid_caps_cpu import TESTS, constant, function_body, group_geometry, source


def shifted(text, name):
    """`constexpr int64_t NAME = (int64_t)A << B;` or `constexpr size_t NAME = (size_t)A << B;`"""
    m = re.search(r"constexpr (?:int64_t|size_t) %s = \((?:int64_t|size_t)\)(\d+) << (\d+);" % name, text)
    return int(m.group(1)) << int(m.group(2))


def test_chain_grids_hold_what_the_tests_assume():
    cand = source("cand.hip")
    assert shifted(cand, "kMaxGrid") == oc.GRID == 1 << 20
    assert constant(cand, "kCandWaves") == oc.CAND_WAVES == 4
    assert "unsigned wave_grid(int64_t rows) { return (unsigned)std::max<int64_t>(1, std::min(ceil_div(rows, kCandWaves), kMaxGrid)); }" in cand
    assert "unsigned block_grid(int64_t rows) { return (unsigned)std::max<int64_t>(1, std::min(rows, kMaxGrid)); }" in cand
    assert oc.BLOCK_GRID_QUERIES == oc.GRID and oc.WAVE_GRID_QUERIES == oc.CAND_WAVES * oc.GRID
    # every launch takes its grid from one of the two, and every kernel strides by its grid
    for kernel, grid in (("cand_sort_kernel", "block_grid(nq)"), ("cand_merge_kernel", "block_grid(nq)"),
                         ("cand_filter_kernel", "wave_grid(nq)"), ("cand_append_kernel", "wave_grid(nq)")):
        launches = re.findall(r"%s<<<dim3\(([^)]*\))\)" % kernel, cand)
        assert launches == [grid], (kernel, launches)
    assert "const dim3 grid(wave_grid(nq)), block(kCandWaves * 64);" in cand
    assert len(re.findall(r"cand_compact_kernel<<<grid, block, 0, st>>>", cand)) == 2  # the counting and the writing pass
    for kernel in ("cand_sort_kernel", "cand_merge_kernel"):
        assert "for (int64_t t = blockIdx.x; t < nq; t += gridDim.x) {" in function_body(cand, "void %s(" % kernel)
    for kernel, n in (("cand_filter_kernel", "A.nq"), ("cand_append_kernel", "nq"), ("cand_compact_kernel", "nq")):
        body = function_body(cand, "void %s(" % kernel)
        assert "const int64_t nw = (int64_t)gridDim.x * kCandWaves;" in body
        assert "for (int64_t t = (int64_t)blockIdx.x * kCandWaves + (threadIdx.x >> 6); t < %s; t += nw) {" % n in body
    assert oc.BIG_NQ > oc.WAVE_GRID_QUERIES > oc.BLOCK_GRID_QUERIES
    assert constant(cand, "kSortLds") == 4096 and sorted(oc.MARKED_LENGTHS)[-2:] == [300, 4097]


def test_table_grid_holds_what_the_tests_assume():
    build = source("nbr_build.hip")
    assert shifted(build, "kMaxGrid") == oc.GRID
    assert constant(build, "kRuleWaves") == oc.RULE_WAVES == 4
    assert "unsigned row_grid(int64_t rows) { return (unsigned)std::max<int64_t>(1, std::min(ceil_div(rows, kRuleWaves), kMaxGrid)); }" in build
    assert oc.ROW_GRID_ROWS == oc.RULE_WAVES * oc.GRID < oc.BIG_ROWS
    for kernel, grid, n in (("nbr_rule_kernel", "row_grid(m)", "A.m"), ("nbr_compact_kernel", "row_grid(n_rows)", "n_rows"),
                            ("nbr_bound_kernel", "row_grid(T1.n_rows)", "n_rows1")):
        assert re.findall(r"%s<<<\s*dim3\(([^)]*\))\)" % kernel, build) == [grid], kernel
        body = function_body(build, "void %s(" % kernel)
        assert "const int64_t nw = (int64_t)gridDim.x * kRuleWaves;" in body
        assert re.search(r"for \(int64_t (\w) = \(int64_t\)blockIdx\.x \* kRuleWaves \+ \(threadIdx\.x >> 6\); \1 < %s; \1 \+= nw\) \{"
                         % re.escape(n), body), kernel
    # the dense searches hand the rule one block at a time, and no block reaches the cap: 65,535 queries of the scan, 2^20 of the
    # MFMA path's chunks
    assert "return std::max<int64_t>(1, std::min<int64_t>(b, 65535));" in function_body(source("topk.hip"), "int64_t topk_scan_block_queries(")
    assert shifted(source("topk_plan.hpp"), "kChunkQ") == 1 << 20 < oc.ROW_GRID_ROWS
    assert "for (int64_t c0 = 0; c0 < nq; c0 += kChunkQ) {" in source("topk_mfma.hip")


def test_scan_holds_what_the_tests_assume():
    scan = source("csr_scan.hpp")
    assert "constexpr int kScanThreads = 256, kScanPer = 8;" in scan
    launch = function_body(scan, "inline int32_t csr_exclusive_scan(")
    assert "const int64_t per = (int64_t)kScanThreads * kScanPer, nb = gorse::ceil_div(n, per);" in launch
    assert 256 * 8 == oc.SCAN_TILE
    assert "nbr_scan_top_kernel<<<dim3(1), dim3(kScanThreads), 0, st>>>(sums.p, nb);" in launch
    assert "for (int64_t b0 = 0; b0 < nb; b0 += kScanThreads) {" in function_body(scan, "void nbr_scan_top_kernel(")
    assert oc.SCAN_TOP == 256 and oc.SCAN_ONE_TOP_PASS == oc.SCAN_TILE * oc.SCAN_TOP == 524_288
    for text, call in ((source("cand.hip"), "csr_exclusive_scan((long long *)c->cur_ptr[other].p, nq + 1, c->sums, st)"),
                       (source("cand.hip"), "csr_exclusive_scan((long long *)c->f_ptr.p, nq + 1, c->sums, st)"),
                       (source("nbr_build.hip"), "csr_exclusive_scan((long long *)ptr.p, ns, sums, st)")):
        assert '#include "csr_scan.hpp"' in text and call in text
    assert "const int64_t ns = n_rows + 1;" in source("nbr_build.hip")
    # nq + 1 counts: 524,287 queries are the last shape of one pass of the top kernel, 524,288 the first with a carry
    assert -(-(524_287 + 1) // oc.SCAN_TILE) == oc.SCAN_TOP and -(-(524_288 + 1) // oc.SCAN_TILE) == oc.SCAN_TOP + 1
    assert -(-(oc.BIG_NQ + 1) // oc.SCAN_TILE) == 2049 == -(-(oc.BIG_ROWS + 1) // oc.SCAN_TILE)


def test_recommend_launch_chunk_is_what_the_tests_assume():
    rec = source("recommend.hip")
    _, _, groups = group_geometry()
    scratch = shifted(rec, "kRecScratchBytes")
    assert scratch == 256 << 20
    assert constant(rec, "kRecMaxSlices") == oc.REC_MAX_SLICES == oc.REC_HOOK[0]
    assert "g_rec_slices = slices > 0 ? std::min<int32_t>(slices, kRecMaxSlices) : 0;" in rec
    core = function_body(rec, "int32_t mf_recommend_core(")
    for line in ("A.kk = k + 1;", "A.cap = std::max(32, 2 * A.kk);", "if (g_rec_buffer > 0) A.cap = std::max(A.kk + 1, g_rec_buffer);",
                 "if (g_rec_slices > 0) slices = g_rec_slices;", "slices = (int)std::min<int64_t>(slices, I);",
                 "A.slice_len = (int32_t)ceil_div(I, slices);",
                 "int64_t chunk = (int64_t)(kRecScratchBytes / per_query) / kGroupsPerBlock * kGroupsPerBlock;",
                 "chunk = std::min<int64_t>(std::max<int64_t>(chunk, kGroupsPerBlock), n_users);",
                 "for (int64_t q0 = 0; q0 < n_users; q0 += chunk) {"):
        assert line in core, line
    expr = re.search(r"const size_t per_query = ([^;]+);", core).group(1)
    k = oc.REC_HOOK_K
    kk = k + 1
    cap = max(kk + 1, oc.REC_HOOK[1])
    per_query = eval(expr.replace("(size_t)", "").replace("A.", ""), {"__builtins__": {}}, {"slices": oc.REC_HOOK[0], "cap": cap, "kk": kk, "k": k})
    assert per_query == 1_049_408
    assert scratch // per_query // groups * groups == oc.REC_HOOK_CHUNK == 240
    # I = 17 in 8 slices: slices of 3 items, and the last two begin past the end
    assert -(-17 // 8) == 3 and 6 * 3 > 17


def test_the_tests_named_above_exist():
    past = source("test_gpu_offline_past_one_grid.py", TESTS)
    named = set(re.findall(r"\b(test_\w+)\b(?!\.py)", __doc__))
    assert len(named) == 10
    for name in named:
        assert "def %s(" % name in past, name


# ---- the restatements over padded arrays ---------------------------------------------------------------------------------------

def same_result(got, want, what):
    for s, (g, w) in enumerate(zip(got.excl, want.excl)):
        oc.assert_csr(g, w, ("exclusion row pointer", "exclusion rows"), (what, "after stage %d" % (s - 1)))
    oc.assert_csr(got.finished, want.finished, ("row pointer", "items", "score bits", "stage numbers"), what)


def small_case(seed):
    """400 queries over 30 items: base rows of 0 .. 4 (repeats), lists of 0 .. 6 (repeats) cut at 3, a shared list of 8 cut at 2
    under a keep, another keep at finish, and three marked queries with long rows"""
    rng = np.random.default_rng(seed)
    nq, n_items = 400, 30
    base, base_len = rng.integers(0, n_items, (nq, 4)).astype(np.int32), rng.integers(0, 5, nq)
    items, lens = rng.integers(0, n_items, (nq, 6)).astype(np.int32), rng.integers(0, 7, nq)
    scores = rng.normal(0, 1, (nq, 6))
    marked = {int(t): (rng.integers(0, n_items, 70).tolist(), [(int(j), float(j)) for j in rng.permutation(n_items)])
              for t in rng.choice(nq, 3, replace=False)}
    keep_shared, keep_finish = (rng.random(n_items) < 0.7).astype(np.uint8), (rng.random(n_items) < 0.7).astype(np.uint8)
    shared = (rng.choice(n_items, 8, replace=False), rng.normal(0, 1, 8))
    keep_shared[shared[0][:2]] = (0, 1)
    return oc.ChainCase(nq, n_items, 5, 3, 2, lambda t: (base[t], base_len[t]), lambda t: (items[t], scores[t], lens[t]), shared,
                        keep_shared, keep_finish, marked)


def test_padded_chain_equals_the_reference_on_small_shapes():
    for seed in range(5):
        case = small_case(seed)
        q = np.arange(case.nq)
        got, want = oc.expected_chain(case), oc.chain_by_reference(case, q)
        same_result(got, want, seed)
        # the shapes hold what they are meant to: lists with excluded items, lists cut at k, items dropped by either keep
        base, blen = case.base_of(q)
        items, _, lens = case.lists_of(q)
        plain = ~case.is_marked(q)
        hit = [t for t in q[plain] if set(items[t, :lens[t]]) & set(base[t, :blen[t]])]
        first = np.diff(want.excl[1][0]) - np.diff(want.excl[0][0])
        assert hit and (first[plain] == case.k_lists).any() and (lens[plain][first[plain] == case.k_lists] > case.k_lists).any()
        assert got.info[2][2] > got.info_finished[2] > 0 and got.info[1][2] < got.info[2][2]
        # the CSRs handed to the device are the rows the reference walked
        ptr, flat = case.base_csr()
        assert np.array_equal(np.diff(ptr), np.diff(want.excl[0][0]))
        assert all(np.array_equal(np.sort(flat[ptr[t]:ptr[t + 1]]), want.excl[0][1][ptr[t]:ptr[t + 1]]) for t in q)
        lp, li, ls = case.lists_csr()
        assert lp[-1] == lens[plain].sum() + sum(len(m[1]) for m in case.marked.values()) and li.size == ls.size == lp[-1]


def test_padded_chain_equals_the_reference_on_the_tiny_rows_case():
    case = oc.tiny_rows_case(3000)
    same_result(oc.expected_chain(case), oc.chain_by_reference(case, np.arange(case.nq)), "tiny rows")


def test_padded_chain_equals_the_reference_on_a_sample_of_the_big_case():
    case = oc.big_chain_case()
    rng = np.random.default_rng(1)
    q = np.unique(np.concatenate([case.marked_at, rng.choice(case.nq, 3000, replace=False)]))
    same_result(oc.expected_chain(case, q), oc.chain_by_reference(case, q), "sample of the big case")
    # what the big case promises
    g = oc.GRID
    assert set([0, 1, g - 1, g, g + 1, 2 * g, 4 * g - 1, 4 * g, 4 * g + 1, case.nq - 1]) <= set(case.marked) and len(case.marked) >= 195
    assert len(case.marked[1][0]) == 4097 and len(case.marked[g + 1][0]) == 300  # a global-memory sort, then an LDS sort, one workgroup
    assert {len(m[0]) for m in case.marked.values()} == set(oc.MARKED_LENGTHS)
    assert all(m[0] != sorted(m[0]) and len(set(m[0])) < len(m[0]) for m in case.marked.values())
    assert {len(m[1]) for m in case.marked.values()} >= {0, 1, 256}
    base, blen = case.base_of(q)
    _, _, lens = case.lists_of(q)
    assert set(blen.tolist()) == {0, 1, 2} and set(lens.tolist()) == {0, 1, 2, 3}
    assert (base[blen == 2, 0] > base[blen == 2, 1]).any() and (base[blen == 2, 0] < base[blen == 2, 1]).any()


def test_expanded_table_equals_the_reference():
    rng = np.random.default_rng(2)
    index_n, n = 50, 3
    lists = {}
    for s in range(index_n):
        c = int(rng.integers(0, n + 2))
        idx = rng.choice(index_n, n + 1, replace=False).astype(np.int32)
        if s % 3 == 0 and c:
            idx[int(rng.integers(0, c))] = s  # the row itself in its list
        lists[s] = (idx, rng.normal(0.2, 1.0, n + 1).astype(np.float32), c)
    stored = B.table_from_lists(range(index_n), lists, n, True)
    sources = rng.integers(-1, index_n, 700)
    sources[[0, 699]] = (-1, 7)
    want = B.table_from_lists(sources, lists, n, True)
    got = oc.expand_table(*stored, sources)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32)) and 0 < want[0][-1] < 700 * n


def test_table_sources_are_where_the_tests_say():
    for n_rows in (2047, 2048, 2049, 4097):
        src = oc.edge_sources(n_rows, 333)
        assert 250 <= (src >= 0).sum() <= 300 and src.max() < 333 and src[0] >= 0 and src[-1] >= 0
        assert all(src[m - 1] >= 0 and src[m] >= 0 for m in range(oc.SCAN_TILE, n_rows, oc.SCAN_TILE))
    src = oc.big_sources(421)
    g4 = oc.ROW_GRID_ROWS
    assert src.size == oc.BIG_ROWS == g4 + 101 and (src < 0).sum() == 64 and src.max() == 420
    assert src[1] < 0 and src[-1] < 0 and (src[g4 - 8:g4] < 0).any() and (src[g4:g4 + 8] < 0).any()
    valid = np.flatnonzero(src >= 0)
    both = (src[:-4] >= 0) & (src[4:] >= 0)  # row r and row r + 4, the same wave slot of the next workgroup, name different sources
    assert (src[valid] != valid).mean() > 0.99 and (src[:-4][both] != src[4:][both]).all()
    rows = oc.big_sample_rows()
    assert 35 <= rows.size <= 45 and rows.max() < oc.BIG_ROWS and {0, oc.BIG_ROWS - 1, g4 - 1, g4} <= set(rows.tolist())
    assert (src[rows] < 0).sum() >= 4
