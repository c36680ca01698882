"""The grid caps that tests/test_gpu_cf_past_one_grid.py sizes its inputs from (the GRID_* literals of tests/cf_cases.py), held against
the launchers' own text (no GPU): a cap raised later fails here instead of silently leaving a kernel's grid-stride loop unvisited again.
The BPR launchers (csrc/bpr_update_users.hip, csrc/bpr_update.hip, csrc/bpr_prepare.hip; named below without their bpr_ prefix) take
their grids from csrc/bpr_plan.hpp: the text read here is the plan function's and the launcher's call of it.

Every capped launch of the matrix-factorisation sources, what one grid of it holds, and the test that gives it more:

  launcher (kernel)                                        one grid holds                    crossed by
  launch_update_users (bpr_update_user_kernel)             65,536 user runs; 131,072 at      test_bpr_user_runs_past_one_grid_equal_the_sequential_result,
                                                           nFactors 8                        test_bpr_user_runs_store_route_past_one_grid
  launch_update_mode (bpr_update_kernel)                   65,536 samples                    test_bpr_per_sample_conflict_free_batch_past_one_grid
  mf_score_device (mf_score_kernel)                        131,072 pairs                     test_score_bit_exact_past_one_grid
  mf_rank_device (expand_users_kernel)                     4,096 lists                       test_rank_exact_past_one_grid_of_lists
  mf_delta_export_async / _import_async (delta_*_kernel)   2,097,152 floats                  test_item_delta_exchange_past_one_grid

and the caps that only an epoch or a whole chunk reaches (smallest shape past the cap; the test that crosses it):

  launch_user_sort (bpr_rank_kernel, bpr_scatter_by_kernel): 524,288 samples; a chunk of 524,289 triplets sorted by user without the
      stable-rank hook (gorse_bpr_apply_triplets on the user-run schedule -- an epoch sorts this way only under that hook, by one
      thread).  No earlier test went there: test_bpr_user_sort_past_one_grid (524,588 samples).
  launch_sampler (bpr_sample_kernel) and the unbinned preparation of launch_prepare_users (bpr_sample_user_kernel,
      bpr_scatter_ids_kernel, bpr_sample_items_kernel), the same 256 * 8 workgroups x 256 threads = 524,288 samples; a chunk of
      524,289.  Crossed by tests/test_gpu_cf_parity.py::test_prepared_chunk_binned_and_unbinned_on_many_users (1,500,000 samples,
      through gorse_bpr_sample_triplets and, under variant bit 21, the preparation without bins).
  bpr_fold_kernel: 512 workgroups x 256 threads = 131,072 elements of hot or accumulated rows; (hot + accumulated slots) x nFactors
      > 131,072 on the per-sample schedule, which at most 1024 hot slots reach from nFactors 129 on.  No earlier test went there
      (S-ml1m: 926 slots x 128 at most; the wide-factor tests: 50 slots): test_bpr_fold_kernel_past_one_grid (1024 x 129 = 132,096).
  exclusive_scan_i32: scan_small_kernel for up to 16 tiles of 2048 = 32,768 counters, three kernels (tile sums, scan of the sums,
      rescan) beyond; U + 2 > 32,768 counters, that is 32,767 users on a path that scans run counters.  Crossed by
      test_prepared_chunk_binned_and_unbinned_on_many_users under variant bit 21 (300,002 counters) and by every user-run test of
      test_gpu_cf_past_one_grid.py (65,575 and 131,111 counters through launch_user_sort)."""
import os
import re

import cf_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gorse_amd", "csrc")
TESTS = os.path.join(ROOT, "tests")


def source(name, where=CSRC):
    with open(os.path.join(where, name)) as f:
        return f.read()


def function_body(text, head):
    at = text.index(head)
    return text[at:text.index("\n}\n", at)]


def product(expr):
    """the value of `256 * 16`, `2048`, ..."""
    out = 1
    for x in re.findall(r"\d+", expr):
        out *= int(x)
    return out


def constant(text, name):
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


def group_geometry():
    dev = source("cf_device.hpp")
    k_group, k_block = constant(dev, "kGroup"), constant(dev, "kBlock")
    assert "constexpr int kGroupsPerBlock = kBlock / kGroup;" in dev
    return k_group, k_block, k_block // k_group


def test_group_kernels_hold_what_the_tests_assume():
    k_group, k_block, groups = group_geometry()
    assert (k_group, k_block, groups) == (16, 256, 16)
    # the BPR launches take their grids from csrc/bpr_plan.hpp (whose values tests/cpp/bpr_plan_main.cpp checks one by one)
    plan = source("bpr_plan.hpp")
    assert constant(plan, "kRunsPerBlock") == groups and "static_assert(kRunsPerBlock == kGroupsPerBlock" in source("bpr_internal.hpp")
    blocks = product(re.search(r"constexpr int64_t kUpdateBlocks = ([\d *]+);", plan).group(1))
    # user runs: a run per group, two at nFactors 8 while GORSE_BPR_D8_PAIRS is on
    users_unit = source("bpr_update_users.hip")
    users = function_body(users_unit, "int32_t gorse::bpr_launch_update_users(gorse_mf *h")
    assert "int64_t blocks = bpr_user_run_workers(h->U, d, GORSE_BPR_D8_PAIRS);" in users
    workers = function_body(plan + "\n}\n", "inline int64_t bpr_user_run_workers(int64_t U, int d, bool d8_pairs) {")
    assert "const int64_t per = (int64_t)kRunsPerBlock * (d == 8 && d8_pairs ? 2 : 1);" in workers
    assert "return std::min<int64_t>((U + per - 1) / per, kUpdateBlocks);" in workers
    assert blocks * groups == cc.GRID_USER_RUNS == 65_536
    assert re.search(r"#define GORSE_BPR_D8_PAIRS 1\b", users_unit) and "dim3 grid((unsigned)blocks), block(kBlock);" in users
    assert 2 * cc.GRID_USER_RUNS == cc.GRID_USER_RUNS_D8 == 131_072
    kernel = function_body(users_unit, "void bpr_update_user_kernel(")
    assert "const int64_t ngroups = (int64_t)((int)gridDim.x - folders) * kGroupsPerBlock * SUBS;" in kernel
    assert "for (int64_t u = group; u < U; u += ngroups) {" in kernel
    # per-sample schedule: a sample per group
    sample_unit = source("bpr_update.hip")
    mode = function_body(sample_unit, "int32_t launch_update_mode(gorse_mf *h")
    assert "int64_t blocks = bpr_sample_workers(n);" in mode and "dim3 grid((unsigned)blocks), block(kBlock);" in mode
    assert ("inline int64_t bpr_sample_workers(int64_t n) { return std::min<int64_t>((n + kRunsPerBlock - 1) / kRunsPerBlock, kUpdateBlocks); }"
            in plan)
    assert blocks * groups == cc.GRID_SAMPLES == 65_536
    kernel = function_body(sample_unit, "void bpr_update_kernel(")
    assert "const int64_t ngroups = (int64_t)((int)gridDim.x - folders) * kGroupsPerBlock;" in kernel
    assert "for (int64_t s = begin + group; s < end; s += ngroups) {" in kernel
    # its fold kernel: an element of a hot or accumulated row per thread
    assert "const int64_t fb = bpr_fold_grid(hot.n_hot, hot.n_acc, d);" in mode
    assert "hipExtLaunchKernelGGL(bpr_fold_kernel, dim3((unsigned)fb), dim3(kFoldThreads)" in mode
    fold = re.search(r"return std::min<int64_t>\(\(\(int64_t\)\(n_hot \+ n_acc\) \* d \+ kFoldThreads - 1\) / kFoldThreads, (\d+)\);",
                     function_body(plan + "\n}\n", "inline int64_t bpr_fold_grid(int n_hot, int n_acc, int d) {"))
    assert int(fold.group(1)) * constant(plan, "kFoldThreads") == cc.GRID_FOLD_ELEMENTS == 131_072
    assert "w < work; w += (int64_t)gridDim.x * blockDim.x) {" in function_body(sample_unit, "void bpr_fold_kernel(")
    # score: a pair per group
    rank = source("mf_rank.hip")
    score = function_body(rank, "int32_t gorse::mf_score_device(")
    assert "int64_t blocks = ceil_div(n, kGroupsPerBlock);" in score and "block(kBlock)" in score
    cap = re.search(r"if \(blocks > ([\d *]+)\) blocks = ([\d *]+);", score)
    assert product(cap.group(1)) == product(cap.group(2)) and product(cap.group(1)) * groups == cc.GRID_SCORE_PAIRS == 131_072
    # rank: a workgroup of expand_users_kernel per list
    lists = function_body(rank, "int32_t gorse::mf_rank_device(")
    cap = re.search(r"int64_t eb = n_users < (\d+) \? n_users : (\d+);\s*expand_users_kernel<<<dim3\(\(unsigned\)eb\)", lists)
    assert int(cap.group(1)) == int(cap.group(2)) == cc.GRID_RANK_LISTS == 4_096


def test_flat_kernels_hold_what_the_tests_assume():
    mf = source("mf.hip")
    for head, kernel in (("int32_t gorse::mf_delta_export_async(", "delta_export_kernel"),
                         ("int32_t gorse::mf_delta_import_async(", "delta_import_kernel")):
        body = function_body(mf, head)
        cap = re.search(r"std::min<int64_t>\(ceil_div\(n4, (\d+)\), (\d+)\);\s*%s<<<dim3\(\(unsigned\)blocks\), dim3\((\d+)\)" % kernel, body)
        assert cap.group(1) == cap.group(3)
        assert int(cap.group(2)) * int(cap.group(3)) * 4 == cc.GRID_DELTA_FLOATS == 2_097_152  # a float4 per thread
    # the flat kernels of the BPR preparation: the grid is csrc/bpr_plan.hpp's, for every launch of them
    plan, prep = source("bpr_plan.hpp"), source("bpr_prepare.hip")
    cap = re.search(r"inline int64_t bpr_flat_grid\(int64_t n\) \{ return std::min<int64_t>\(\(n \+ kFlatThreads - 1\) / kFlatThreads, ([\d *]+)\); \}",
                    plan)
    sort = function_body(prep, "int32_t gorse::bpr_launch_user_sort(")
    assert "const int64_t blocks = bpr_flat_grid(n);" in sort
    assert sort.count("<<<dim3((unsigned)blocks), dim3(kFlatThreads)") == 2  # bpr_rank_kernel, bpr_scatter_by_kernel
    assert constant(plan, "kFlatThreads") * product(cap.group(1)) == cc.GRID_SORT_SAMPLES == 524_288
    for head in ("int32_t gorse::bpr_launch_sampler(", "int32_t gorse::bpr_launch_prepare_users("):
        body = function_body(prep, head)
        assert "blocks = bpr_flat_grid(n);" in body and "dim3((unsigned)blocks), dim3(kFlatThreads)" in body, head
    for kernel in ("bpr_sample_kernel", "bpr_sample_user_kernel", "bpr_scatter_ids_kernel", "bpr_sample_items_kernel", "bpr_rank_kernel",
                   "bpr_scatter_by_kernel"):
        assert re.search(r"< n; \w \+= \(int64_t\)gridDim\.x \* blockDim\.x\)", function_body(prep, "void %s(" % kernel)), kernel
    scan = function_body(prep, "int32_t exclusive_scan_i32(")
    assert re.search(r"if \(bpr_scan_one_workgroup\(m\)\) \{\s*scan_small_kernel", scan) and "const int64_t nt = bpr_scan_tiles(m);" in scan
    assert "inline int64_t bpr_scan_tiles(int64_t m) { return (m + kScanTile - 1) / kScanTile; }" in plan
    assert "inline bool bpr_scan_one_workgroup(int64_t m) { return bpr_scan_tiles(m) <= kScanSmallTiles; }" in plan
    assert constant(plan, "kScanSmallTiles") * constant(plan, "kScanTile") == cc.SCAN_ONE_WORKGROUP == 32_768


def test_the_tests_named_above_exist():
    past = source("test_gpu_cf_past_one_grid.py", TESTS)
    named = set(re.findall(r"\b(test_\w+)\b(?!\.py)", __doc__))
    assert len(named) == 9
    for name in named:
        where = source("test_gpu_cf_parity.py", TESTS) if name.startswith("test_prepared_chunk") else past
        assert "def %s(" % name in where, name
