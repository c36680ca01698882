"""The grid caps that tests/test_gpu_cf_past_one_grid.py sizes its inputs from (the GRID_* literals of tests/cf_cases.py), held against
the launchers' own text (no GPU): a cap raised later fails here instead of silently leaving a kernel's grid-stride loop unvisited again.

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
    bpr = source("bpr.hip")
    # user runs: a run per group, two at nFactors 8 while GORSE_BPR_D8_PAIRS is on
    users = function_body(bpr, "int32_t launch_update_users(gorse_mf *h")
    assert "int64_t blocks = ceil_div(h->U, (int64_t)kGroupsPerBlock * (d == 8 && GORSE_BPR_D8_PAIRS ? 2 : 1));" in users
    cap = re.search(r"const int64_t capb = ([\d *]+);\s*if \(blocks > capb\) blocks = capb;", users)
    assert product(cap.group(1)) * groups == cc.GRID_USER_RUNS == 65_536
    assert re.search(r"#define GORSE_BPR_D8_PAIRS 1\b", bpr) and "dim3 grid((unsigned)blocks), block(kBlock);" in users
    assert 2 * cc.GRID_USER_RUNS == cc.GRID_USER_RUNS_D8 == 131_072
    kernel = function_body(bpr, "void bpr_update_user_kernel(")
    assert "const int64_t ngroups = (int64_t)((int)gridDim.x - folders) * kGroupsPerBlock * SUBS;" in kernel
    assert "for (int64_t u = group; u < U; u += ngroups) {" in kernel
    # per-sample schedule: a sample per group
    mode = function_body(bpr, "int32_t launch_update_mode(gorse_mf *h")
    assert "int64_t blocks = ceil_div(n, kGroupsPerBlock);" in mode
    cap = re.search(r"const int64_t cap = ([\d *]+);[^\n]*\n\s*if \(blocks > cap\) blocks = cap;", mode)
    assert product(cap.group(1)) * groups == cc.GRID_SAMPLES == 65_536
    # its fold kernel: an element of a hot or accumulated row per thread
    fold = re.search(r"ceil_div\(\(int64_t\)\(hot\.n_hot \+ hot\.n_acc\) \* d, (\d+)\), (\d+)\);\s*hipExtLaunchKernelGGL\(bpr_fold_kernel, "
                     r"dim3\(\(unsigned\)fb\), dim3\((\d+)\)", mode)
    assert fold.group(1) == fold.group(3) and int(fold.group(2)) * int(fold.group(3)) == cc.GRID_FOLD_ELEMENTS == 131_072
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
    bpr = source("bpr.hip")
    sort = function_body(bpr, "int32_t launch_user_sort(")
    cap = re.search(r"const int64_t blocks = std::min<int64_t>\(ceil_div\(n, (\d+)\), ([\d *]+)\);", sort)
    assert sort.count("<<<dim3((unsigned)blocks), dim3(%s)" % cap.group(1)) == 2  # bpr_rank_kernel, bpr_scatter_by_kernel
    assert int(cap.group(1)) * product(cap.group(2)) == cc.GRID_SORT_SAMPLES == 524_288
    scan = function_body(bpr, "int32_t exclusive_scan_i32(")
    tiles = re.search(r"if \(nt <= (\d+)\) \{\s*scan_small_kernel", scan)
    assert "const int64_t nt = ceil_div(m, kScanTile);" in scan
    assert int(tiles.group(1)) * constant(bpr, "kScanTile") == cc.SCAN_ONE_WORKGROUP == 32_768


def test_the_tests_named_above_exist():
    past = source("test_gpu_cf_past_one_grid.py", TESTS)
    named = set(re.findall(r"\b(test_\w+)\b(?!\.py)", __doc__))
    assert len(named) == 9
    for name in named:
        where = source("test_gpu_cf_parity.py", TESTS) if name.startswith("test_prepared_chunk") else past
        assert "def %s(" % name in where, name
