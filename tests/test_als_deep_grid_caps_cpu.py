"""The caps that tests/test_gpu_als_deep_past_one_grid.py sizes its data from (GRID_ALS_DEEP_ITEMS and ALS_GRAM_CHUNK_ROWS of
tests/cf_cases.py), held against the launchers' and the plan's own text (no GPU): a cap raised later fails here instead of silently
leaving a strided loop's second step, a Gram of several chunks or the reduce's eight-wide step unvisited again.

  launcher (kernel)                                       one step holds                      crossed by
  deep_launch (als_deep_kernel<NB, false>, the short      2048 rows, a workgroup each         test_tall_half_sweeps_meet_the_float64_gram_solve,
    rows)                                                                                     test_rows_solved_on_a_later_trip_equal_the_rows_of_a_one_grid_range
  deep_launch (als_deep_kernel<NB, true>, the long rows'  2048 chunks, a workgroup each       the same two (both sides),
    chunks)                                                                                   test_two_handles_one_tall_epoch_same_bits
  the k.solve launch (als_deep_long_kernel<NB>)           2048 long rows, a workgroup each    the same three (user side)
  als_build_plan's Gram chunks (als_deep_kernel<NB,       1024 rows with feedback per chunk   the same three (item half-sweeps: nine chunks),
    true> over fb_rows, als_deep_reduce_kernel)                                               test_the_gram_skips_the_empty_users
  als_deep_reduce_kernel's unrolled loop                  eight partials per step             the same (nine Gram chunks; item rows of 8 k and
                                                                                              8 k + r chunks)

test_the_tall_data_is_past_every_cap derives, from the data and a restatement of the plan rule, that each of these is crossed."""
import re

import cf_cases as cc
from test_mf_grid_caps_cpu import TESTS, constant, function_body, source


def test_deep_grids_hold_what_the_tests_assume():
    deep = source("als_deep.hip")
    cap = "std::min<int64_t>(%%s, %d)" % cc.GRID_ALS_DEEP_ITEMS
    assert cc.GRID_ALS_DEEP_ITEMS == 2048
    # every row and chunk launch goes through deep_launch: a workgroup per item up to the cap, and the kernel strides by its grid
    launch = function_body(deep, "int32_t deep_launch(K kernel")
    assert "kernel<<<dim3((unsigned)%s), dim3(256), deep_lds_bytes(nb), st>>>(" % (cap % "items") in launch
    sweep = function_body(deep, "int32_t als_deep_half_epoch(")
    assert re.findall(r"deep_launch\(k\.(\w+), ([\w.]+),", sweep) == [("chunk", "gp.n_gchunks"), ("row", "pl.n_short"), ("chunk", "pl.n_chunks")]
    assert re.findall(r"(\w[\w.]*)<<<", sweep) == ["k.solve"] and deep.count("als_deep_kernel<<<") == 0
    assert "k.solve<<<dim3((unsigned)%s), dim3(256), deep_lds_bytes(nb), h->stream>>>(" % (cap % "pl.n_long") in sweep
    assert "for (int64_t t = blockIdx.x; t < n_items; t += gridDim.x) {" in function_body(deep, "void als_deep_kernel(")
    assert "for (int64_t t = blockIdx.x; t < n_rows; t += gridDim.x) {" in function_body(deep, "void als_deep_long_kernel(")
    # the reduce: eight partials per step, then a tail; one row of n_gchunks partials for S, a row per long row otherwise
    reduce = function_body(deep, "void als_deep_reduce_kernel(")
    assert "for (; c + 7 < nc; c += 8) {" in reduce and "for (; c < nc; c++) acc += src[(int64_t)c * stride];" in reduce
    assert "const int nc = first ? nch[t] : nch_all;" in reduce
    assert "nullptr, nullptr, 1, (int)gp.n_gchunks, stride" in sweep and "pl.long_first.p, pl.long_nch.p, pl.n_long, 0, stride" in sweep
    # the gather batch that the row lengths 31 / 32 / 33 of tests/test_gpu_als_deep.py stand around
    assert constant(source("als_deep_plan.hpp"), "kDeepBatch") == 32


def test_plan_rule_is_what_the_tests_restate():
    build = function_body(source("als.hip"), "int32_t als_build_plan(")
    assert int(re.search(r"constexpr int64_t kGramChunk = (\d+);", build).group(1)) == cc.ALS_GRAM_CHUNK_ROWS == 1024
    for line in ("int64_t long_row = g_als_long_row, chunk_len = g_als_chunk;", "if (n <= long_row) {",
                 "const int64_t chunk = std::max<int64_t>(chunk_len, (ceil_div(n, 256) + 15) / 16 * 16);",
                 "for (int64_t b = 0; b < n; b += chunk, nc++) {", "if (ptr[r + 1] > ptr[r]) fbr.push_back((int32_t)r);",
                 "for (int64_t b = 0; b < (int64_t)fbr.size(); b += kGramChunk) {",
                 "gcnt.push_back((int32_t)std::min<int64_t>(kGramChunk, (int64_t)fbr.size() - b));"):
        assert line in build, line
    # the restatement itself, on lengths around the rule's edges
    import test_gpu_als_deep_past_one_grid as tall
    n_short, n_long, nch = tall.plan([0, 1, 16, 17, 32, 33, 256 * 16, 256 * 16 + 1])
    assert (n_short, n_long) == (3, 5) and nch.tolist() == [2, 2, 3, 256, 129]  # (past 4096 entries a chunk is 32: at most 256 chunks a row)
    assert tall.gram_chunks([1] * 2049 + [0] * 5) == [1024, 1024, 1] and tall.gram_chunks([0, 0]) == []


def test_the_tests_named_above_exist():
    past = source("test_gpu_als_deep_past_one_grid.py", TESTS)
    named = set(re.findall(r"\b(test_\w+)\b(?!\.py)", __doc__))
    assert len(named) == 5
    for name in named:
        assert "def %s(" % name in past, name
