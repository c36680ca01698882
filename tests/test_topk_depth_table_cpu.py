"""The tables of tests/topk_cases.py held against the kernels' sources (no GPU): every operand depth path B's sweep is instantiated for
(kSupportedKP in csrc/topk_plan.hpp and the cases of dispatch_sweep in csrc/topk_sweep.hip) is named by the depth tests in both dtypes,
so that a depth added later cannot arrive untested, and the widths of the wide-row tests contain both sides of every edge of
csrc/topk.hip's scan_groups.  The rules of csrc/topk_plan.hpp themselves -- the sweep's launch geometry at every instantiated shape,
the depth rule, the symmetric form's predicate, the triangle's geometry, the slice and queries-per-wave rules -- are checked by value
in tests/cpp/topk_plan_main.cpp, which is built and run here under AddressSanitizer and UBSan."""
import os
import re
import shutil
import subprocess

import pytest

import topk_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gorse_amd", "csrc")


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def function_body(text, head):
    at = text.index(head)
    return text[at:text.index("\n}\n", at)]


def ints(s):
    return [int(x) for x in re.findall(r"\d+", s)]


@pytest.mark.skipif(shutil.which("g++") is None and shutil.which("clang++") is None, reason="no host C++ compiler")
def test_plan_rules_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    exe = str(tmp_path / "topk_plan")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "cpp", "topk_plan_main.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "topk_plan ok" in out.stdout


def test_depth_table_names_every_instantiated_depth_in_both_dtypes():
    plan = source("topk_plan.hpp")
    supported = ints(re.search(r"kSupportedKP\[\]\s*=\s*\{([^}]*)\}", plan).group(1))
    dispatched = ints(" ".join(re.findall(r"case (\d+):", function_body(source("topk_sweep.hip"), "int32_t gorse::dispatch_sweep("))))
    assert supported == sorted(supported) and supported == dispatched == list(tc.SUPPORTED_KP)
    # the depth of an index as topk_mfma_prepare derives it (operand_depth, whose values tests/cpp/topk_plan_main.cpp checks at the
    # same widths), restated by topk_cases.expected_kp
    depth = function_body(plan, "inline int operand_depth(")
    assert "((bf16 ? d : 3 * (int64_t)d) + 15) / 16" in depth and "if (c >= need) return c;" in depth
    assert "const int kp = operand_depth(bf, d);" in function_body(source("topk_mfma.hip"), "int32_t topk_mfma_prepare(")
    assert [tc.expected_kp(tc.BF16, d) for d in (1, 16, 17, 80, 81, 384, 385)] == [1, 1, 2, 6, 6, 24, None]
    assert [tc.expected_kp(tc.F32, d) for d in (1, 5, 6, 42, 43, 128, 129)] == [1, 1, 2, 8, 12, 24, None]
    for dtype in (tc.F32, tc.BF16):
        reached = {tc.expected_kp(t, d) for t, d in tc.DEPTH_CASES if t == dtype}
        assert reached == set(supported), (dtype, sorted(set(supported) - reached))
    # bf16: the index as its own operand matrix (d == 16 KP) and operand rows that end in zeros, at every depth
    for kp in supported:
        forms = {tc.operand_form(t, d) for t, d in tc.DEPTH_CASES if t == tc.BF16 and tc.expected_kp(t, d) == kp}
        assert "padded" in forms, kp
        assert "aliased" in forms or kp == 8, kp  # d = 128 (KP 8 aliased) is tests/test_gpu_topk_mfma.py's main shape
    # whole k-steps of zeros above KP 1: the narrowest row of a depth, in either dtype
    for kp in supported[1:]:
        prev = supported[supported.index(kp) - 1]
        assert any(tc.expected_kp(t, d) == kp and (d if t == tc.BF16 else 3 * d) <= 16 * (prev + 1) for t, d in tc.DEPTH_CASES), kp
    assert {tc.expected_kp(*c) for c in tc.DEPTH_K100} == {kp for kp in supported if kp >= 12}
    deepest = max(supported)
    assert set(tc.TOO_DEEP_CASES) == {(tc.BF16, 16 * deepest + 1), (tc.F32, 16 * deepest // 3 + 1)}
    assert all(tc.expected_kp(*c) is None for c in tc.TOO_DEEP_CASES)


def test_tie_cases_name_every_history_sweep_shape():
    text = source("topk_plan.hpp")
    supported = ints(re.search(r"kSupportedKP\[\]\s*=\s*\{([^}]*)\}", text).group(1))
    dma = ints(re.search(r"constexpr bool sweep_hist_dma\(int kp\) \{ return ([^;]*); \}", text).group(1))
    waves = re.search(r"constexpr int sweep_waves\(bool hist, int kp\) \{ return ([^;]*); \}", text).group(1)
    assert waves == "!hist || sweep_hist_dma(kp) ? kWavesMain : (kp <= 8 ? 2 : (kp <= 12 ? 4 : 8))"
    # the depths whose history sweep is not the main sweep's DMA form; KP 1 (two waves) is test_gpu_topk_mfma.py's d 4 / 6 / 8 in fp32
    own_form = [kp for kp in supported if kp not in dma and kp > 1]
    assert sorted(tc.expected_kp(*c) for c in tc.TIE_CASES) == own_form == [3, 6, 12, 16, 24]
    assert {t for t, _ in tc.TIE_CASES} == {tc.F32, tc.BF16}
    assert all(c in tc.DEPTH_CASES for c in tc.TIE_CASES + tc.TILE64_CASES)
    assert [tc.expected_kp(*c) for c in tc.TILE64_CASES] == [3, 6]


def test_wide_widths_hold_both_sides_of_every_scan_groups_edge():
    text, dev = source("topk.hip"), source("cf_device.hpp")
    body = function_body(text, "int scan_groups(int d) {")
    assert "int g = kGroupsPerBlock;" in body
    assert "while (g > 1 && (size_t)(1 + g) * (size_t)d * sizeof(float) > (size_t)144 * 1024) g >>= 1;" in body
    k_group = int(re.search(r"constexpr int kGroup = (\d+);", dev).group(1))
    k_block = int(re.search(r"constexpr int kBlock = (\d+);", dev).group(1))
    assert k_block // k_group == 16 == tc.scan_groups(1) and tc.SCAN_LDS_BYTES == 144 * 1024
    assert int(re.search(r"constexpr int kTopkMaxDim = (\d+);", text).group(1)) == tc.TOPK_MAX_DIM
    edges = [d for d in range(1, tc.TOPK_MAX_DIM) if tc.scan_groups(d) != tc.scan_groups(d + 1)]
    assert edges == [2168, 4096, 7372, 12288]
    for d in edges:
        assert d in tc.WIDE_WIDTHS and d + 1 in tc.WIDE_WIDTHS, d
    assert {tc.scan_groups(d) for d in tc.WIDE_WIDTHS} == {16, 8, 4, 2, 1}
    assert tc.TOPK_MAX_DIM in tc.WIDE_WIDTHS and max(tc.WIDE_WIDTHS) == tc.TOPK_MAX_DIM and tc.scan_groups(tc.TOPK_MAX_DIM) == 1
    assert (1 + tc.scan_groups(tc.TOPK_MAX_DIM)) * tc.TOPK_MAX_DIM * 4 <= tc.SCAN_LDS_BYTES  # the widest row still fits
    assert [tc.scan_groups(d) for d in tc.WIDE_BF16_ORDER_WIDTHS] == [16, 2, 1]
    # rows with a 16-chunk, an 8-tail and a scalar tail (d % 16 in 9..15), wide and narrow; and every width is too deep for path B
    # or is asked fewer queries than the sweep takes
    assert {d % 16 for d in tc.WIDE_WIDTHS if d % 16 >= 9} >= {9, 15} and {1031 % 16, 1033 % 16, 1039 % 16} == {7, 9, 15}
    assert all(tc.expected_kp(tc.BF16, d) is None for d in tc.WIDE_WIDTHS if d >= 1024)
