"""The tie path of a deep top-k handle without a device (csrc/topk_deep_hist.hip, topk_deep_hist_plan.hpp): the resource report of the
deep history kernels and of topk_tie_sort_kernel's forms on the gfx950 assembly, and the plan header in a stand-alone C++ program
under AddressSanitizer and UBSan."""
import os
import shutil
import subprocess

import pytest

from test_topk_deep_cpu import ROOT, census

SORT_BEFORE = (0, 16, 0)  # topk_tie_sort_kernel before its staging groups became a template argument: vector, scalar spills, scratch


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_no_deep_history_kernel_spills_or_scratch():
    seen = census("topk_deep_hist.hip", "deep")
    assert sorted(seen) == ["topk_deep_hist_kernel<false>", "topk_deep_hist_kernel<true>"], sorted(seen)
    assert all(vspill == 0 and scratch == 0 for vspill, _, scratch in seen.values()), seen
    seen = census("topk_tie.hip", "tie_sort")  # (a deep index is at most 4096 wide: never fewer than four groups)
    assert sorted(seen) == ["topk_tie_sort_kernel<%d>" % g for g in (16, 2, 4, 8)], sorted(seen)
    assert all(now <= before for figures in seen.values() for now, before in zip(figures, SORT_BEFORE)), seen


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_plan_rules_under_sanitizers(tmp_path):
    exe = str(tmp_path / "topk_deep_hist_plan")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "cpp", "topk_deep_hist_plan_main.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.splitlines()[-1] == "topk_deep_hist_plan ok", out.stdout + out.stderr
    rows = {tuple(ln.split()[:3]) for ln in out.stdout.splitlines()[:-1]}  # (dtype, d, staging groups) at the edges of the rule
    assert rows == {("bf16", "1", "16"), ("bf16", "1446", "8"), ("bf16", "2731", "4"), ("bf16", "4096", "4"),
                    ("f32", "1", "16"), ("f32", "1446", "8"), ("f32", "1536", "8")}, rows
