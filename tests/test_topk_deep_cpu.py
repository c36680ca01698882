"""The deep sweep form of the exact top-k without a device (gorse_amd/csrc/topk_deep.hip, topk_deep_plan.hpp): the resource report of its
kernels on the gfx950 assembly (no scratch, no spills), the plan header in a stand-alone C++ program under AddressSanitizer and
UBSan, and the served ranges and padded depths restated in numpy against that program's printout."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KP_MAX, SLICE = 24, 64  # the deepest register-resident operand (kSupportedKP), bf16 values per K-slice


def census(unit, pattern):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "isa_census.py"), os.path.join(ROOT, "gorse_amd", "csrc", unit), pattern],
                         capture_output=True, text=True, check=True).stdout
    seen = {}
    for line in out.splitlines():
        m = re.match(r"^(?:void )?(\S.*?)\s+vgpr\s+(\d+)\s+agpr\s+(\d+)\s+sgpr\s+(\d+)\s+spills: vgpr (\d+) sgpr (\d+)\s+scratch (\d+) B", line)
        if m:
            seen[m.group(1)] = tuple(int(m.group(i)) for i in (5, 6, 7))
    return seen


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_no_deep_kernel_spills_or_scratch():
    seen = census("topk_deep.hip", "deep")
    assert sorted(seen) == ["topk_deep_sweep_kernel<false>", "topk_deep_sweep_kernel<true>"], sorted(seen)
    for name, figures in seen.items():
        assert figures == (0, 0, 0), (name, figures)
    # the rescoring's forms for deep rows: no vector register spilled, no scratch (its scalar spills are those of the form it had)
    seen = census("topk_rescore.hip", "rescore")
    for g in (1, 2, 4, 8, 16):
        vspill, sspill, scratch = seen["topk_rescore_kernel<%d>" % g]
        assert vspill == 0 and scratch == 0 and sspill <= seen["topk_rescore_kernel<16>"][1] + 8, (g, vspill, sspill, scratch)


@pytest.fixture(scope="module")
def plan_lines(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("deep_plan") / "topk_deep_plan")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "cpp", "topk_deep_plan_main.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout.splitlines()


def test_plan_rules_under_sanitizers(plan_lines):
    assert plan_lines[-1] == "topk_deep_plan ok"


def test_served_ranges_and_padded_depths(plan_lines):
    """bf16 384 < d <= 4096, fp32 128 < d <= 1536; the operand (d or 3 d values) padded to whole 64-value slices; the rescoring's
    staging groups: the most of 16 .. 1 with (1 + 2 g) d + 2 x 1024 + 8 floats inside 144 KB"""
    rows = [ln.split() for ln in plan_lines[:-1]]
    assert {r[0] for r in rows} == {"bf16", "f32"}
    for name, d, serves, pad, slices, groups in rows:
        d, bf = int(d), name == "bf16"
        values = d if bf else 3 * d
        want = -(-values // 16) > KP_MAX and d <= (4096 if bf else 1536)
        assert int(serves) == want, (name, d)
        assert int(pad) == (-(-values // SLICE) * SLICE if want else 0) and int(slices) * SLICE == int(pad), (name, d)
        fits = [g for g in (16, 8, 4, 2, 1) if ((1 + 2 * g) * d + 2 * 1024 + 8) * 4 <= 144 * 1024]
        assert int(groups) == fits[0], (name, d)
    edges = {(r[0], int(r[1])) for r in rows}
    assert {("bf16", 384), ("bf16", 385), ("bf16", 4096), ("bf16", 4097), ("f32", 128), ("f32", 129), ("f32", 1536), ("f32", 1537)} <= edges
