"""The Deep ALS kernels (csrc/als_deep.hip) keep their accumulators in registers: no vector spill and no scratch in the gfx950 code
hipcc emits for them (scripts/isa_census.py, as tests/test_als_no_spills_cpu.py does for als.hip), and the packed block triangle's
index arithmetic (csrc/als_deep_plan.hpp) passes its stand-alone check under AddressSanitizer and UBSan.  No device needed."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["als_deep_kernel<%d, %s>" % (nb, c) for nb in (5, 6, 7, 8) for c in ("false", "true")] + \
          ["als_deep_long_kernel<%d>" % nb for nb in (5, 6, 7, 8)] + ["als_deep_reduce_kernel"]


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_no_deep_kernel_spills():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "isa_census.py"), os.path.join(ROOT, "gorse_amd", "csrc", "als_deep.hip")],
                         capture_output=True, text=True, check=True).stdout
    seen = {}
    for line in out.splitlines():
        m = re.match(r"^(?:void )?(\S.*?)\s+vgpr\s+(\d+)\s+agpr\s+(\d+)\s+sgpr\s+(\d+)\s+spills: vgpr (\d+) sgpr (\d+)\s+scratch (\d+) B", line)
        if m:
            seen[m.group(1)] = tuple(int(m.group(i)) for i in (2, 5, 6, 7))
    assert sorted(seen) == sorted(KERNELS)
    for name, (vgpr, vspill, sspill, scratch) in seen.items():
        assert vspill == 0 and scratch == 0, (name, vspill, scratch)
        # (the row kernel of nFactors 225..256 parks two scalars of its prologue in vector lanes, once per workgroup)
        assert sspill <= (2 if name == "als_deep_kernel<8, false>" else 0), (name, sspill)
        assert vgpr <= 512, (name, vgpr)  # one workgroup of four waves per CU: arch + accumulator registers of a lane


def test_packed_triangle_index_arithmetic_under_sanitizers(tmp_path):
    exe = str(tmp_path / "als_deep_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "gorse_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "als_deep_plan_check.cpp"), "-o", exe],
                   check=True)
    assert subprocess.run([exe], capture_output=True, text=True).returncode == 0
