"""csrc/mf_rank.hip without a device: every instantiation of mf_score_kernel that with_factor_chunks (cf_device.hpp) can reach and
mf_rank_kernel are in the object, and no kernel of the file spills or uses scratch (the form of
tests/test_recommend_no_scratch_cpu.py and tests/test_mf_evaluate_cpu.py).  Checked on the gfx950 assembly hipcc emits."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_no_score_or_rank_kernel_spills_or_scratch():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "isa_census.py"), os.path.join(ROOT, "gorse_amd", "csrc", "mf_rank.hip")],
                         capture_output=True, text=True, check=True).stdout
    seen = {}
    for line in out.splitlines():
        m = re.match(r"^(?:void )?(\S.*?)\s+vgpr\s+(\d+)\s+agpr\s+(\d+)\s+sgpr\s+(\d+)\s+spills: vgpr (\d+) sgpr (\d+)\s+scratch (\d+) B", line)
        if m:
            seen[m.group(1)] = tuple(int(m.group(i)) for i in (5, 6, 7))
    # the register form for nFactors 16 .. 128, the LDS form, the literal heap
    for name in ["mf_score_kernel<%d>" % nc for nc in range(9)] + ["mf_rank_kernel", "expand_users_kernel"]:
        assert name in seen, (name, sorted(seen))
    for name, (vspill, sspill, scratch) in seen.items():
        assert vspill == 0 and sspill == 0 and scratch == 0, (name, vspill, sspill, scratch)
