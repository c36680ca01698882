"""No kernel of gorse_mf_recommend spills or uses scratch ("Recommending unseen items"): the threshold kernel keeps
a user's row in registers for nFactors 16 .. 128 and its survivor buffer in global memory, never in a per-lane array.  Checked on the
gfx950 assembly hipcc emits for recommend.hip (no device)."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_no_recommend_kernel_spills_or_scratch():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "isa_census.py"), os.path.join(ROOT, "gorse_amd", "csrc", "recommend.hip")],
                         capture_output=True, text=True, check=True).stdout
    seen = {}
    for line in out.splitlines():
        m = re.match(r"^(?:void )?(\S.*?)\s+vgpr\s+(\d+)\s+agpr\s+(\d+)\s+sgpr\s+(\d+)\s+spills: vgpr (\d+) sgpr (\d+)\s+scratch (\d+) B", line)
        if m:
            seen[m.group(1)] = tuple(int(m.group(i)) for i in (5, 6, 7))
    # the register form for every chunk count, the LDS form, the merge and the literal path's list builder
    for name in ["rec_fast_kernel<%d>" % nc for nc in range(9)] + ["rec_finish_kernel", "rec_candidates_kernel"]:
        assert name in seen, (name, sorted(seen))
    for name, (vspill, sspill, scratch) in seen.items():
        assert vspill == 0 and sspill == 0 and scratch == 0, (name, vspill, sspill, scratch)
