"""No kernel of gorse_mf_recommend's literal mode 1 spills or uses scratch (csrc/recommend_literal.hip): the user's row in registers for
nFactors 16 .. 128, heap and tiles in LDS, never a per-lane array.  Checked on the gfx950 assembly hipcc emits (no device)."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_no_literal_kernel_spills_or_scratch():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "isa_census.py"),
                          os.path.join(ROOT, "gorse_amd", "csrc", "recommend_literal.hip"),
                          "-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"], capture_output=True, text=True, check=True).stdout
    seen = {}
    for line in out.splitlines():
        m = re.match(r"^(?:void )?(\S.*?)\s+vgpr\s+(\d+)\s+agpr\s+(\d+)\s+sgpr\s+(\d+)\s+spills: vgpr (\d+) sgpr (\d+)\s+scratch (\d+) B", line)
        if m:
            seen[m.group(1)] = tuple(int(m.group(i)) for i in (5, 6, 7))
    assert set(seen) == {"rec_literal_kernel<%d>" % nc for nc in range(9)}, sorted(seen)
    assert all(v == (0, 0, 0) for v in seen.values()), seen
