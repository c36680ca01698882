"""Neither instantiation of sgemm_nt_mfma_kernel (csrc/sgemm_nt.hip) spills or uses scratch: 256 accumulator registers stay live
across the k loop, and nothing of a lane lives in memory.  Checked on the gfx950 assembly hipcc emits (no device)."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_nt_mfma_kernel_neither_spills_nor_uses_scratch():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "isa_census.py"),
                          os.path.join(ROOT, "gorse_amd", "csrc", "sgemm_nt.hip"),
                          "-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"], capture_output=True, text=True, check=True).stdout
    seen = {}
    for line in out.splitlines():
        m = re.match(r"^(?:void )?(\S.*?)\s+vgpr\s+(\d+)\s+agpr\s+(\d+)\s+sgpr\s+(\d+)\s+spills: vgpr (\d+) sgpr (\d+)\s+scratch (\d+) B", line)
        if m:
            seen[m.group(1)] = tuple(int(m.group(i)) for i in (5, 6, 7))
    assert set(seen) == {"sgemm_nt_mfma_kernel<true>", "sgemm_nt_mfma_kernel<false>"}, sorted(seen)
    assert all(v == (0, 0, 0) for v in seen.values()), seen
