"""No kernel of the factorization machine spills or uses scratch ("Factorization machine"): the optimizer
pass once indexed its by-value argument block with a runtime tensor number, which put a 184-byte copy of the block in every lane's
scratch and cost more traffic than the step's own parameters.  Checked on the gfx950 assembly hipcc emits for fm.hip (no device)."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_no_fm_kernel_spills_or_scratch():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "isa_census.py"), os.path.join(ROOT, "gorse_amd", "csrc", "fm.hip")],
                         capture_output=True, text=True, check=True).stdout
    seen = {}
    for line in out.splitlines():
        m = re.match(r"^(?:void )?(\S.*?)\s+vgpr\s+(\d+)\s+agpr\s+(\d+)\s+sgpr\s+(\d+)\s+spills: vgpr (\d+) sgpr (\d+)\s+scratch (\d+) B", line)
        if m:
            seen[m.group(1)] = tuple(int(m.group(i)) for i in (5, 6, 7))
    for name in ("gorse::fm::fm_opt_kernel<true>", "gorse::fm::fm_opt_kernel<false>", "gorse::fm::fm_accum_kernel<16, 1>",
                 "gorse::fm::fm_accum_kernel<64, 2>", "gorse::fm::fm_forward_kernel<64, 2, gorse::fm::PaddedRows, 2>",
                 "gorse::fm::fm_forward_kernel<8, 1, gorse::fm::PaddedRows, 0>"):
        assert name in seen, (name, sorted(seen))
    for name, (vspill, sspill, scratch) in seen.items():
        assert vspill == 0 and sspill == 0 and scratch == 0, (name, vspill, sspill, scratch)
