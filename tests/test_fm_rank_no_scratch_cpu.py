"""No kernel of gorse_fm_rank_users spills or uses scratch: every instantiation the dispatcher can launch is named here, on the
gfx950 assembly hipcc emits for fm_rank.hip (no device).  Register and scratch figures only."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KERNELS = ("gorse::fm::att_score_slices_kernel", "gorse::fm::att_exp_slices_kernel", "gorse::fm::att_enc_slices_kernel",
           "gorse::fm::fm_rank_sort_kernel") + tuple(
    "gorse::fm::fm_rank_forward_kernel<%d, %d, %s>" % (g, nf, vx)
    for g, nf in ((8, 1), (16, 1), (32, 1), (64, 1), (64, 2)) for vx in ("false", "true"))


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_no_rank_kernel_spills_or_scratch():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "isa_census.py"),
                          os.path.join(ROOT, "gorse_amd", "csrc", "fm_rank.hip")], capture_output=True, text=True, check=True).stdout
    seen = {}
    for line in out.splitlines():
        m = re.match(r"^(?:void )?(\S.*?)\s+vgpr\s+(\d+)\s+agpr\s+(\d+)\s+sgpr\s+(\d+)\s+spills: vgpr (\d+) sgpr (\d+)\s+scratch (\d+) B", line)
        if m:
            seen[m.group(1)] = tuple(int(m.group(i)) for i in (5, 6, 7))
    for name in KERNELS:
        assert name in seen, (name, sorted(seen))
        assert seen[name] == (0, 0, 0), (name, seen[name])
