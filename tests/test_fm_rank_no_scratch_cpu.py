"""No kernel of gorse_fm_rank_users spills or uses scratch: every instantiation the dispatcher can launch is named here, on the
gfx950 assembly hipcc emits for fm_resident.hip (the forward kernel over both row sources and the branch's kernels over slices:
what score_rounds launches) and for fm_rank.hip (the sort), no device.  No kernel of either file goes unnamed.  Register and
scratch figures only."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = ((8, 1), (16, 1), (32, 1), (64, 1), (64, 2))
KERNELS = {
    "fm_resident.hip": ("gorse::fm::att_score_kernel<gorse::fm::SliceRows>", "gorse::fm::att_exp_kernel<gorse::fm::SliceRows>",
                        "gorse::fm::att_enc_kernel<gorse::fm::SliceRows>") + tuple(
        "gorse::fm::fm_forward_kernel<%d, %d, gorse::fm::%s, %d>" % (g, nf, src, out)
        for g, nf in SHAPES for src in ("ComposedRows", "PaddedRows") for out in (0, 1)),
    "fm_rank.hip": ("gorse::fm::fm_rank_sort_kernel",),
}


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_no_rank_kernel_spills_or_scratch():
    for src, kernels in KERNELS.items():
        out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "isa_census.py"),
                              os.path.join(ROOT, "gorse_amd", "csrc", src)], capture_output=True, text=True, check=True).stdout
        seen = {}
        for line in out.splitlines():
            m = re.match(r"^(?:void )?(\S.*?)\s+vgpr\s+(\d+)\s+agpr\s+(\d+)\s+sgpr\s+(\d+)\s+spills: vgpr (\d+) sgpr (\d+)\s+scratch (\d+) B", line)
            if m:
                seen[m.group(1)] = tuple(int(m.group(i)) for i in (5, 6, 7))
        for name in kernels:
            assert name in seen, (name, sorted(seen))
            assert seen[name] == (0, 0, 0), (name, seen[name])
        assert set(seen) == set(kernels), (src, sorted(set(seen) - set(kernels)))  # no kernel of the file goes unnamed
