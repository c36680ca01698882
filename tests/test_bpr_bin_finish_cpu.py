"""The per-bin finish of the BPR chunk preparation and the one-read offsets kernel (csrc/bpr_prepare.hip: bpr_bin_finish_kernel,
bpr_bin_offsets_kernel) compile for gfx950 without spills and without scratch, and the finish kernel's LDS -- all of it static: the
launch asks for none beyond it -- leaves room for two workgroups on a CU's 160 KiB.  Checked on the gfx950 assembly hipcc emits for
bpr_prepare.hip (no device)."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import pytest

from gorse_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_PER_CU = 160 * 1024


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_finish_and_offsets_kernels_without_spills_scratch_or_excess_lds():
    src = os.path.join(ROOT, "gorse_amd", "csrc", "bpr_prepare.hip")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "isa_census.py"), src, "bpr_bin_"],
                         capture_output=True, text=True, check=True).stdout
    seen = {}
    for line in out.splitlines():
        m = re.match(r"^(?:void )?(\S+)\s+vgpr\s+(\d+)\s+agpr\s+(\d+)\s+sgpr\s+(\d+)\s+spills: vgpr (\d+) sgpr (\d+)\s+scratch (\d+) B\s+lds (\d+)", line)
        if m:
            seen[m.group(1)] = tuple(int(m.group(i)) for i in (2, 5, 6, 7, 8))
    for name in ("bpr_bin_finish_kernel", "bpr_bin_offsets_kernel"):
        assert name in seen, (name, sorted(seen))
        vgpr, vspill, sspill, scratch, lds = seen[name]
        assert vspill == 0 and sspill == 0 and scratch == 0, (name, vspill, sspill, scratch)
    vgpr, _, _, _, lds = seen["bpr_bin_finish_kernel"]
    # the launch passes no dynamic LDS: the static figure is the whole of it.  It must hold the capacities the library's own hook
    # reports (8 bytes per sample, 4 per staged row entry; a host function, no device needed) and fit a CU twice over; 512 threads
    # twice over need at most 128 registers each.
    cap, stage = C.c_int32(0), C.c_int32(0)
    capi.lib().gorse_hip_test_bpr_finish_capacities(C.byref(cap), C.byref(stage))
    assert 8 * cap.value + 4 * stage.value <= lds <= LDS_PER_CU // 2, (cap.value, stage.value, lds)
    assert vgpr <= 128, vgpr
