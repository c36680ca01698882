"""No BPR update kernel spills or uses scratch (csrc/bpr_update_users.hip, csrc/bpr_update.hip): the folder workgroups of an update
launch (csrc/bpr_fold.hpp run_folders, fold_pass) keep a slot's replica values in registers whatever its replica count, and the workers
address a hot item's replica row from the item's class word alone.  Checked on the gfx950 assembly hipcc emits for the two update
units (no device)."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_no_bpr_update_kernel_spills_or_scratch():
    out = "".join(subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "isa_census.py"), os.path.join(ROOT, "gorse_amd", "csrc", unit),
                                  "update"], capture_output=True, text=True, check=True).stdout
                  for unit in ("bpr_update_users.hip", "bpr_update.hip"))
    seen = {}
    for line in out.splitlines():
        m = re.match(r"^(?:void )?(\S.*?)\s+vgpr\s+(\d+)\s+agpr\s+(\d+)\s+sgpr\s+(\d+)\s+spills: vgpr (\d+) sgpr (\d+)\s+scratch (\d+) B", line)
        if m:
            seen[m.group(1)] = tuple(int(m.group(i)) for i in (5, 6, 7))
    # the forms the product launches: the user-run kernel at every width (atomics only / cold negatives by store), the per-sample kernel
    for name in ("bpr_update_user_kernel<4, true, false>", "bpr_update_user_kernel<4, false, false>",
                 "bpr_update_user_kernel<1, true, true>", "bpr_update_user_kernel<1, true, false>",
                 "bpr_update_user_kernel<2, true, false>", "bpr_update_user_kernel<8, true, false>",
                 "bpr_update_kernel<0, 0>", "bpr_update_kernel<1, 0>", "bpr_update_kernel<4, 0>", "bpr_update_kernel<8, 0>"):
        assert name in seen, (name, sorted(seen))
    for name, (vspill, sspill, scratch) in seen.items():
        assert vspill == 0 and sspill == 0 and scratch == 0, (name, vspill, sspill, scratch)
