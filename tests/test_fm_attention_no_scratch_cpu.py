"""No kernel of the factorization machine's item-embedding branch spills or uses scratch: every instantiation the dispatcher
can launch is named here, on the gfx950 assembly hipcc emits for fm.hip (no device).  The branch's kernels live in fm.hip, so
test_fm_no_scratch_cpu.py covers them as well; this test pins that they exist under these names."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = ((8, 1), (16, 1), (32, 1), (64, 1), (64, 2))
KERNELS = ("gorse::fm::att_score_kernel<gorse::fm::BatchRows>", "gorse::fm::att_exp_kernel<gorse::fm::BatchRows>",
           "gorse::fm::att_enc_kernel<gorse::fm::BatchRows>", "gorse::fm::att_loss_kernel",
           "gorse::fm::att_bwd_gx_kernel", "gorse::fm::att_bwd_ds_kernel", "gorse::fm::att_grad_kernel",
           "gorse::fm::fm_dense_opt_kernel<true>", "gorse::fm::fm_dense_opt_kernel<false>") + tuple(
    # with fields, scoring runs the logit + vx form (1) of the forward kernel and training its training form (2)
    "gorse::fm::fm_forward_kernel<%d, %d, gorse::fm::PaddedRows, %d>" % (g, nf, out) for g, nf in SHAPES for out in (1, 2))


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_no_attention_kernel_spills_or_scratch():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "isa_census.py"), os.path.join(ROOT, "gorse_amd", "csrc", "fm.hip")],
                         capture_output=True, text=True, check=True).stdout
    seen = {}
    for line in out.splitlines():
        m = re.match(r"^(?:void )?(\S.*?)\s+vgpr\s+(\d+)\s+agpr\s+(\d+)\s+sgpr\s+(\d+)\s+spills: vgpr (\d+) sgpr (\d+)\s+scratch (\d+) B", line)
        if m:
            seen[m.group(1)] = tuple(int(m.group(i)) for i in (5, 6, 7))
    for name in KERNELS:
        assert name in seen, (name, sorted(seen))
        assert seen[name] == (0, 0, 0), (name, seen[name])
