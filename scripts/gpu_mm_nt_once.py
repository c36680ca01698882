#!/usr/bin/env python3
"""floats.MM 4096^3 NT on the matrix cores (sgemm_nt_mfma_kernel), five calls on resident operands: the command of the NT counter pass
(rocprofv3 --pmc ... -- python scripts/gpu_mm_nt_once.py; the counters of scripts/gpu_session.sh mmsq)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from gorse_amd import capi

n = 4096
g = torch.Generator(device="cuda").manual_seed(3)
a, b = torch.randn(n, n, device="cuda", generator=g), torch.randn(n, n, device="cuda", generator=g)
c = torch.zeros(n, n, device="cuda")
for _ in range(5):
    capi.sgemm_device(0, 1, n, n, n, a.data_ptr(), n, b.data_ptr(), n, c.data_ptr(), n)
    assert capi.lib().gorse_hip_test_sgemm_last_form() == capi.SGEMM_NT | capi.SGEMM_NT_MFMA
    print("kernel %.3f ms" % capi.lib().gorse_hip_test_sgemm_last_ms(), flush=True)
