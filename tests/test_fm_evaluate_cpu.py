"""gorse_fm_set_test / gorse_fm_evaluate without a device: the register budget of every kernel of fm_eval.hip, and of what
score_rounds launches for it from fm_resident.hip, on the gfx950 assembly, the partition and slice-planner header (the test
split's two sides and gorse_fm_rank_users' candidate lists) in a stand-alone C++ program under AddressSanitizer and UBSan, the
numpy restatement the GPU test compares with (fm_eval_ref) against the host library's metrics, and the new symbols."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import fm_eval_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32

KERNELS = {
    "fm_eval.hip": ("gorse::fm::fm_eval_keys_kernel", "gorse::fm::fm_eval_sort_count_kernel", "gorse::fm::fm_eval_sort_scan_kernel",
                    "gorse::fm::fm_eval_sort_scatter_kernel", "gorse::fm::fm_eval_count_kernel", "gorse::fm::fm_eval_chain_kernel"),
    # scoring: the forward kernel over the split's padded rows and the branch's kernels over slices (test_fm_rank_no_scratch_cpu.py
    # names every kernel of this file)
    "fm_resident.hip": ("gorse::fm::att_score_kernel<gorse::fm::SliceRows>", "gorse::fm::att_exp_kernel<gorse::fm::SliceRows>",
                        "gorse::fm::att_enc_kernel<gorse::fm::SliceRows>") + tuple(
        "gorse::fm::fm_forward_kernel<%d, %d, gorse::fm::PaddedRows, %d>" % (g, nf, out)
        for g, nf in ((8, 1), (16, 1), (32, 1), (64, 1), (64, 2)) for out in (0, 1)),
}


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_no_evaluate_kernel_spills_or_scratch():
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
        if src == "fm_eval.hip":
            assert set(seen) == set(kernels), sorted(set(seen) - set(kernels))  # no kernel of the file goes unnamed


@pytest.mark.skipif(shutil.which("g++") is None and shutil.which("clang++") is None, reason="no host C++ compiler")
def test_plan_header_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    exe = str(tmp_path / "fm_eval_plan")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "cpp", "fm_eval_plan_main.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "fm_eval_plan ok" in out.stdout


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()


@pytest.mark.parametrize("kind", sorted(E.CONTENTS))
def test_restatement_against_host_metrics(built, kind):
    """counts + chain -> Score equals ctr.Precision / Recall / Accuracy / AUC in every bit, at the GPU test's sizes"""
    for n_pos in E.SIZES:
        for n_neg in E.SIZES:
            pos, neg = E.sides(kind, n_pos, n_neg)
            c, s = E.counts(pos, neg)
            assert E.same_bits(E.score(c, s), E.host_score(pos, neg)), (kind, n_pos, n_neg, c, s)
            # strict <: ties and zeros of either sign are not below each other
            assert c[6] == sum(int((neg < p).sum()) for p in pos)


def test_restatement_where_the_chain_rounds(built):
    pos, neg = E.wide()
    c, s = E.counts(pos, neg)
    assert c[6] > 1 << 25
    assert float(s) != float(c[6])  # a sum of exact integers would be the exact total: the chain is not
    assert E.same_bits(E.score(c, s), E.host_score(pos, neg))
    # a pairwise (tree) sum of the same counts is yet another number, so the order is part of the result
    assert float(np.sum(E.below(pos, neg).astype(f32), dtype=f32)) != float(s)


def test_restatement_leaves_nans_out(built):
    pos, neg = E.with_nans()
    c, s = E.counts(pos, neg)
    assert c[5] == 5
    keep_p, keep_n = pos[~np.isnan(pos)], neg[~np.isnan(neg)]
    c2, s2 = E.counts(keep_p, keep_n)
    assert c[6] == c2[6] and E.same_bits(s, s2)
    from gorse_amd import ctr
    assert E.same_bits(f32(s2) / f32(len(keep_p) * len(keep_n)), f32(ctr.AUC(keep_p, keep_n)))


def test_counter_stops_at_2_to_24():
    x = f32(E.CAP)
    assert f32(x + f32(1)) == x and f32(f32(E.CAP - 1) + f32(1)) == x


def test_symbols_exported_and_declared(built):
    import ctypes as C
    from gorse_amd import capi, cf
    hdr = open(os.path.join(ROOT, "include", "gorse_hip.h")).read()
    thdr = open(os.path.join(ROOT, "include", "gorse_hip_test.h")).read()
    L = C.CDLL(capi.LIB_PATH)
    for name in ("gorse_fm_set_test", "gorse_fm_evaluate", "gorse_fm_evaluate_stats"):
        assert hasattr(L, name) and name in capi.SIGNATURES and re.search(r"\b%s\s*\(" % name, hdr), name
    for name in ("gorse_hip_test_set_fm_evaluate", "gorse_hip_test_fm_auc", "gorse_hip_test_fm_evaluate_times"):
        assert hasattr(L, name) and name in capi.SIGNATURES and re.search(r"\b%s\s*\(" % name, thdr), name
    assert "GORSE_FM_EVAL_COUNTS 7" in hdr and len(capi.EVAL_COUNTS) == 7
    H = cf.host()
    for name in ("gh_fm_set_test", "gh_fm_evaluate_resident", "gh_fm_set_host_evaluate"):
        assert hasattr(H, name), name
    from gorse_amd import ctr
    for cls, names in ((capi.FM, ("set_test", "evaluate", "evaluate_stats")), (ctr.FM, ("SetTest", "EvaluateResident", "SetHostEvaluate"))):
        for name in names:
            assert callable(getattr(cls, name)), name
    assert capi.lib().gorse_hip_abi_version() == 1
