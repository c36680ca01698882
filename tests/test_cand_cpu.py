"""The candidate chain without a device: the register budget of cand.hip's kernels on the gfx950 assembly, the validation header in a
stand-alone C++ program under AddressSanitizer and UBSan, the plain-Python restatement (tests/cand_ref.py) on a pass worked out by
hand from logics/recommend.go:135-156 and against the per-user host call logics::RecommendSequential (exact CPU searchers built on
the oracle), the reference's known answers for the single list recommenders, and the new symbols."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import cand_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("cand_filter_kernel", "cand_append_kernel", "cand_merge_kernel", "cand_sort_kernel", "cand_compact_kernel",
           "nbr_scan_sums_kernel", "nbr_scan_top_kernel", "nbr_scan_apply_kernel")


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_no_cand_kernel_spills_or_scratch():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "isa_census.py"), os.path.join(ROOT, "gorse_amd", "csrc", "cand.hip")],
                         capture_output=True, text=True, check=True).stdout
    seen = {}
    for line in out.splitlines():
        m = re.match(r"^(?:void )?(\S.*?)\s+vgpr\s+(\d+)\s+agpr\s+(\d+)\s+sgpr\s+(\d+)\s+spills: vgpr (\d+) sgpr (\d+)\s+scratch (\d+) B", line)
        if m:
            seen[m.group(1)] = tuple(int(m.group(i)) for i in (5, 6, 7))
    for name in KERNELS:
        assert name in seen, (name, sorted(seen))
        assert seen[name] == (0, 0, 0), (name, seen[name])
    assert set(seen) == set(KERNELS), sorted(set(seen) - set(KERNELS))  # no kernel of the file goes unnamed


@pytest.mark.skipif(shutil.which("g++") is None and shutil.which("clang++") is None, reason="no host C++ compiler")
def test_plan_header_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    exe = str(tmp_path / "cand_plan")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "cpp", "cand_plan_main.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "cand_plan ok" in out.stdout


def test_restatement_on_a_pass_worked_out_by_hand():
    """RecommendSequential, limit = 0: each recommender filtered by the exclude set, its results added to the set afterwards"""
    ref = R.Chain(2, [[5, 1, 5], []])
    keep = np.ones(10, np.uint8)
    keep[2] = 0
    # stage 0: query 0 excludes 1 and 5; the repeated 3 stays twice (the set is updated after the list); k cuts query 1
    ref.add([[(1, 9.0), (3, 8.0), (3, 7.0), (5, 6.0), (4, 5.0)], [(0, 1.0), (1, 2.0), (2, 3.0), (3, 4.0)]], 3)
    assert [c[0] for c in ref.cand[0]] == [3, 3, 4] and [c[0] for c in ref.cand[1]] == [0, 1, 2]
    # stage 1, one list for both: what stage 0 took is excluded now; keep drops 2 for query 0 without excluding it
    ref.add_shared([4, 2, 6, 0, 7], [0.5, 0.4, 0.3, 0.2, 0.1], 2, keep)
    assert [c[0] for c in ref.cand[0]] == [3, 3, 4, 6, 0] and [c[0] for c in ref.cand[1]] == [0, 1, 2, 4, 6]
    ref.add_shared([2], [1.5], 1)
    assert [c for c in ref.cand[0][-1:]] == [(2, R.bits(1.5), 2)] and len(ref.cand[1]) == 5
    ptr, items = ref.exclusion()
    assert ptr.tolist() == [0, 9, 14] and items.tolist() == [0, 1, 2, 3, 3, 4, 5, 5, 6, 0, 1, 2, 4, 6]
    fptr, fitems, fscores, fstages = ref.finished(keep)
    assert fptr.tolist() == [0, 5, 9] and fitems.tolist() == [3, 3, 4, 6, 0, 0, 1, 4, 6] and fstages.tolist() == [0, 0, 0, 1, 1, 0, 0, 1, 1]
    assert fscores.view(np.float64).tolist() == [8.0, 7.0, 5.0, 0.3, 0.2, 1.0, 2.0, 0.5, 0.3]


@pytest.fixture(scope="module")
def db(oracle):
    import __graft_entry__ as g
    g.build()
    import nbr_host_suite as S
    return S.cpu_db(oracle)


@pytest.mark.parametrize("seed", [3, 4])
def test_restatement_is_the_per_user_host_call(db, seed):
    """tests/cand_ref.py, the GPU tests' yardstick, against logics::RecommendSequential (maps and sets, per user) on string ids: a
    cached list per user, item-to-item, user-to-user and a shared list, in two orders"""
    import cand_host_suite as H
    users, positives, excludes, stages = H.world(db, seed)
    for order in (stages, [stages[3], stages[1], stages[2], stages[0]]):
        got = H.per_user(db, users, positives, excludes, order)
        H.same_lists(got, H.restatement(db, users, positives, excludes, order))
        assert sum(map(len, got)) > 10 * len(users)
        assert {len(g) for g in got} != {sum(s.cache_size for s in order)}  # some stage came up short for somebody


def test_reference_known_answers_per_user(db):
    import cand_host_suite as H
    from gorse_amd import vectors as V
    for case in H.kats():
        for query in case["queries"]:
            H.check_kat(query, V.RecommendSequential(db, "user_1", [], case["exclude"], [H.kat_stage(case, query)]))


def test_symbols_exported_and_declared():
    import ctypes as C

    import __graft_entry__ as g
    g.build()
    from gorse_amd import capi
    hdr = open(os.path.join(ROOT, "include", "gorse_hip.h")).read()
    L = C.CDLL(capi.LIB_PATH)
    names = ["gorse_cand_" + n for n in ("create", "destroy", "begin", "add_mf", "add_nbr", "add_shared", "add_lists", "finish", "info", "get",
                                         "get_exclusion", "stats")] + ["gorse_fm_rank_cand"]
    for name in names:
        assert hasattr(L, name) and name in capi.SIGNATURES and re.search(r"\b%s\s*\(" % name, hdr), name
    assert (capi.CAND_MAX_K, capi.CAND_MAX_STAGES) == (256, 255)
    assert re.search(r"#define GORSE_CAND_MAX_K 256\b", hdr) and re.search(r"#define GORSE_CAND_MAX_STAGES 255\b", hdr)
    for name in ("begin", "add_mf", "add_nbr", "add_shared", "add_lists", "finish", "get", "exclusion", "info", "stats"):
        assert callable(getattr(capi.CandidateChain, name)), name
    assert callable(capi.FM.rank_cand)
    from gorse_amd import cf, vectors as V
    for name in ("gh_logics_seq_clear", "gh_logics_seq_add_lists", "gh_logics_seq_add_nbr", "gh_logics_seq_run"):
        assert hasattr(cf.host(), name), name
    assert callable(V.RecommendSequential) and callable(V.RecommendSequentialBulk)
    if capi.device_count() == 0:  # no CPU path
        with pytest.raises(capi.GorseHipError) as e:
            capi.CandidateChain(10)
        assert e.value.code == capi.ERR_NO_DEVICE
