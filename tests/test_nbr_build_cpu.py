"""Neighbour tables built on the device (csrc/nbr_build.hip) without a device: the register budget of the new kernels on the gfx950
assembly, the host-side argument validation of gorse_nbr_set_table_from_topk / _from_sparse in a stand-alone C++ program under
AddressSanitizer and UBSan, the Python restatement of the list rule (tests/nbr_build_ref.py, the GPU test's yardstick) against
similar_scores through the per-user host calls, and the new symbols."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import nbr_build_ref as B
import nbr_host_suite as S
import nbr_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("nbr_rule_kernel", "nbr_scan_sums_kernel", "nbr_scan_top_kernel", "nbr_scan_apply_kernel", "nbr_compact_kernel",
           "nbr_bound_kernel")


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_no_nbr_build_kernel_spills_or_scratch():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "isa_census.py"),
                          os.path.join(ROOT, "gorse_amd", "csrc", "nbr_build.hip")], capture_output=True, text=True, check=True).stdout
    seen = {}
    for line in out.splitlines():
        m = re.match(r"^(?:void )?(\S.*?)\s+vgpr\s+(\d+)\s+agpr\s+(\d+)\s+sgpr\s+(\d+)\s+spills: vgpr (\d+) sgpr (\d+)\s+scratch (\d+) B", line)
        if m:
            seen[re.sub(r"\(.*", "", m.group(1))] = tuple(int(m.group(i)) for i in (5, 6, 7))
    for name in KERNELS:  # the rule, the three kernels of the 64-bit scan, the compaction, the hop-1 bounds
        assert name in seen, (name, sorted(seen))
        assert seen[name] == (0, 0, 0), (name, seen[name])
    assert set(seen) == set(KERNELS), sorted(set(seen) - set(KERNELS))  # no kernel of the file goes unnamed


@pytest.mark.skipif(shutil.which("g++") is None and shutil.which("clang++") is None, reason="no host C++ compiler")
def test_argument_validation_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    exe = str(tmp_path / "nbr_build")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "cpp", "nbr_build_main.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "nbr_build ok" in out.stdout


def test_rule_by_hand():
    idx = np.array([4, 2, 9, 2, 7, 1, -1, -1], np.int32)
    raw = np.array([3.0, 2.0, 0.0, -0.0, np.nan, -1.0, 0.0, 0.0], np.float32)
    assert B.apply_rule(idx, raw, 6, 2, 5, False)[0] == [4, 9, 7, 1]  # both entries of the source skipped, whatever their score
    assert B.apply_rule(idx, raw, 6, 3, 5, False)[0] == [4, 2, 9, 2, 7]  # the cut at n
    ki, kw = B.apply_rule(idx, raw, 6, 3, 5, True)
    assert ki == [4, 2, 7] and np.isnan(kw[2])  # +0, -0 and negative dropped, a NaN is not <= 0
    assert B.apply_rule(idx, raw, 6, 4, 1, True)[0] == [2] and B.apply_rule(idx, raw, 0, 4, 1, True) == ([], [])
    ptr, ix, w = B.table_from_lists([3, -1, 3], {3: (idx, raw, 6)}, 2, True)
    assert ptr.tolist() == [0, 2, 2, 4] and ix.tolist() == [4, 2, 4, 2] and w.dtype == np.float32


@pytest.fixture(scope="module")
def db(oracle):
    import __graft_entry__ as g
    g.build()
    return S.cpu_db(oracle)


@pytest.mark.parametrize("kind,n", [("embedding", 4), ("tags", 4), ("auto", 4), ("tags", 30)])
def test_rule_is_similar_scores(db, kind, n):
    """a dense collection read as each kind: its lists hold the vector itself (first under Euclidean, wherever its own score puts it
    under Dot), inner products of exactly zero and negative ones, and -- n = 30 -- fewer than n survivors"""
    from gorse_amd import vectors as V
    rng = np.random.default_rng(5)
    X = np.zeros((24, 6), np.float32)
    for r in range(24):
        X[r, (r % 3) * 2:(r % 3) * 2 + 2] = rng.choice([-1.0, 1.0]) * (0.5 + rng.random(2))
    coll = "rule_%s_%d" % (kind, n)
    db.AddCollection(coll, 6, V.Euclidean if kind == "embedding" else V.Dot)
    ids = ["v%02d" % r for r in range(24)]
    db.AddVectors(coll, [V.Vector(ids[r], X[r]) for r in range(24)])
    transform, scale = (R.RECIP, 1.0) if kind == "embedding" else (R.RAW, 0.5 if kind == "auto" else 1.0)
    zero = negative = short = with_self = 0
    for s in range(24):
        res = db.QueryVectors(coll, db.GetVectors(coll, [ids[s]])[0], None, n + 1)
        idx = np.array([ids.index(v.Id) for v in res], np.int32)
        raw = np.array([v.Score for v in res], np.float32)
        ki, kw = B.apply_rule(idx, raw, len(res), s, n, kind != "embedding")
        got = V.QuerySimilarTyped(db, coll, kind, ids[s], None, n)
        assert [g.Id for g in got] == [ids[j] for j in ki], (kind, s)
        want = np.array([R.weight(w, transform, scale) for w in kw], np.float64)
        assert np.array_equal(np.array([g.Score for g in got], np.float64).view(np.uint64), want.view(np.uint64)), (kind, s)
        zero += int((raw == 0).any())
        negative += int((raw < 0).any())
        short += len(ki) < n
        with_self += s in idx.tolist()
    assert with_self > 0 and (kind == "embedding" or zero > 0) and (n < 30 or (short == 24 and negative > 0))


def test_symbols_exported_and_declared(db):
    import ctypes as C
    from gorse_amd import capi, cf, vectors as V
    hdr = open(os.path.join(ROOT, "include", "gorse_hip.h")).read()
    L = C.CDLL(capi.LIB_PATH)
    for name in ("gorse_nbr_set_table_from_topk", "gorse_nbr_set_table_from_sparse", "gorse_nbr_table_info", "gorse_nbr_get_table"):
        assert hasattr(L, name) and name in capi.SIGNATURES and re.search(r"\b%s\s*\(" % name, hdr), name
    for name in ("set_table_from_topk", "set_table_from_sparse", "get_table", "table_info"):
        assert callable(getattr(capi.NbrRecommender, name)), name
    assert hasattr(cf.host(), "gh_vdb_set_nbr_table_from_index") and callable(V.SetNbrTableFromIndex)
    assert re.search(r"#define\s+GORSE_NBR_MAX_LIST\s+1023\b", hdr) and capi.lib().gorse_hip_abi_version() == 1


def test_a_searcher_without_a_resident_index_is_refused(db):
    """the CPU searchers keep nothing on a device: the host method says so instead of falling back"""
    from gorse_amd import vectors as V
    coll, ids, positives, excludes, feedback = S.world(db, "embedding", 6, n=20, n_users=2)

    class Handle:
        h = None
    with pytest.raises(Exception, match="keeps no index on the device"):
        V.SetNbrTableFromIndex(db, coll, "embedding", Handle, R.HOP2, None, 5)
