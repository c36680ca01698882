"""The neighbourhood recommenders without a device: the register budget of nbr_recommend.hip's kernels on the gfx950 assembly, the
plan header (validation, bounds, launch planner) in a stand-alone C++ program under AddressSanitizer and UBSan, tests/nbr_ref.py
against the per-user host calls on the reference's known answers and on random worlds (exact CPU searchers built on the oracle), the
order sensitivity of the inputs the GPU test asserts, and the new symbols."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import nbr_host_suite as S
import nbr_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("nbr_walk_kernel<64, true>", "nbr_walk_kernel<256, true>", "nbr_walk_kernel<256, false>")


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_no_nbr_kernel_spills_or_scratch():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "isa_census.py"),
                          os.path.join(ROOT, "gorse_amd", "csrc", "nbr_recommend.hip")], capture_output=True, text=True, check=True).stdout
    seen = {}
    for line in out.splitlines():
        m = re.match(r"^(?:void )?(\S.*?)\s+vgpr\s+(\d+)\s+agpr\s+(\d+)\s+sgpr\s+(\d+)\s+spills: vgpr (\d+) sgpr (\d+)\s+scratch (\d+) B", line)
        if m:
            seen[m.group(1)] = tuple(int(m.group(i)) for i in (5, 6, 7))
    for name in KERNELS:  # one wave per query, a workgroup per query over an LDS table, the same over a global table
        assert name in seen, (name, sorted(seen))
        assert seen[name] == (0, 0, 0), (name, seen[name])
    assert set(seen) == set(KERNELS), sorted(set(seen) - set(KERNELS))  # no kernel of the file goes unnamed


@pytest.mark.skipif(shutil.which("g++") is None and shutil.which("clang++") is None, reason="no host C++ compiler")
def test_plan_header_under_sanitizers(tmp_path):
    """host-side validation returns its codes without a device; the bound; the launch planner"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    exe = str(tmp_path / "nbr_plan")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "cpp", "nbr_plan_main.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "nbr_plan ok" in out.stdout


def test_order_sensitive_inputs_are_order_sensitive():
    """the inputs of test_gpu_nbr_recommend's order case: adding the same lists in reverse changes the bits of at least a tenth of
    the sums in every query, so a kernel that adds the lists in another order cannot pass there"""
    hop1, hop2, n_items = R.order_sensitive_inputs()
    assert n_items == 257 and len(hop1.rows) == 32 and all(len(r) == 24 for r in hop1.rows)
    assert all(len(r) == 65 == len(set(r.tolist())) for r in hop2.rows) and hop2.transform == R.RECIP
    share = []
    for t in range(32):
        fwd, rev = R.sums(hop1, hop2, t), R.sums(hop1, hop2, t, reverse=True)
        assert set(fwd) == set(rev)
        a = np.array([fwd[j] for j in sorted(fwd)]).view(np.uint64)
        b = np.array([rev[j] for j in sorted(fwd)]).view(np.uint64)
        share.append(float((a != b).mean()))
        assert np.allclose(a.view(np.float64), b.view(np.float64), rtol=1e-12)
    assert min(share) >= 0.1, share


def test_ref_order_and_padding():
    hop2 = R.Table([[4, 1, 7, 2]], [[0.5, 0.5, np.inf, 0.25]])
    hop1 = R.Table([[0, 0], []], [[1.0, -1.0], []])  # inf - inf: item 7's sum is NaN and ranks last; 4, 1 and 2 tie at zero
    items, sums, cnt = R.recommend(hop1, hop2, [0, 1, -1], 5, [[2], [], []])
    assert items.tolist() == [[1, 4, 7, -1, -1], [-1] * 5, [-1] * 5] and cnt.tolist() == [3, 0, 0]
    assert np.isnan(sums[0, 2]) and sums[0, 3] == 0 and not sums[1:].any()
    assert R.weight(np.float32(0.5), R.RECIP, 1.0) == 2.0 and R.weight(3.0, R.RAW, 0.5) == 1.5 and R.weight(1.0, R.RECIP, 1.0) == np.inf


@pytest.fixture(scope="module")
def db(oracle):
    import __graft_entry__ as g
    g.build()
    return S.cpu_db(oracle)


@pytest.mark.parametrize("case", S.kats(), ids=lambda c: c["name"])
def test_reference_known_answers_per_user(db, case):
    scores = S.run_kat(db, case, False)
    S.check_kat(case, scores)
    if case["recommender"] == "item_to_item":
        coll = "item_to_item_" + case["name"]
        want = S.ref_item_to_item(db, coll, case["kind"], case["positives"], case["exclude"], case["categories"], case["cache_size"])
    else:
        coll = "user_to_user_" + case["name"]
        want = S.ref_user_to_user(db, coll, case["kind"], case["user"], case["exclude"], case["feedback"], case["cache_size"])
    S.same(scores, want)


@pytest.mark.parametrize("kind", ["embedding", "tags"])
def test_per_user_host_calls_are_the_restatement(db, kind):
    from gorse_amd import vectors as V
    coll, ids, positives, excludes, feedback = S.world(db, kind, 3, n=60, n_users=10)
    nonempty = 0
    for t in range(10):
        for n, categories in ((5, None), (50, ["b"])):
            got = V.ItemToItemRecommend(db, coll, kind, positives[t], excludes[t], categories, n)
            S.same(got, S.ref_item_to_item(db, coll, kind, positives[t], excludes[t], categories, n), ("item-to-item", t, n))
            nonempty += bool(got)
        got = V.UserToUserRecommend(db, coll, kind, ids[t], excludes[t], feedback, 7)
        S.same(got, S.ref_user_to_user(db, coll, kind, ids[t], excludes[t], feedback, 7), ("user-to-user", t))
        nonempty += bool(got)
    assert nonempty >= 15


def test_bulk_forms_need_a_device(db):
    """no CPU path: without a device the bulk calls end in the library's error"""
    from gorse_amd import capi, vectors as V
    if capi.device_count() > 0:
        pytest.skip("a GPU is present")
    coll, ids, positives, excludes, feedback = S.world(db, "embedding", 4, n=30, n_users=3)
    with pytest.raises(RuntimeError, match="no HIP device"):
        V.ItemToItemRecommendBulk(db, coll, "embedding", positives, excludes, None, 5)
    with pytest.raises(capi.GorseHipError) as e:
        capi.NbrRecommender(10)
    assert e.value.code == capi.ERR_NO_DEVICE
    with pytest.raises(capi.GorseHipError) as e:
        capi.NbrRecommender(0)
    assert e.value.code == capi.ERR_INVALID


def test_symbols_exported_and_declared(db):
    import ctypes as C
    from gorse_amd import capi, cf, vectors as V
    hdr = open(os.path.join(ROOT, "include", "gorse_hip.h")).read()
    L = C.CDLL(capi.LIB_PATH)
    for name in ("gorse_nbr_create", "gorse_nbr_destroy", "gorse_nbr_set_table", "gorse_nbr_recommend", "gorse_nbr_recommend_stats"):
        assert hasattr(L, name) and name in capi.SIGNATURES and re.search(r"\b%s\s*\(" % name, hdr), name
    assert hasattr(L, "gorse_hip_test_set_nbr") and "gorse_hip_test_set_nbr" in capi.SIGNATURES
    assert hasattr(cf.host(), "gh_logics_nbr_recommend")
    for name in ("ItemToItemRecommend", "UserToUserRecommend", "ItemToItemRecommendBulk", "UserToUserRecommendBulk"):
        assert callable(getattr(V, name)), name
    assert (capi.NBR_HOP1, capi.NBR_HOP2, capi.NBR_RAW, capi.NBR_RECIP, capi.NBR_MAX_K) == (0, 1, 0, 1, 256)
    assert capi.lib().gorse_hip_abi_version() == 1
