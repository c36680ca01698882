"""gorse_fm_set_train_samples / gorse_fm_set_test_samples without a device: the register budget of every kernel of
fm_samples.hip on the gfx950 assembly (register and scratch figures only), the plan header in a stand-alone C++ program under
AddressSanitizer and UBSan against the numpy restatement of fm.hip's build_plan on the materialised rows, the host mirror's
Materialise against a Python restatement of Dataset.Get (model/ctr/data.go:221-267), and the new symbols."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import fm_rank_ref as K
import fm_ref as R
import fm_samples_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32

SHAPES = ((8, 1), (16, 1), (32, 1), (64, 1), (64, 2))
KERNELS = ("gorse::fm::att_score_kernel<gorse::fm::ItemRows>", "gorse::fm::att_exp_kernel<gorse::fm::ItemRows>",
           "gorse::fm::att_enc_kernel<gorse::fm::ItemRows>", "gorse::fm::att_bwd_gx_items_kernel",
           "gorse::fm::att_grad_items_kernel") + tuple(
    "gorse::fm::fm_forward_kernel<%d, %d, gorse::fm::ComposedRows, 2>" % s for s in SHAPES) + tuple(
    "gorse::fm::fm_accum_samples_kernel<%d, %d>" % s for s in SHAPES)


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_no_samples_kernel_spills_or_scratch():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "isa_census.py"),
                          os.path.join(ROOT, "gorse_amd", "csrc", "fm_samples.hip")], capture_output=True, text=True, check=True).stdout
    seen = {}
    for line in out.splitlines():
        m = re.match(r"^(?:void )?(\S.*?)\s+vgpr\s+(\d+)\s+agpr\s+(\d+)\s+sgpr\s+(\d+)\s+spills: vgpr (\d+) sgpr (\d+)\s+scratch (\d+) B", line)
        if m:
            seen[m.group(1)] = tuple(int(m.group(i)) for i in (5, 6, 7))
    for name in KERNELS:
        assert name in seen, (name, sorted(seen))
        assert seen[name] == (0, 0, 0), (name, seen[name])
    assert set(seen) == set(KERNELS), sorted(set(seen) - set(KERNELS))  # no kernel of the file goes unnamed


def _side_text(rows, lead):
    ptr, idx, val = K.csr(rows)
    ld = np.zeros(len(rows), np.int32) if lead is None else lead
    return " ".join(map(str, [len(rows), int(lead is not None)] + list(ptr) + list(idx) + list(val.view(np.uint32)) + list(ld)))


def _world_file(path, users, ulead, items, ilead, user, item, bs):
    """the world and, per batch, what build_plan's order gives on its materialised rows"""
    rows = [K.compose(users[u], 0 if ulead is None else int(ulead[u]), items[c], 0 if ilead is None else int(ilead[c]))
            for u, c in zip(user, item)]
    width = max([int(np.count_nonzero(v)) for _, v in rows] + [0])
    out = [_side_text(users, ulead), _side_text(items, ilead), "%d %d %d" % (len(user), bs, width),
           " ".join(map(str, user)), " ".join(map(str, item))]
    plan = S.plan_of_padded(*R.pad(rows, max(1, max(len(a) for a, _ in rows)) + 2), bs) if rows else []
    out.append(str(len(plan)))
    for feat, row, val in plan:
        out.append(" ".join(map(str, [len(feat)] + [x for t in zip(feat, row, val.view(np.uint32)) for x in t])))
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")
    return plan


def _random_world(seed):
    """sides with empty rows, zero values, leads up to the whole row and features on both sides; samples in any order"""
    rng = np.random.default_rng(seed)
    def side(n, lo, hi):  # noqa: E306
        rows, lead = [], []
        for _ in range(n):
            k = int(rng.integers(0, 6))
            idx = rng.choice(np.arange(lo, hi), k, replace=False).astype(np.int32)
            val = rng.normal(0, 1, k).astype(f32)
            val[rng.random(k) < 0.2] = 0
            rows.append((idx, val))
            lead.append(int(rng.integers(0, k + 1)))
        return rows, np.array(lead, np.int32)
    users, ulead = side(int(rng.integers(1, 20)), 0, 30)
    items, ilead = side(int(rng.integers(1, 20)), 20, 50)
    n = int(rng.integers(1, 200))
    return users, ulead, items, ilead, rng.integers(0, len(users), n).astype(np.int32), rng.integers(0, len(items), n).astype(np.int32)


@pytest.mark.skipif(shutil.which("g++") is None and shutil.which("clang++") is None, reason="no host C++ compiler")
def test_plan_header_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    exe = str(tmp_path / "fm_samples_plan")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "cpp", "fm_samples_plan_main.cpp"), "-o", exe], check=True)
    files = []

    def add(*a):
        files.append(str(tmp_path / ("world%d.txt" % len(files))))
        return _world_file(files[-1], *a)

    w = S.World()
    plan = add(w.users, w.ulead, w.items, w.ilead, w.user, w.item, S.BS)
    assert [len(p[0]) > 0 for p in plan] == [True] * 3 and int((plan[0][0] == S.SHARED).sum()) == 64
    add(w.users, w.ulead, w.items, w.ilead, w.user, w.item, 1)
    add(w.users, w.ulead, w.items, w.ilead, w.user, w.item, 256)           # one batch larger than the set
    add(w.users, None, w.items, None, w.user[:128], w.item[:128], 64)     # no leads; n a multiple of the batch size
    # an empty batch tail: the last batch's rows (user 0, item 3) hold no entry at all, and so does row 0
    user, item = np.concatenate([[0], w.user[1:64], np.zeros(5, np.int32)]), np.concatenate([[3], w.item[1:64], np.full(5, 3, np.int32)])
    plan = add(w.users, w.ulead, w.items, w.ilead, user.astype(np.int32), item.astype(np.int32), 64)
    assert len(plan) == 2 and len(plan[1][0]) == 0 and 0 not in plan[0][1]
    for seed in range(12):
        u, ul, it, il, us, its = _random_world(seed)
        add(u, ul, it, il, us, its, int(np.random.default_rng(seed).integers(1, 70)))
    out = subprocess.run([exe] + files, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "fm_samples_plan ok" in out.stdout


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()


@pytest.mark.parametrize("dims", [(), (5, 3)], ids=str)
def test_materialise_is_dataset_get(built, dims):
    """ctr.Materialise against Dataset.Get (data.go:221-267) restated in Python, sample by sample, in every bit"""
    from gorse_amd import ctr
    w = S.LabelWorld(dims)
    ds = ctr.SampleDataset(w.n_features, *w.sides(), embs=w.embs, samples=w.train)
    ptr, idx, val, tgt, embs = ds.Materialise().rows()
    user, item, target = w.train
    assert len(ptr) == len(user) + 1 and np.array_equal(tgt.view(np.uint32), target.view(np.uint32)) and len(embs) == len(dims)
    for i, (u, c) in enumerate(zip(user, item)):
        gi, gv, ge = w.get(int(u), int(c))
        a, b = int(ptr[i]), int(ptr[i + 1])
        assert np.array_equal(idx[a:b], gi) and np.array_equal(val[a:b].view(np.uint32), gv.view(np.uint32)), i
        assert gi[0] == u and gi[1] == w.n_users + c and b - a == 2 + len(w.user_labels[u]) + len(w.item_labels[c])
        for k in range(len(dims)):
            assert np.array_equal(embs[k][i], ge[k]), (i, k)
    assert not embs or not embs[0][item == 2].any()
    # a sample outside its side is refused
    bad = ctr.SampleDataset(w.n_features, *w.sides(), embs=w.embs, samples=([w.n_users], [0], [1.0]))
    with pytest.raises(ValueError):
        bad.Materialise()


def test_symbols_exported_and_declared(built):
    import ctypes as C
    from gorse_amd import capi, cf, ctr
    hdr = open(os.path.join(ROOT, "include", "gorse_hip.h")).read()
    L = C.CDLL(capi.LIB_PATH)
    for name in ("gorse_fm_set_train_samples", "gorse_fm_set_test_samples"):
        assert hasattr(L, name) and name in capi.SIGNATURES and re.search(r"\b%s\s*\(" % name, hdr), name
    assert "ContextLabels" in hdr  # the header says that per-sample context labels keep the padded route
    H = cf.host()
    for name in ("gh_ctr_samples_new", "gh_ctr_samples_set_side", "gh_ctr_samples_set_embeddings", "gh_ctr_samples_add",
                 "gh_ctr_samples_materialise", "gh_fm_fit_samples"):
        assert hasattr(H, name), name
    for cls, names in ((capi.FM, ("set_train_samples", "set_test_samples")), (ctr.FM, ("FitSamples",)),
                       (ctr.SampleDataset, ("Materialise", "add_samples"))):
        for name in names:
            assert callable(getattr(cls, name)), name
    assert capi.lib().gorse_hip_abi_version() == 1
