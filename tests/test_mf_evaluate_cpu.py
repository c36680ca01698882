"""gorse_mf_evaluate without a device: no kernel of csrc/mf_eval.hip spills or uses scratch and every instantiation its dispatcher can
reach is in the object (the form of tests/test_recommend_no_scratch_cpu.py); and the six metrics restated in numpy over the
library's own 1 / log2 and IDCG tables equal the host mirror's metric functions bit for bit -- the yardstick of
tests/test_gpu_mf_evaluate.py, pinned against the arithmetic the kernel is written in."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_no_evaluate_kernel_spills_or_scratch():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "isa_census.py"), os.path.join(ROOT, "gorse_amd", "csrc", "mf_eval.hip")],
                         capture_output=True, text=True, check=True).stdout
    seen = {}
    for line in out.splitlines():
        m = re.match(r"^(?:void )?(\S.*?)\s+vgpr\s+(\d+)\s+agpr\s+(\d+)\s+sgpr\s+(\d+)\s+spills: vgpr (\d+) sgpr (\d+)\s+scratch (\d+) B", line)
        if m:
            seen[m.group(1)] = tuple(int(m.group(i)) for i in (5, 6, 7))
    # the register form for nFactors 16 .. 128, the LDS form, the sum chain
    for name in ["mf_eval_user_kernel<%d>" % nc for nc in range(9)] + ["mf_eval_chain_kernel"]:
        assert name in seen, (name, sorted(seen))
    for name, (vspill, sspill, scratch) in seen.items():
        assert vspill == 0 and sspill == 0 and scratch == 0, (name, vspill, sspill, scratch)


def numpy_metrics(target, rank, inv_log, idcg):
    """NDCG, Precision, Recall, HR, MAP, MRR as mf_eval_user_kernel computes them: float32 operations in evaluator.go's order, the
    logarithms and the IDCG from the tables"""
    f = np.float32
    tset = set(int(x) for x in target)
    card, cnt = len(tset), len(rank)
    dcg, map_sum, mrr, hr, hit = f(0), f(0), f(0), f(0), 0
    for i, item in enumerate(rank):
        if int(item) in tset:
            dcg = f(dcg + inv_log[i])
            hit += 1
            map_sum = f(map_sum + f(hit) / f(i + 1))
            if hit == 1:
                mrr, hr = f(1) / f(i + 1), f(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.array([dcg / idcg[min(card, cnt)], f(hit) / f(cnt), f(hit) / f(card), hr, map_sum / f(card), mrr], np.float32)


def test_numpy_restatement_over_the_library_tables_equals_the_host_metrics():
    import __graft_entry__ as g
    g.build()
    from gorse_amd import capi, cf
    cap = capi.MF_EVAL_MAX_TOPK
    assert cap >= 100
    inv_log, idcg = capi.mf_evaluate_tables()
    assert inv_log.size == cap and idcg.size == cap + 1 and inv_log[0] == 1.0 and idcg[0] == 0.0 and idcg[1] == 1.0
    with pytest.raises(capi.GorseHipError):
        capi.mf_evaluate_tables(cap + 1)
    rng = np.random.default_rng(4)
    cases = [(np.array([3], np.int32), np.zeros(0, np.int32))]  # an empty rank list: 0 / 0
    for trial in range(300):
        n_items = int(rng.choice([12, 40, 400]))
        rank = rng.permutation(n_items)[:int(rng.choice([1, 2, 3, 10, 11, cap - 1, cap]))].astype(np.int32)
        target = rng.integers(0, n_items, int(rng.choice([1, 2, 5, 30, cap + 20]))).astype(np.int32)  # with duplicates
        cases.append((target, rank))
    some_hit = some_dup = 0
    for target, rank in cases:
        got = numpy_metrics(target, rank, inv_log, idcg)
        exp = np.array([cf.metric(mid, target, rank) for mid in range(6)], np.float32)
        nan = np.isnan(exp)
        assert np.array_equal(np.isnan(got), nan), (target, rank, got, exp)
        assert np.array_equal(got.view(np.uint32)[~nan], exp.view(np.uint32)[~nan]), (target, rank, got, exp)
        some_hit += exp[3] == 1
        some_dup += len(set(target.tolist())) < target.size
    assert some_hit > 50 and some_dup > 50
    assert np.isnan(np.array([cf.metric(mid, cases[0][0], cases[0][1]) for mid in (0, 1)])).all()
