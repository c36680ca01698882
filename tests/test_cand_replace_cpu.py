"""Replacement without a device: the register budget of cand_replace.hip's kernels on the gfx950 assembly, the validation header in a
stand-alone C++ program under AddressSanitizer and UBSan, the plain-Python restatement (tests/replace_ref.py) on a pass worked out by
hand from worker/pipeline.go:573-643 and against the per-user host calls logics::AddReplacementCandidates / ApplyReplacementDecay
on string ids, the reference's known answer (TestReplacement), the new symbols, and -- by the restatement alone -- that every case
of tests/test_gpu_cand_replace.py reaches what it is named for."""
import json
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import cand_ref as R
import replace_cases as RC
import replace_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("repl_sort_kernel", "repl_mark_kernel", "repl_write_kernel", "repl_decay_sort_kernel", "nbr_scan_sums_kernel",
           "nbr_scan_top_kernel", "nbr_scan_apply_kernel")
P, RD = RR.POSITIVE, RR.READ


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_no_replacement_kernel_spills_or_scratch():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "isa_census.py"),
                          os.path.join(ROOT, "gorse_amd", "csrc", "cand_replace.hip")], capture_output=True, text=True, check=True).stdout
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
    exe = str(tmp_path / "cand_replace_plan")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "cpp", "cand_replace_plan_main.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "cand_replace_plan ok" in out.stdout


def test_restatement_on_a_pass_worked_out_by_hand():
    chain = R.Chain(2, [[6], []])
    chain.add([[(3, 1.5), (1, 1.0), (3, 0.5)], [(2, 9.0)]], 3)
    exists = np.ones(10, np.uint8)
    exists[5] = 0
    # user 0: 3 is positive and read -> positive; 7 read; 5 is gone; 6 is excluded (no recommender offered it) and still comes back;
    # the feedback of kind 0 matched neither expression.  user 1: no feedback that counts
    history = [[(7, RD), (3, RD), (5, P), (3, P), (6, P), (9, 0), (7, RD)], [(4, 0)]]
    rep = RR.Replaced(chain, history, None, exists)
    assert rep.rows == [[(3, P), (6, P), (7, RD)], []]
    assert rep.cand[0] == [(3, R.bits(1.5), 0), (1, R.bits(1.0), 0), (3, R.bits(0.5), 0), (6, 0, 255), (7, 0, 255)]
    assert rep.cand[1] == [(2, R.bits(9.0), 0)]
    assert rep.finished()[0].tolist() == [0, 5, 6] and rep.replacement()[2].tolist() == [P, P, RD] and rep.stats() == (2, 2, 1)
    assert chain.exclusion()[1].tolist() == [1, 3, 3, 6, 2]  # the exclude set is not touched
    # the ranker: both copies of 3 are decayed; 10 * 0.8 ties with the untouched 8 and keeps the ranker's place in front of it; the
    # NaN stays last
    scores = np.array([10.0, 8.0, 5.0, np.nan, 9.0, 1.0], np.float32)
    final, order = rep.decayed(scores, 0.8, 0.7)
    assert final[:3].tolist() == [8.0, 8.0, 4.0] and math.isnan(final[3]) and final[4:].tolist() == [6.3, 1.0]
    assert order.tolist() == [0, 1, 4, 2, 3, 0]
    final, order = rep.decayed(np.array([8.0, 8.0, 8.0, 6.0, 4.0, 1.0], np.float32), 1.0, 2.0)  # 4 * 2: a tie of four, in the ranker's order
    assert final[:5].tolist() == [8.0, 8.0, 8.0, 6.0, 8.0] and order[:5].tolist() == [0, 1, 2, 4, 3]
    assert 9 * 0.7 == 6.3 and 10 * 0.8 == 8.0


def world(seed):
    """a user per row: a recommender's list, feedback of three kinds, items that are gone, a ranker score per item with many ties"""
    rng = np.random.default_rng(seed)
    n_items, nq = 60, 40
    lists = [[(int(i), float(s)) for i, s in zip(rng.choice(n_items, int(n), replace=False), rng.normal(0, 1, int(n)))]
             for n in rng.integers(0, 12, nq)]
    lists[3] = lists[3] + lists[3][:1]  # a list that repeats an item
    history = [[(int(i), int(k)) for i, k in zip(rng.integers(0, n_items, int(n)), rng.choice([0, P, RD], int(n)))]
               for n in rng.integers(0, 15, nq)]
    exists = (rng.uniform(0, 1, n_items) > 0.2).astype(np.uint8)
    W = rng.choice(np.array([10.0, 8.0, 5.0, 4.0, 0.0, -1.0, 6.25, 2.5], np.float32), n_items)
    return n_items, lists, history, exists, W


@pytest.mark.parametrize("seed", [5, 6])
def test_restatement_is_the_per_user_host_mirror(seed):
    import __graft_entry__ as g
    g.build()
    from gorse_amd import vectors as V
    n_items, lists, history, exists, W = world(seed)
    name = lambda i: "item_%02d" % i  # noqa: E731  (ascending ids = ascending indices)
    chain = R.Chain(len(lists))
    chain.add(lists, 12)
    rep = RR.Replaced(chain, history, None, exists)
    ptr, items, _, _ = rep.finished()
    final, order = rep.decayed(W[items], 0.8, 0.7)
    existing = [name(i) for i in range(n_items) if exists[i]]
    decayed_in_place = 0
    for t, lst in enumerate(lists):
        cands = [V.Score(name(i), s, []) for i, s in lst]
        fb = [(name(i), k) for i, k in history[t]]
        grown, positive, negative = V.AddReplacementCandidates(cands, fb, existing)
        assert [s.Id for s in grown] == [name(c[0]) for c in rep.cand[t]]
        assert [R.bits(s.Score) for s in grown] == [c[1] for c in rep.cand[t]]
        assert positive == {name(i) for i, k in rep.rows[t] if k == P} and negative == {name(i) for i, k in rep.rows[t] if k == RD}
        got = V.RecommendWithReplacement(cands, fb, existing, lambda item: W[int(item[5:])], 0.8, 0.7)
        p0 = int(ptr[t])
        want = [(name(rep.cand[t][r][0]), R.bits(final[p0 + r])) for r in order[p0:int(ptr[t + 1])]]
        assert [(s.Id, R.bits(s.Score)) for s in got] == want, t
        # the same through the two steps, the ranking in between done here
        ranked = [grown[r] for r in RR.ranker_order(W[items[p0:int(ptr[t + 1])]])]
        for s in ranked:
            s.Score = float(W[int(s.Id[5:])])
        again = V.ApplyReplacementDecay(ranked, positive, negative, 0.8, 0.7)
        assert [(s.Id, R.bits(s.Score)) for s in again] == want, t
        decayed_in_place += sum(1 for kd, c in zip(rep.kinds()[t], rep.cand[t]) if kd and c[2] != RR.STAGE)
    added, positive, read = rep.stats()
    assert added > 20 and positive > 20 and read > 20 and decayed_in_place > 5


def test_reference_known_answer():
    import __graft_entry__ as g
    g.build()
    from gorse_amd import vectors as V
    kat = json.load(open(os.path.join(ROOT, "tests", "golden", "replacement_kats.json")))
    pd, rd = kat["positive_decay"], kat["read_decay"]
    assert (pd, rd) == (0.8, 0.7) and 9 * 0.7 == 6.3 and 10 * 0.8 == 8.0  # exact doubles: the expected lists can be compared with ==
    kind = lambda ty: P if ty in kat["positive_types"] else RD if ty in kat["read_types"] else 0  # noqa: E731
    assert len(kat["parts"]) == 2
    for part in kat["parts"]:
        expected = [(i, s) for i, s in part["expected"]]
        cands = [V.Score(i, 0.0, []) for i in part["candidates"]]
        fb = [(i, kind(ty)) for i, ty in kat["feedback"]]
        got = V.RecommendWithReplacement(cands, fb, kat["items"], lambda item: float(int(item)), pd, rd)
        assert [(s.Id, s.Score) for s in got[: part["top"]]] == expected, part["name"]
        assert "8" not in [s.Id for s in got]  # feedback of type i counts for nothing
        # the restatement on indices: item id = index
        chain = R.Chain(1)
        chain.add([[(int(i), 0.0) for i in part["candidates"]]], 8)
        exists = np.zeros(11, np.uint8)
        exists[[int(i) for i in kat["items"]]] = 1
        rep = RR.Replaced(chain, [[(int(i), k) for i, k in fb]], None, exists)
        items = rep.finished()[1]
        final, order = rep.decayed(items.astype(np.float32), pd, rd)
        assert [(str(items[r]), final[r]) for r in order[: part["top"]]] == expected, part["name"]


def test_symbols_exported_and_declared():
    import ctypes as C

    import __graft_entry__ as g
    g.build()
    from gorse_amd import capi, cf, vectors as V
    hdr = open(os.path.join(ROOT, "include", "gorse_hip.h")).read()
    L = C.CDLL(capi.LIB_PATH)
    for name in ("gorse_cand_add_replacement", "gorse_cand_get_replacement", "gorse_cand_replacement_stats", "gorse_fm_rank_cand_decayed"):
        assert hasattr(L, name) and name in capi.SIGNATURES and re.search(r"\b%s\s*\(" % name, hdr), name
    assert (capi.CAND_STAGE_REPLACEMENT, capi.CAND_KIND_POSITIVE, capi.CAND_KIND_READ) == (255, 1, 2) == (RR.STAGE, P, RD)
    for define in ("GORSE_CAND_STAGE_REPLACEMENT 255", "GORSE_CAND_KIND_POSITIVE 1", "GORSE_CAND_KIND_READ 2", "GORSE_HIP_ABI_VERSION 1"):
        assert re.search(r"#define %s\b" % define, hdr), define
    for name in ("add_replacement", "replacement", "replacement_stats"):
        assert callable(getattr(capi.CandidateChain, name)), name
    assert callable(capi.FM.rank_cand_decayed)
    for name in ("gh_logics_replacement_add", "gh_logics_replacement_decay", "gh_logics_replacement_run"):
        assert hasattr(cf.host(), name), name
    assert callable(V.AddReplacementCandidates) and callable(V.ApplyReplacementDecay) and callable(V.RecommendWithReplacement)


# ---- every case of the GPU module reaches what it is named for ------------------------------------------------------------------

def edges(c, rep, decays):
    """per query: (appended items, history items decayed in place, ties between a decayed and an untouched entry)"""
    ptr, items = rep.finished()[:2]
    final, _ = rep.decayed(RC.ranker_scores(c, rep), *decays)
    out = []
    for t, kinds in enumerate(rep.kinds()):
        f = final[int(ptr[t]):int(ptr[t + 1])]
        appended = sum(1 for cd in rep.cand[t] if cd[2] == RR.STAGE)
        in_place = sum(1 for kd, cd in zip(kinds, rep.cand[t]) if kd and cd[2] != RR.STAGE)
        touched = {float(x) for x, kd in zip(f, kinds) if kd and not math.isnan(x)}
        ties = sum(1 for x, kd in zip(f, kinds) if not kd and float(x) in touched)
        out.append((appended, in_place, ties))
    return out


@pytest.mark.parametrize("name,decay", RC.CASE_DECAYS)
def test_ranked_cases_reach_their_edges(name, decay):
    c = RC.RANKED[name]()
    chain, rep = RC.restate(c)
    decays = RC.DECAYS[decay]
    e = edges(c, rep, decays)
    assert min(e[0]) >= 1, (name, decay, e[0])  # the anchor: an appended item, one decayed in place, a tie only the decay makes
    lens = np.diff(rep.finished()[0]).tolist()
    raw = [len(h) for h in c.history]
    if name == "history_rows":
        assert raw[1:1 + len(c.lengths)] == c.lengths == [0, 1, 63, 64, 65, 4095, 4096, 4097]
        assert all(len(set(h)) < len(h) and len({i for i, _ in h}) < len(set(h)) for h in c.history[3:9])  # repeats, and items of both kinds
        assert raw[c.one_item] == 100 and rep.rows[c.one_item] == [(33, P)]
        assert raw[c.dropped] > 64 and rep.rows[c.dropped] == [] and lens[c.dropped] == 3
        assert any(not c.keep[i] for h in c.history[3:9] for i, _ in h) and all(c.keep[i] for r in rep.rows for i, _ in r)
    if name == "candidates":
        assert lens[c.empty] == len(rep.rows[c.empty]) == e[c.empty][0] > 0 and not chain.cand[c.empty]
        assert e[c.whole][0] == 0 and e[c.whole][1] == len(rep.rows[c.whole]) > 0
        rows = [cd[0] for cd in rep.cand[c.repeat]]
        assert rows.count(rows[0]) == 2 and rep.kinds()[c.repeat][0] and rep.kinds()[c.repeat][2]
        assert e[c.excluded][1] == 0 and e[c.excluded][0] == len(rep.rows[c.excluded]) and e[c.excluded + 1][1] > 0
        assert set(c.base[c.excluded]) >= {i for i, _ in c.history[c.excluded]}
    if name.startswith("queries_"):
        assert c.nq == int(name[8:]) and (c.nq == 1 or sum(x[0] for x in e) > c.nq / 2 and sum(x[1] for x in e) > c.nq / 20)
    if name == "sort_lengths":
        assert lens[1:] == c.lengths == [1, 2, 63, 64, 65, 4096, 4097]
        assert all(x[0] and x[1] and x[2] for x in e[4:])
    if name == "sort_cap_hook":
        assert lens[1:] == [15, 16, 17, 40] and c.sort_cap == 16
    if name == "specials":
        ptr, items = rep.finished()[:2]
        s = RC.ranker_scores(c, rep)[int(ptr[c.special]):int(ptr[c.special + 1])]
        final, _ = rep.decayed(RC.ranker_scores(c, rep), *decays)
        f = final[int(ptr[c.special]):int(ptr[c.special + 1])]
        kinds = rep.kinds()[c.special]
        for test in (math.isnan, lambda x: x == math.inf, lambda x: x == -math.inf):
            assert {bool(kd) for x, kd in zip(s, kinds) if test(float(x))} == {True, False}  # once decayed, once not
        if decay == "tiny":
            zeros = [float(x) for x in f if x == 0.0]
            assert any(math.copysign(1, z) < 0 for z in zeros) and any(math.copysign(1, z) > 0 for z in zeros)  # -0 against +0
            assert any(0.0 < abs(float(x)) < sys.float_info.min for x in f)  # a subnormal product
        if decay == "above_one":
            assert decays[0] > 1 and decays[1] > 1
    if decay == "one":
        _, order = rep.decayed(RC.ranker_scores(c, rep), 1.0, 1.0)
        ptr = rep.finished()[0]
        s = RC.ranker_scores(c, rep)
        assert all(order[int(ptr[t]):int(ptr[t + 1])].tolist() == RR.ranker_order(s[int(ptr[t]):int(ptr[t + 1])]) for t in range(c.nq))


def test_rows_case_reaches_the_largest_item():
    c = RC.top_items()
    _, rep = RC.restate(c)
    top = 2**31 - 2
    assert c.n_items == top + 1 and rep.rows[0][-1] == (top, P) and rep.rows[1] == [(top, RD)]
    assert rep.cand[0][-1] == (top, 0, 255) and rep.cand[1] == [(top, R.bits(1.0), 0)] and rep.stats() == (6, 4, 4)
