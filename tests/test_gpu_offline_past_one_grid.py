"""The offline pass's device modules (csrc/recommend.hip, csrc/nbr_build.hip, csrc/cand.hip and the scan they share,
csrc/csr_scan.hpp) past the first step of every loop that walks more work than one launch, one grid or one scan workgroup holds.
The neighbouring modules pin the per-row rules; every case of theirs fits the first step.  Here the second step runs, where state
survives from one item of work to the next: cand_merge_kernel's LDS arrays behind the loop-top barrier, cand_sort_kernel's LDS
sort after a sort in global memory (and its `continue`), nbr_rule_kernel's accumulators across rows, and everything
mf_recommend_core offsets by q0.

The caps are reached at their real values (tests/offline_cases.py holds them as literals, tests/test_offline_grid_caps_cpu.py holds
those against the sources), the launch chunk of gorse_mf_recommend through gorse_hip_test_set_recommend.  Expected values never
come from the code under test: the oracle's rank and score for recommend, the host route through public calls for the neighbour
tables, tests/cand_ref.py for the chain -- restated over padded arrays for the millions of short rows (the CPU test holds the
restatement against cand_ref.Chain).  Every comparison is of integers or bit patterns, over ALL rows of the big cases."""
import functools

import numpy as np
import pytest

import cand_ref as R
import nbr_build_ref as B
import nbr_ref as NR
import offline_cases as oc
import test_gpu_mf_recommend as MR
import test_gpu_nbr_from_search as NS
from gorse_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _hooks_at_default():
    yield
    capi.set_nbr(0, 0)
    capi.lib().gorse_hip_test_set_recommend(0, 0, 0)
    capi.lib().gorse_hip_test_set_topk_path(0)
    capi.lib().gorse_hip_test_set_scan_block(0)


# ---- 1. recommend: the second and third launch, and tiny catalogues ------------------------------------------------------------

K = oc.REC_HOOK_K
CHUNK = oc.REC_HOOK_CHUNK  # queries per launch under the hook at k = 10


def small_launches():
    capi.lib().gorse_hip_test_set_recommend(oc.REC_HOOK[0], oc.REC_HOOK[1], 0)


@pytest.mark.parametrize("d", [64, 100])  # the register form and the LDS form of rec_fast_kernel
def test_recommend_all_users_in_two_launches(d):
    """users = NULL: query t of the second launch is user 240 + t"""
    P, Q = MR.base_factors(d)
    rows = MR.base_rows()
    mf = MR.make_mf(P, Q, rows)
    assert CHUNK < MR.U < 2 * CHUNK
    small_launches()
    _, _, cnt, n_fast, _ = MR.check(mf, P, Q, rows, np.arange(MR.U, dtype=np.int32), K, users_arg=None)
    assert cnt[1] == 0 and cnt[2] == 7 and n_fast > 0


@functools.lru_cache(maxsize=None)
def user_list_case():
    """500 queries (240 + 240 + 20): repeats, -1 on both sides of positions 240 and 480, seen rows of every kind; the positions next
    to the launch edges and the last one carry a valid user and a non-empty seen row"""
    rng = np.random.default_rng(17)
    users = rng.integers(0, MR.U, 500).astype(np.int32)
    users[[3, 238, 242, 477, 482]] = -1
    users[[239, 240]] = 17   # one user on both sides of the edge
    users[[479, 480]] = 2    # the user with 7 candidates
    users[[241, 481]] = 1    # the user with none
    users[499] = 5
    seen = MR.base_seen(users, rng)
    for t in (239, 240, 479, 480, 499):
        if seen[t].size == 0:
            seen[t] = rng.integers(0, MR.I, 23).astype(np.int32)
        assert users[t] >= 0
    assert any(s.size == 0 for s in seen[CHUNK:]) and 2 * CHUNK < users.size
    return users, seen


def test_recommend_user_list_in_three_launches():
    P, Q = MR.base_factors(64)
    rows = MR.base_rows()
    users, seen = user_list_case()
    mf = MR.make_mf(P, Q, rows)
    small_launches()
    _, _, cnt, n_fast, _ = MR.check(mf, P, Q, rows, users, K, seen=seen)
    assert not cnt[[3, 238, 241, 242, 477, 481, 482]].any() and 0 < cnt[479] <= 7 and cnt[239] == K and n_fast > 0


@functools.lru_cache(maxsize=None)
def ties_case():
    """500 queries over tests/offline_cases.py's ties_world: literal queries in every launch"""
    P, Q, rows = oc.ties_world()
    rng = np.random.default_rng(29)
    users = rng.integers(0, P.shape[0], 500).astype(np.int32)
    users[[245, 250, 485, 490]] = (3, 25, 4, 21)  # equal item rows and an all-zero user row, in the second and the third launch
    users[[7, 260, 495]] = -1
    seen = [rng.integers(0, Q.shape[0], 0 if t % 4 == 0 else int(rng.integers(1, 40))).astype(np.int32) for t in range(500)]
    return P, Q, rows, users, seen


def test_recommend_ties_past_the_first_launch():
    P, Q, rows, users, _ = ties_case()
    ok = np.ones(Q.shape[0], np.uint8)
    tied = MR.expected(P, Q, rows, users, K, ok)[3]
    assert tied[:CHUNK].any() and tied[CHUNK:2 * CHUNK].any() and tied[2 * CHUNK:].any() and not tied.all()
    assert tied[[245, 250, 485, 490]].all()
    mf = MR.make_mf(P, Q, rows)
    small_launches()
    _, _, _, _, n_lit = MR.check(mf, P, Q, rows, users, K, ok=ok)
    assert n_lit == int(tied.sum())


@pytest.mark.parametrize("which", ["user list", "ties"])
def test_chain_mf_stage_in_three_launches(which):
    """the same queries through gorse_cand_add_mf with their seen rows as the chain's base rows: the launches' rows go to
    dev->items + q0 * k on the device, the literal queries' rows are copied over them one by one"""
    if which == "ties":
        P, Q, rows, users, seen = ties_case()
        ok = np.ones(Q.shape[0], np.uint8)
    else:
        P, Q = MR.base_factors(64)
        rows = MR.base_rows()
        users, seen = user_list_case()
        ok = None
    n, n_items = users.size, Q.shape[0]
    mf = MR.make_mf(P, Q, rows)
    base = [s.tolist() for s in seen]
    keep = (np.arange(n_items) % 7 != 0).astype(np.uint8)
    ref = R.Chain(n, base)
    lists = R.mf_lists(mf, users, K, ok, ref)  # the hook at its default: one launch
    exp_i, exp_s, exp_c, tied = MR.expected(P, Q, rows, users, K, ok, seen)
    assert lists == R.rows_to_lists(exp_i, exp_s, exp_c)
    ref.add(lists, K, keep)
    ch = capi.CandidateChain(n_items)
    ch.begin(n, 2 * K, *R.csr(base))
    small_launches()
    ch.add_mf(mf, users, K, ok, keep)
    assert mf.recommend_stats()[:2] == (n - int(tied.sum()), int(tied.sum()))
    assert (which == "ties") <= bool(tied[CHUNK:2 * CHUNK].any() and tied[2 * CHUNK:].any())
    R.assert_exclusion(ch, ref, which)
    shared = np.arange(0, n_items, 3, dtype=np.int32)[:200]
    ref.add_shared(shared.tolist(), (-shared).astype(np.float64).tolist(), K)
    ch.add_shared(shared, (-shared).astype(np.float64), K)
    R.assert_exclusion(ch, ref, which + ", a stage merged over the mf rows")
    assert ch.info() == (n, 2, sum(len(r) for r in ref.cand), sum(len(r) for r in ref.cur))
    ch.finish()
    R.assert_same(ch, ref, what=which)
    assert any(c[2] == 0 for c in ref.cand[-1]) and any(c[2] == 0 for c in ref.cand[CHUNK])


@pytest.mark.parametrize("d", [16, 100])
@pytest.mark.parametrize("n_items", [1, 2, 7, 17])
def test_recommend_tiny_catalogues(n_items, d):
    """fewer items than slices (the launcher clamps to min(8, I)), and at I = 17 slices of 3 items of which the last two begin past
    the end; k + 1 beyond the catalogue; the default item filter and one that admits items without feedback"""
    rng = np.random.default_rng(100 * n_items + d)
    P = rng.standard_normal((6, d)).astype(np.float32)
    Q = rng.standard_normal((n_items, d)).astype(np.float32)
    everything = np.arange(n_items, dtype=np.int32)
    fed = everything[:-1] if n_items > 1 else everything  # the last item of a catalogue of several has no feedback
    rows = [everything[:0], fed[::-1].copy(), everything[:1], rng.permutation(fed)[: n_items // 2], fed[-1:], fed[1:]]
    assert (MR.default_ok(rows, n_items).sum() < n_items) == (n_items > 1)
    users = np.array([0, 1, 2, -1, 3, 4, 5, 2], np.int32)
    mf = MR.make_mf(P, Q, rows)
    for ok in (None, np.ones(n_items, np.uint8)):
        for k in (1, 10, 256):
            for slices in (0, oc.REC_MAX_SLICES):
                capi.lib().gorse_hip_test_set_recommend(slices, 0, 0)
                _, _, cnt, _, _ = MR.check(mf, P, Q, rows, users, k, ok=ok)
                assert cnt[3] == 0 and cnt.max() <= min(k, n_items)
                if ok is not None:
                    assert cnt[0] == min(k, n_items) and cnt[1] == int(n_items > 1)  # the item nobody has touched


# ---- 2. neighbour tables: the scan past one workgroup, the row kernels past one grid -----------------------------------------------

SCAN_EDGE_ROWS = [2047, 2048, 2049, 4097]  # n_rows + 1 counts: one workgroup exactly, two, two, three


@pytest.mark.parametrize("path", [NS.SCAN, NS.MFMA])
@pytest.mark.parametrize("n_rows", SCAN_EDGE_ROWS)
def test_table_scan_past_one_workgroup_dense(n_rows, path):
    src = oc.edge_sources(n_rows, 333)
    ptr, _, _ = NS.dense_case(NS.gauss(12, 333, 16), NS.EUCLIDEAN, capi.DTYPE_F32, path, 5, sources=src.tolist(), which=NR.HOP1,
                              what="%d rows" % n_rows)
    assert ptr.size == n_rows + 1 and (np.diff(ptr)[src >= 0] == 5).all() and not np.diff(ptr)[src < 0].any()


@pytest.mark.parametrize("n_rows", SCAN_EDGE_ROWS)
def test_table_scan_past_one_workgroup_sparse(n_rows):
    src = oc.edge_sources(n_rows, 421)
    ptr, _, _ = NS.sparse_case(5, sources=src.tolist(), which=NR.HOP1)
    assert ptr.size == n_rows + 1 and np.diff(ptr)[src >= 0].max() == 5 and not np.diff(ptr)[src < 0].any()


def row_step(r):
    return "row %d: step %d of the wave-per-row kernels" % (r, r // oc.ROW_GRID_ROWS)


def test_table_past_one_grid():
    """4 * 2^20 + 101 rows from the sparse search's 421 stored rows: nbr_rule_kernel strides over valid queries whose table row
    differs from their query number (64 rows have no source), nbr_compact_kernel over rows, nbr_bound_kernel once a hop-2 table
    is set and a call asks for the bounds; the scan's top kernel takes nine passes.  A row's list depends on its source alone:
    the expected table is the host route's 421 lists expanded over the sources.

    The dense route cannot get here: the searches hand the rule one block at a time (m = the block's queries), and the largest
    block is 2^20 queries (kChunkQ of topk_plan.hpp, the MFMA path's chunk in topk_mfma.hip; the scan's blocks of topk.hip hold
    65,535 at most), a quarter of what one grid of nbr_rule_kernel holds."""
    n, n_items = 3, 500
    ptr, idx, val = NS.sparse_world()
    index = capi.Sparse(ptr, idx, val)
    dev, host = capi.NbrRecommender(n_items), capi.NbrRecommender(n_items)
    try:
        src = oc.big_sources(index.N)
        stored = B.table_from_lists(range(index.N), B.sparse_lists(index, ptr, idx, val, range(index.N), n), n, True)
        want = oc.expand_table(*stored, src)
        assert np.diff(stored[0]).max() == n and want[0][-1] > oc.BIG_ROWS
        dev.set_table_from_sparse(NR.HOP1, index, n, src, None, True, NR.RAW, 1.0)
        assert dev.table_info(NR.HOP1) == (oc.BIG_ROWS, int(want[0][-1]), True)
        gp, gi, gw = dev.get_table(NR.HOP1)
        r = oc.first_difference(gp, want[0])
        assert r is None, ("indptr", row_step(max(r - 1, 0)))
        for name, g, w in (("indices", gi, want[1]), ("weights", gw.view(np.uint32), want[2].view(np.uint32))):
            r = oc.first_difference(g, w, want[0])
            assert r is None, (name, row_step(r))
        # recommend from a sample of its rows against a handle whose host-built hop-1 table holds just those rows' lists
        rng = np.random.default_rng(11)
        hop2 = NR.Table([rng.integers(0, n_items, int(m)) for m in rng.choice([0, 2, 7, 30], index.N)])
        rows = oc.big_sample_rows()
        host.set_table(NR.HOP1, *oc.expand_table(*stored, src[rows]), NR.RAW, 1.0)
        for h in (dev, host):
            hop2.set_on(h, NR.HOP2)
        q_dev = np.concatenate([rows, [-1]]).astype(np.int32)
        q_host = np.concatenate([np.arange(rows.size), [-1]]).astype(np.int32)
        sp, si = NR.seen_csr([rng.integers(0, n_items, int(m)) for m in rng.choice([0, 0, 4], q_dev.size)])
        for slots in (0, 48):  # 48: the queries split between LDS tables and global ones, by the bounds formed on the device
            capi.set_nbr(slots, 0)
            got, exp = dev.recommend(q_dev, 10, sp, si), host.recommend(q_host, 10, sp, si)
            NR.assert_same(got, exp, ("sampled rows", slots))
            assert dev.recommend_stats()[:2] == host.recommend_stats()[:2], (slots, dev.recommend_stats(), host.recommend_stats())
            assert exp[2].max() == 10 and (exp[2] == 0).sum() >= 5
    finally:
        for x in (dev, host, index):
            x.close()


# ---- 3. the candidate chain: past both grids and the scan's top pass -----------------------------------------------------------------

def run_case(case, what):
    """begin, add_lists, add_shared(keep), finish(keep) on the device; every row of every stage against the restatement"""
    want = oc.expected_chain(case)
    ch = capi.CandidateChain(case.n_items)
    try:
        def stage(s):
            oc.assert_csr(ch.exclusion(), want.excl[s], ("exclusion row pointer", "exclusion rows"), (what, "after stage %d" % (s - 1)))
            assert ch.info() == want.info[s], (what, s)

        ch.begin(case.nq, case.capacity, *case.base_csr())
        stage(0)
        ch.add_lists(*case.lists_csr(), case.k_lists)
        stage(1)
        ch.add_shared(case.shared_items, case.shared_scores, case.k_shared, case.keep_shared)
        stage(2)
        ch.finish(case.keep_finish)
        ptr, items, scores, stages = ch.get()
        oc.assert_csr((ptr, items, scores.view(np.uint64), stages), want.finished, ("row pointer", "items", "score bits", "stage numbers"),
                      (what, "finished"))
        assert ch.info() == want.info_finished, what
    finally:
        ch.close()
    return want


@pytest.mark.parametrize("nq", [oc.SCAN_ONE_TOP_PASS - 1, oc.SCAN_ONE_TOP_PASS])
def test_chain_scan_top_pass_edges(nq):
    """nq + 1 counts in exactly 256 and in 257 workgroup sums: the last shape nbr_scan_top_kernel scans in one pass and the first
    whose second pass starts from a carry"""
    want = run_case(oc.tiny_rows_case(nq), "%d queries" % nq)
    assert want.info[2][2] > want.info_finished[2] > 0 and want.info[2][2] > want.info[1][2] > 0


def test_chain_past_both_grids():
    """tests/offline_cases.py's big_chain_case: 4 * 2^20 + 37 queries, capacity 4"""
    case = oc.big_chain_case()
    want = run_case(case, "%d queries" % case.nq)
    assert want.info[2][2] > want.info_finished[2] > 0 and want.info[2][2] > want.info[1][2] > 0
