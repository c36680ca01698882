"""gorse_cand (csrc/cand.hip): the recommenders of the offline pass chained on the device.

Expected candidates and exclusion rows never come from the chain: tests/cand_ref.py restates the stage rule in plain Python, and its
mf / neighbourhood lists come from the public host-to-host calls (MF.recommend under the base rows, NbrRecommender.recommend under
the concatenated rows).  Every comparison is exact: items, the scores' bits, stage numbers, row pointers, and the exclusion rows
after every stage against the sorted concatenation.  gorse_fm_rank_cand is held against gorse_fm_rank_users on the downloaded lists."""
import functools

import numpy as np
import pytest

import cand_ref as R
from gorse_amd import capi, synth

pytestmark = pytest.mark.gpu

INVALID, RANGE = capi.ERR_INVALID, capi.ERR_RANGE


@pytest.fixture(autouse=True)
def _hooks_at_default():
    yield
    capi.set_nbr(0, 0)
    capi.lib().gorse_hip_test_set_recommend(0, 0, 0)


def lists_stage(ch, ref, lists, k, keep=None, what=""):
    """one add_lists stage on both sides, then the exclusion rows compared"""
    ptr, items = R.csr([[e[0] for e in l] for l in lists])
    _, scores = R.csr([[e[1] for e in l] for l in lists], np.float64)
    ch.add_lists(ptr, items, scores, k, keep)
    ref.add(lists, k, keep)
    R.assert_exclusion(ch, ref, what)


def shared_stage(ch, ref, items, scores, k, keep=None, what=""):
    ch.add_shared(items, scores, k, keep)
    ref.add_shared(items, scores, k, keep)
    R.assert_exclusion(ch, ref, what)


def scored(items, rng):
    return [(int(i), float(s)) for i, s in zip(items, rng.normal(0, 1, len(items)))]


# ---- merge: old row lengths x new counts x where the new items fall ----------------------------------------------------------

OLD_LENS = [0, 1, 63, 64, 65, 255, 256, 257, 4096, 4097, 5000]  # 4096 = the longest row the begin's sort keeps in LDS
NEW_COUNTS = [0, 1, 63, 64, 65, 255, 256]


@pytest.mark.parametrize("where", ["below", "above", "interleaved"])
def test_merge_edges(where):
    rng = np.random.default_rng(3)
    n_items = 400000
    base, lists = [], []
    for n_old in OLD_LENS:
        for n_new in NEW_COUNTS:
            old = (100000 + 2 * rng.choice(50000, n_old, replace=False)).tolist()  # even items of [100000, 200000)
            if n_old >= 63:  # repeats inside the row, and an unsorted row
                old[5] = old[40]
                old[-1] = old[0]
            if where == "below":
                new = rng.choice(100000, n_new, replace=False)
            elif where == "above":
                new = 300000 + rng.choice(100000, n_new, replace=False)
            else:
                new = 100001 + 2 * rng.choice(50000, n_new, replace=False)  # odd items of the old row's range
            base.append(old)
            lists.append(scored(new, rng))
    nq = len(base)
    ch, ref = capi.CandidateChain(n_items), R.Chain(nq, base)
    ch.begin(nq, 512, *R.csr(base))
    R.assert_exclusion(ch, ref, "the base rows sorted")
    lists_stage(ch, ref, lists, 256, what=where)
    # a second stage over the merged rows: its items interleave with old and first-stage items alike
    second = [scored(rng.choice(n_items, 70, replace=False), rng) for _ in range(nq)]
    lists_stage(ch, ref, second, 256, what=where + " second stage")
    assert ch.info() == (nq, 2, sum(len(r) for r in ref.cand), sum(len(r) for r in ref.cur))
    ch.finish()
    R.assert_same(ch, ref, what=where)


def test_merge_next_to_the_largest_item():
    n_items = 2**31 - 1
    top = n_items - 1
    base = [[top, 5, top - 3], [], [top - 1], [0, top]]
    lists = [[(top - 1, 1.0), (top - 2, 2.0), (top, 3.0), (0, 4.0)], [(top, 0.5), (top, 0.25)], [(top, -1.0), (top - 2, -0.0)],
             [(top - 1, 7.0)]]
    ch, ref = capi.CandidateChain(n_items), R.Chain(4, base)
    ch.begin(4, 8, *R.csr(base))
    lists_stage(ch, ref, lists, 4)
    shared_stage(ch, ref, [top, top - 1, top - 2, 1], [1.0, 2.0, 3.0, 4.0], 4)
    ch.finish()
    R.assert_same(ch, ref)
    assert ref.cand[1][:2] == [(top, R.bits(0.5), 0), (top, R.bits(0.25), 0)]  # a list that repeats an item keeps both copies


# ---- filter -------------------------------------------------------------------------------------------------------------------

def test_filter_edges():
    rng = np.random.default_rng(4)
    n_items = 5000
    base, lists = [], []

    def case(excl, lst):
        base.append(list(excl))
        lists.append(scored(lst, rng))

    for n in [0, 1, 64, 65, 1000]:
        lst = rng.choice(n_items, n, replace=False)
        case([], lst)                                   # none excluded
        case(lst, lst)                                  # every entry excluded
        case(lst[::2], lst)                             # every other one
    full = rng.choice(n_items, 1000, replace=False)
    case(full[:54], full)                               # k = 10 reached inside the first chunk of 64, exactly at its end (54 + 10)
    case(full[:60], full)                               # ... reached inside the second chunk
    case([], [7, 8, 7, 9, 7] + list(range(100, 140)))   # a repeated item stays twice
    nq = len(base)
    keep = np.ones(n_items, np.uint8)
    keep[lists[-1][9][0]] = 0                           # the entry that would have been the 10th of the last list
    keep[full[63]] = 0                                  # ... and of the list whose 10th survivor ends the first chunk
    for k in [10, 64, 256]:
        for kp in (None, keep):
            what = "k=%d%s" % (k, ", keep" if kp is not None else "")
            ch, ref = capi.CandidateChain(n_items), R.Chain(nq, base)
            ch.begin(nq, 2 * k, *R.csr(base))
            lists_stage(ch, ref, lists, k, kp, what=what)
            lists_stage(ch, ref, lists, k, kp, what=what + ", what is left of the same lists")
            ch.finish()
            R.assert_same(ch, ref, what=what)
            if k == 10 and kp is not None:
                assert [c[0] for c in ref.cand[-1][:10]] == [7, 8, 7, 9, 7, 100, 101, 102, 103, 105]
    assert [c[0] for c in ref.cand[-1][:5]] == [7, 8, 7, 9, 7]


def test_a_dropped_entry_is_neither_candidate_nor_excluded():
    keep = np.ones(50, np.uint8)
    keep[[3, 4]] = 0
    ch, ref = capi.CandidateChain(50), R.Chain(2)
    ch.begin(2, 6)
    shared_stage(ch, ref, [3, 1, 4, 2, 9], [5.0, 4.0, 3.0, 2.0, 1.0], 3, keep)
    assert [c[0] for c in ref.cand[0]] == [1, 2, 9]
    shared_stage(ch, ref, [3, 1, 4], [1.0, 1.0, 1.0], 3)  # 3 and 4 were never excluded: this stage takes them
    assert [c[0] for c in ref.cand[0]] == [1, 2, 9, 3, 4]
    ch.finish()
    R.assert_same(ch, ref)


def test_the_longest_shared_list_with_the_survivors_at_its_end():
    n_items, n = 70000, 65536
    items = np.arange(n, dtype=np.int32)
    scores = np.arange(n, dtype=np.float64) * -0.5
    base = [list(range(n - 3)), list(range(0, n - 1, 1))[::-1], [], list(range(n))]
    ch, ref = capi.CandidateChain(n_items), R.Chain(4, base)
    ch.begin(4, 5, *R.csr(base))
    shared_stage(ch, ref, items, scores, 5)
    assert [len(r) for r in ref.cand] == [3, 1, 5, 0]
    ch.finish()
    R.assert_same(ch, ref)
    with pytest.raises(capi.GorseHipError) as e:
        ch2 = capi.CandidateChain(n_items)
        ch2.begin(1, 5)
        ch2.add_shared(np.arange(n + 1), np.zeros(n + 1), 5)
    assert e.value.code == INVALID


# ---- the scan over several workgroups -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("nq", [2047, 2048, 2049, 4097])
def test_many_queries_with_tiny_rows(nq):
    rng = np.random.default_rng(nq)
    n_items = 97
    base = [rng.integers(0, n_items, int(n)).tolist() for n in rng.integers(0, 4, nq)]
    lists = [scored(rng.integers(0, n_items, int(n)), rng) for n in rng.integers(0, 6, nq)]
    ch, ref = capi.CandidateChain(n_items), R.Chain(nq, base)
    ch.begin(nq, 5, *R.csr(base))
    lists_stage(ch, ref, lists, 3)
    shared_stage(ch, ref, [5, 96, 0, 33], [1.0, 2.0, 3.0, 4.0], 2)
    keep = (np.arange(n_items) % 5 != 0).astype(np.uint8)
    ch.finish(keep)
    R.assert_same(ch, ref, keep)


# ---- chains over the device stages ---------------------------------------------------------------------------------------------

NQ, NF = 300, 16


class World:
    """S-ml100k-sized synthetic feedback, a model at nFactors 16, an item-to-item and a user-to-user pair of tables, 300 queries"""

    def __init__(self, duplicate_items=False):
        d = synth.s_ml100k()
        rng = np.random.default_rng(11)
        self.U, self.I = d.U, d.I
        P, Q = synth.init_factors(d.U, d.I, NF, 0.0, 0.1, 1)
        if duplicate_items:  # equal factor rows: tied scores inside every top-k, so the queries take the literal route
            Q[1::2] = Q[0:-1:2][: Q[1::2].shape[0]]
        self.mf = capi.MF(d.U, d.I, NF, d.uptr, d.uidx, d.iptr, d.iidx)
        self.mf.set_factors(P, Q)
        self.users = rng.choice(d.U, NQ, replace=False).astype(np.int32)
        rows = [d.uidx[d.uptr[u]:d.uptr[u + 1]] for u in range(d.U)]
        # item-to-item: hop 1 = the queries' positives, hop 2 = 20 weighted neighbours per item
        nb = [rng.choice(d.I, 20, replace=False) for _ in range(d.I)]
        self.i2i = capi.NbrRecommender(d.I)
        self.i2i.set_table(capi.NBR_HOP1, *R.csr([rows[u][:30] for u in self.users]))
        p2, i2 = R.csr(nb)
        self.i2i.set_table(capi.NBR_HOP2, p2, i2, rng.uniform(0.01, 0.99, i2.size).astype(np.float32))
        # user-to-user: hop 1 = 10 weighted neighbour users per query, hop 2 = every user's positives
        un = [rng.choice(d.U, 10, replace=False) for _ in range(NQ)]
        self.u2u = capi.NbrRecommender(d.I)
        p1, i1 = R.csr(un)
        self.u2u.set_table(capi.NBR_HOP1, p1, i1, rng.uniform(0.01, 0.99, i1.size).astype(np.float32))
        self.u2u.set_table(capi.NBR_HOP2, d.uptr, d.uidx)
        # the base rows: part of the user's positives, unsorted and with a repeat, and a few other items
        self.base = []
        for t, u in enumerate(self.users):
            r = list(rng.permutation(rows[u])[: len(rows[u]) // 2]) + list(rng.integers(0, d.I, 3))
            self.base.append([int(x) for x in (r + r[:1] if t % 3 else r)])
        self.latest = rng.choice(d.I, 400, replace=False).astype(np.int32)
        self.latest_scores = np.sort(rng.uniform(1e9, 2e9, 400))[::-1].copy()
        self.keep = (rng.uniform(0, 1, d.I) > 0.1).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def world(duplicate_items=False):
    return World(duplicate_items)


def run_chain(w, order, k, base=True, users=None, rows=None, keep=None, finish_keep=None, what=""):
    """the stages named in `order` on the device chain and on the restatement; returns both"""
    users = w.users if users is None else users
    ch = capi.CandidateChain(w.I)
    ref = R.Chain(NQ, w.base if base else None)
    ch.begin(NQ, k * len(order), *(R.csr(w.base) if base else (None, None)))
    stats = {}
    for s, name in enumerate(order):
        if name == "mf":
            ref.add(R.mf_lists(w.mf, users, k, None, ref), k, keep)
            host = w.mf.recommend_stats()
            ch.add_mf(w.mf, users, k, keep=keep)
            stats["mf"] = (host, w.mf.recommend_stats())
        elif name in ("i2i", "u2u"):
            nbr = getattr(w, name)
            ref.add(R.nbr_lists(nbr, rows, k, ref), k, keep)
            host = nbr.recommend_stats()
            ch.add_nbr(nbr, rows, k, keep)
            stats[name] = (host, nbr.recommend_stats())
        elif name == "latest":
            ref.add_shared(w.latest, w.latest_scores, k, keep)
            ch.add_shared(w.latest, w.latest_scores, k, keep)
        elif name == "nothing":  # every query gets nothing: a list of items everybody excludes already
            item = [r[0] for r in ref.cur]
            assert len(set(item)) == 1
            ref.add_shared(item[:1], [1.0], k)
            ch.add_shared(item[:1], [1.0], k)
        R.assert_exclusion(ch, ref, "%s after stage %d (%s)" % (what, s, name))
        assert ch.info()[1:] == (s + 1, sum(len(r) for r in ref.cand), sum(len(r) for r in ref.cur))
    ch.finish(finish_keep)
    R.assert_same(ch, ref, finish_keep, what)
    for s in range(len(order)):
        stage_ms, chain_ms = ch.stats(s)
        assert chain_ms > 0.0 and (stage_ms > 0.0) == (order[s] in ("mf", "i2i", "u2u"))
    return ch, ref, stats


@pytest.mark.parametrize("k", [1, 10, 100, 256])
def test_chain_mf_first(k):
    w = world()
    ch, ref, stats = run_chain(w, ["mf", "i2i", "u2u", "latest"], k, what="k=%d" % k)
    assert {c[2] for r in ref.cand for c in r} == {0, 1, 2, 3}
    host, dev = stats["mf"]
    assert host[:2] == dev[:2]  # the same split between the threshold kernel and the literal route


def test_chain_mf_last_searches_under_the_base_rows():
    w = world()
    k = 100
    ch, ref, _ = run_chain(w, ["i2i", "u2u", "latest", "mf"], k, keep=w.keep)
    # the search ran under the base rows, so it returned items the earlier stages had taken: the filter dropped them
    mf_kept = [sum(1 for c in r if c[2] == 3) for r in ref.cand]
    assert min(mf_kept) < k and max(mf_kept) > 0


def test_two_nbr_stages_and_a_stage_that_gives_nothing():
    w = world()
    base0 = w.base
    try:
        w.base = [[7] + r for r in base0]  # item 7 is excluded for everybody: the stage "nothing" offers only that
        run_chain(w, ["u2u", "nothing", "i2i"], 10)
    finally:
        w.base = base0


def test_negative_users_and_rows_get_nothing_and_no_base_rows():
    w = world()
    users = w.users.copy()
    users[::7] = -1
    rows = np.arange(NQ, dtype=np.int32)
    rows[3::5] = -1
    ch, ref, _ = run_chain(w, ["mf", "i2i", "latest"], 10, base=False, users=users, rows=rows)
    assert all(not any(c[2] == 0 for c in ref.cand[t]) for t in range(0, NQ, 7))
    assert all(not any(c[2] == 1 for c in ref.cand[t]) for t in range(3, NQ, 5))


def test_mf_literal_route_rows():
    w = world(True)
    ch, ref, stats = run_chain(w, ["latest", "mf"], 10)
    host, dev = stats["mf"]
    assert dev[1] > 0 and host[:2] == dev[:2], (host, dev)


@pytest.mark.parametrize("lds_slots", [0, 1])
def test_nbr_lds_and_global_paths(lds_slots):
    w = world()
    capi.set_nbr(lds_slots, 64)  # 64 queries per launch: several launches
    ch, ref, stats = run_chain(w, ["latest", "i2i", "u2u"], 10)
    for name in ("i2i", "u2u"):
        host, dev = stats[name]
        assert host[:2] == dev[:2] and sum(dev[:2]) == NQ
        assert (dev[1] > 0) == (lds_slots == 1)


# ---- finish(keep) and gorse_fm_rank_cand ------------------------------------------------------------------------------------------

def fm_side(n, lo, hi, rng):
    rows = [(rng.choice(np.arange(lo, hi), 3, replace=False), rng.normal(0.5, 1.0, 3)) for _ in range(n)]
    ptr, idx = R.csr([r[0] for r in rows])
    _, val = R.csr([r[1] for r in rows], np.float32)
    return ptr, idx, val


@pytest.mark.parametrize("batch_size", [4, 1000])
def test_finish_keep_and_rank_cand(batch_size):
    rng = np.random.default_rng(8)
    n_items, nq, nf, d = 90, 9, 200, 8
    fm = capi.FM(nf, d)
    fm.set_params(np.float32(0.1), rng.normal(0, 0.3, nf).astype(np.float32), rng.normal(0, 0.3, (nf, d)).astype(np.float32))
    fm.set_items(*fm_side(n_items, 100, nf, rng))
    uptr, uidx, uval = fm_side(nq, 0, 120, rng)
    lists = [scored(rng.choice(n_items, int(n), replace=False), rng) for n in [0, 1, 2, 7, 8, 9, 30, 5, 12]]
    keep = np.ones(n_items, np.uint8)
    keep[[e[0] for e in lists[3]]] = 0  # a whole row goes
    keep[lists[4][0][0]] = 0            # a first entry
    keep[lists[5][-1][0]] = 0           # a last entry
    ch, ref = capi.CandidateChain(n_items), R.Chain(nq)
    ch.begin(nq, 40)
    lists_stage(ch, ref, lists, 30)
    shared_stage(ch, ref, np.arange(10), np.zeros(10), 10)
    with pytest.raises(capi.GorseHipError) as e:  # no finished pass yet
        fm.rank_cand(ch, uptr, uidx, uval, batch_size)
    assert e.value.code == INVALID
    ch.finish(keep)
    R.assert_same(ch, ref, keep)
    ptr, items, _, _ = ch.get()
    assert ptr[4] == ptr[3] or not set(items[ptr[3]:ptr[4]]) & {e[0] for e in lists[3]}
    want_s, want_o = fm.rank_users(uptr, uidx, uval, ptr, items, batch_size)
    want_stats = fm.rank_stats()
    got_s, got_o = fm.rank_cand(ch, uptr, uidx, uval, batch_size)
    got_stats = fm.rank_stats()
    assert np.array_equal(got_s.view(np.uint32), want_s.view(np.uint32))
    assert np.array_equal(got_o, want_o)
    for key in ("rows", "slices", "rounds", "host_sorted"):
        assert got_stats[key] == want_stats[key]
    other = capi.CandidateChain(n_items + 1)  # another item numbering than the catalogue's
    other.begin(nq, 4)
    other.finish()
    with pytest.raises(capi.GorseHipError) as e:
        fm.rank_cand(other, uptr, uidx, uval, batch_size)
    assert e.value.code == INVALID


# ---- errors leave the chain as it was ----------------------------------------------------------------------------------------------

def snapshot(ch):
    return ch.info(), [a.copy() for a in ch.exclusion()]


def refused(ch, code, call, *args, **kw):
    before = snapshot(ch)
    with pytest.raises(capi.GorseHipError) as e:
        call(*args, **kw)
    assert e.value.code == code, str(e.value)
    after = snapshot(ch)
    assert before[0] == after[0] and all(np.array_equal(a, b) for a, b in zip(before[1], after[1]))
    return str(e.value)


def test_errors_leave_the_chain_as_it_was():
    w = world()
    n = w.I
    ch = capi.CandidateChain(n)
    for call in (lambda: ch.add_shared([1], [1.0], 1), lambda: ch.finish(), lambda: ch.get(), lambda: ch.exclusion()):
        with pytest.raises(capi.GorseHipError) as e:  # no pass begun
            call()
        assert e.value.code == INVALID
    assert ch.info() == (0, 0, 0, 0)
    with pytest.raises(capi.GorseHipError) as e:
        ch.begin(2, 4, [0, 1, 2], [1, n])
    assert e.value.code == RANGE
    for bad_ptr in ([1, 1, 2], [0, 2, 1]):
        with pytest.raises(capi.GorseHipError) as e:
            ch.begin(2, 4, bad_ptr, [1, 2])
        assert e.value.code == INVALID
    with pytest.raises(capi.GorseHipError) as e:
        ch.begin(2, 0)
    assert e.value.code == INVALID

    ref = R.Chain(NQ, w.base)
    ch.begin(NQ, 30, *R.csr(w.base))
    shared_stage(ch, ref, w.latest, w.latest_scores, 10)
    one = np.zeros(NQ + 1, np.int64)
    for k in (0, -1, 257):
        refused(ch, INVALID, ch.add_shared, [1], [1.0], k)
        refused(ch, INVALID, ch.add_lists, one, [], [], k)
        refused(ch, INVALID, ch.add_mf, w.mf, w.users, k)
        refused(ch, INVALID, ch.add_nbr, w.i2i, None, k)
    # a refused begin leaves the pass that is under way, its exclusion rows and its candidates, alone
    refused(ch, RANGE, ch.begin, 2, 4, [0, 1, 2], [1, n])
    refused(ch, INVALID, ch.begin, 2, 4, [0, 2, 1], [1, 2])
    refused(ch, INVALID, ch.begin, 2, 0)
    refused(ch, INVALID, ch.add_shared, [1], [1.0], 21)          # 10 + 21 > 30
    refused(ch, INVALID, ch.add_nbr, w.i2i, None, 21)
    refused(ch, RANGE, ch.add_shared, [1, n], [1.0, 2.0], 5)
    refused(ch, RANGE, ch.add_shared, [-1], [1.0], 5)
    ptr = np.arange(NQ + 1, dtype=np.int64)
    refused(ch, RANGE, ch.add_lists, ptr, np.full(NQ, n), np.zeros(NQ), 5)
    refused(ch, INVALID, ch.add_lists, ptr + 1, np.zeros(NQ + 1), np.zeros(NQ + 1), 5)
    bent = ptr.copy()
    bent[5] = 0
    refused(ch, INVALID, ch.add_lists, bent, np.zeros(NQ), np.zeros(NQ), 5)
    too_far = w.users.copy()
    too_far[5] = w.U
    assert "out of range" in refused(ch, RANGE, ch.add_mf, w.mf, too_far, 5)
    rows = np.arange(NQ, dtype=np.int32)
    rows[9] = NQ
    assert "hop-1 rows" in refused(ch, RANGE, ch.add_nbr, w.i2i, rows, 5)
    other_nbr = capi.NbrRecommender(n + 1)
    other_nbr.set_table(capi.NBR_HOP1, np.zeros(NQ + 1, np.int64), [])
    other_nbr.set_table(capi.NBR_HOP2, np.zeros(2, np.int64), [])
    refused(ch, INVALID, ch.add_nbr, other_nbr, None, 5)
    unset = capi.NbrRecommender(n)
    refused(ch, INVALID, ch.add_nbr, unset, None, 5)
    small = synth.synth_cf(50, 40, 400, seed=1)
    other_mf = capi.MF(small.U, small.I, NF, small.uptr, small.uidx, small.iptr, small.iidx)
    refused(ch, INVALID, ch.add_mf, other_mf, None, 5)
    with pytest.raises(capi.GorseHipError) as e:
        ch.stats(1)
    assert e.value.code == INVALID
    # the capacity reached exactly is allowed; the pass goes on as if nothing had been refused
    ref.add(R.nbr_lists(w.i2i, None, 20, ref), 20)
    ch.add_nbr(w.i2i, None, 20)
    R.assert_exclusion(ch, ref)
    refused(ch, INVALID, ch.add_shared, [1], [1.0], 1)
    with pytest.raises(capi.GorseHipError) as e:
        ch.get()  # not finished
    assert e.value.code == INVALID
    ch.finish()
    R.assert_same(ch, ref)
    refused(ch, INVALID, ch.add_shared, [1], [1.0], 1)            # finished
    refused(ch, INVALID, ch.finish)


def test_at_most_255_stages():
    ch, ref = capi.CandidateChain(1000), R.Chain(1)
    ch.begin(1, 300)
    for s in range(capi.CAND_MAX_STAGES):
        ch.add_shared([s, s + 1], [1.0, 2.0], 1)
        ref.add_shared([s, s + 1], [1.0, 2.0], 1)
    refused(ch, INVALID, ch.add_shared, [999], [1.0], 1)
    ch.finish()
    R.assert_same(ch, ref)
    assert ch.get()[3][-1] == capi.CAND_MAX_STAGES - 1


# ---- lifetime -------------------------------------------------------------------------------------------------------------------------

def test_passes_on_one_handle():
    rng = np.random.default_rng(2)
    d = synth.synth_cf(60, 80, 900, seed=3)
    mf = capi.MF(d.U, d.I, NF, d.uptr, d.uidx, d.iptr, d.iidx)
    mf.set_factors(*synth.init_factors(d.U, d.I, NF, 0.0, 0.1, 2))
    ch = capi.CandidateChain(d.I)
    for nq in (40, 7, 60):
        base = [rng.integers(0, d.I, int(n)).tolist() for n in rng.integers(0, 9, nq)]
        ref = R.Chain(nq, base)
        ch.begin(nq, 12, *R.csr(base))
        assert ch.info() == (nq, 0, 0, sum(len(r) for r in base))
        if mf is not None:
            ref.add(R.mf_lists(mf, None, 5, None, ref), 5)
            ch.add_mf(mf, None, 5)
            R.assert_exclusion(ch, ref)
        shared_stage(ch, ref, rng.choice(d.I, 30, replace=False), rng.normal(0, 1, 30), 7)
        if nq == 40:
            continue  # a pass left unfinished: the next begin drops it
        ch.finish()
        R.assert_same(ch, ref)
        if nq == 7:  # an attached stage handle goes away between two passes
            mf.close()
            mf = None
