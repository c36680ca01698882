"""Replacement on the device (csrc/cand_replace.hip): gorse_cand_add_replacement and gorse_fm_rank_cand_decayed.

Expected rows, decayed scores and orders never come from the device: tests/replace_ref.py restates worker/pipeline.go:573-643 in
plain Python on top of tests/cand_ref.py, and is given the ranker's float32 scores.  Every comparison is exact: the grown row
pointer, items, score bits and stage bytes, the replacement rows and kinds, the counts, the ranker's bits against
gorse_fm_rank_cand's on the same pass, the decayed doubles' bits and the order.  The cases are tests/replace_cases.py's;
tests/test_cand_replace_cpu.py shows without a device that each reaches what it is named for."""
import functools

import numpy as np
import pytest

import cand_ref as R
import replace_cases as RC
import replace_ref as RR
from gorse_amd import capi

pytestmark = pytest.mark.gpu

INVALID, RANGE = capi.ERR_INVALID, capi.ERR_RANGE


@pytest.fixture(autouse=True)
def _hooks_at_default():
    yield
    capi.lib().gorse_hip_test_set_fm_rank(0, 0)


def ranker(c):
    """the factorization machine whose score of item i is c.W[i]: feature i with weight W[i] per item, no factors, and one
    weightless feature for every user"""
    n, d = c.n_items, 8
    fm = capi.FM(n + 1, d)
    fm.set_params(np.float32(0.0), np.append(c.W, np.float32(0.0)).astype(np.float32), np.zeros((n + 1, d), np.float32))
    fm.set_items(np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.int32), np.ones(n, np.float32))
    users = (np.arange(c.nq + 1, dtype=np.int64), np.full(c.nq, n, np.int32), np.ones(c.nq, np.float32))
    return fm, users


def history_csr(history):
    ptr, items = R.csr([[e[0] for e in r] for r in history])
    _, kinds = R.csr([[e[1] for e in r] for r in history], np.uint8)
    return ptr, items, kinds


def finished_chain(c):
    """the case's list stage and finish on the device and on the restatement"""
    ch = capi.CandidateChain(c.n_items)
    ch.begin(c.nq, c.k, *R.csr(c.base))
    ptr, items = R.csr([[e[0] for e in l] for l in c.lists])
    _, scores = R.csr([[e[1] for e in l] for l in c.lists], np.float64)
    ch.add_lists(ptr, items, scores, c.k)
    ch.finish(c.finish_keep)
    chain, rep = RC.restate(c)
    R.assert_same(ch, chain, c.finish_keep, c.name)
    return ch, chain, rep


def replaced_chain(c):
    ch, chain, rep = finished_chain(c)
    excl = [a.copy() for a in ch.exclusion()]
    ch.add_replacement(*history_csr(c.history), c.keep)
    RR.assert_same(ch, rep, c.name)
    assert all(np.array_equal(a, b) for a, b in zip(excl, ch.exclusion())), "the exclusion rows are not touched"
    assert ch.replacement_stats()[3] > 0.0
    return ch, rep


def bits(a):
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def check_ranking(c, ch, rep, fm, users, decays, batch_size=1000):
    """rank_cand_decayed against rank_cand on the same pass and against the restatement fed with the device's float scores"""
    want_s, want_o = fm.rank_cand(ch, *users, batch_size)
    if c.sort_cap:
        capi.lib().gorse_hip_test_set_fm_rank(0, c.sort_cap)
    s, f, o = fm.rank_cand_decayed(ch, *users, batch_size, *decays)
    stats = fm.rank_stats()
    assert np.array_equal(bits(s), bits(want_s)), (c.name, "the ranker's bits")
    ef, eo = rep.decayed(s, *decays)
    assert np.array_equal(bits(f), bits(ef)), (c.name, decays, "decayed bits")
    assert np.array_equal(o, eo), (c.name, decays, "order")
    ptr = rep.finished()[0]
    cap = c.sort_cap or RC.SORT_LDS
    assert stats["host_sorted"] == int(np.sum(np.diff(ptr) > cap)) and stats["rows"] == int(ptr[-1]) and stats["device_ms"] > 0.0
    if decays == (1.0, 1.0):
        assert np.array_equal(f, want_s.astype(np.float64), equal_nan=True) and np.array_equal(o, want_o)
    return s, f, o


@functools.lru_cache(maxsize=None)
def case(name):
    return RC.RANKED[name]()


@pytest.mark.parametrize("name,decay", RC.CASE_DECAYS)
def test_case(name, decay):
    c = case(name)
    ch, rep = replaced_chain(c)
    fm, users = ranker(c)
    s, _, _ = check_ranking(c, ch, rep, fm, users, RC.DECAYS[decay])
    want = RC.ranker_scores(c, rep)  # the ranker is what the cases take it for
    assert np.array_equal(bits(s)[~np.isnan(want)], bits(want)[~np.isnan(want)]) and np.array_equal(np.isnan(s), np.isnan(want))


def test_items_next_to_the_largest():
    c = RC.top_items()
    replaced_chain(c)


def test_scores_and_order_alone():
    """outputs that are not wanted stay away; the host fallback then fetches what it needs by itself"""
    c = case("sort_cap_hook")
    ch, rep = replaced_chain(c)
    fm, users = ranker(c)
    s, f, o = check_ranking(c, ch, rep, fm, users, (0.8, 0.7))
    capi.lib().gorse_hip_test_set_fm_rank(0, c.sort_cap)
    assert np.array_equal(fm.rank_cand_decayed(ch, *users, 7, 0.8, 0.7, scores=False, final=False)[2], o)
    assert fm.rank_stats()["host_sorted"] == int(np.sum(np.diff(rep.finished()[0]) > c.sort_cap)) == 2
    s2, f2, o2 = fm.rank_cand_decayed(ch, *users, 7, 0.8, 0.7, order=False)
    assert o2 is None and np.array_equal(bits(s2), bits(s)) and np.array_equal(bits(f2), bits(f))
    assert fm.rank_stats()["host_sorted"] == 0


def test_a_pass_without_replacement():
    c = case("candidates")
    ch, chain, _ = finished_chain(c)
    fm, users = ranker(c)
    want_s, want_o = fm.rank_cand(ch, *users, 4)
    s, f, o = fm.rank_cand_decayed(ch, *users, 4, 0.8, 0.7)
    assert np.array_equal(bits(s), bits(want_s)) and np.array_equal(o, want_o)
    assert np.array_equal(bits(f), bits(want_s.astype(np.float64)))
    ptr, items, kinds = ch.replacement()
    assert not ptr.any() and items.size == 0 and kinds.size == 0 and ch.replacement_stats() == (0, 0, 0, 0.0)


# ---- lifetime and errors: the pass and its replacement rows stay what they were ------------------------------------------------

def snapshot(ch):
    return [a.copy() for a in ch.get()] + [a.copy() for a in ch.replacement()] + [ch.info(), ch.replacement_stats()]


def refused(ch, code, call, *args, **kw):
    before = snapshot(ch)
    with pytest.raises(capi.GorseHipError) as e:
        call(*args, **kw)
    assert e.value.code == code, str(e.value)
    after = snapshot(ch)
    assert all(np.array_equal(a, b) for a, b in zip(before[:7], after[:7])) and before[7:] == after[7:]


def test_lifetime_and_errors():
    c = case("candidates")
    hist = history_csr(c.history)
    fm, users = ranker(c)
    ch = capi.CandidateChain(c.n_items)
    for call in (lambda: ch.add_replacement(*hist), ch.replacement):  # no pass
        with pytest.raises(capi.GorseHipError) as e:
            call()
        assert e.value.code == INVALID
    ch.begin(c.nq, c.k, *R.csr(c.base))
    for call in (lambda: ch.add_replacement(*hist), ch.replacement):  # before finish
        with pytest.raises(capi.GorseHipError) as e:
            call()
        assert e.value.code == INVALID
    assert ch.info()[:3] == (c.nq, 0, 0) and ch.replacement_stats() == (0, 0, 0, 0.0)

    ch, chain, rep = finished_chain(c)
    ptr, items, kinds = hist
    bad_kind, far = kinds.copy(), items.copy()
    bad_kind[-1] = 3
    far[3] = c.n_items
    refused(ch, INVALID, ch.add_replacement, ptr, items, bad_kind)
    bad_kind[-1] = 0
    refused(ch, INVALID, ch.add_replacement, ptr, items, bad_kind)
    refused(ch, RANGE, ch.add_replacement, ptr, far, kinds)
    far[3] = -1
    refused(ch, RANGE, ch.add_replacement, ptr, far, kinds)
    bent = ptr.copy()
    bent[2] = 0
    refused(ch, INVALID, ch.add_replacement, bent, items, kinds)
    refused(ch, INVALID, ch.add_replacement, ptr + 1, np.append(items, 0), np.append(kinds, 1))
    R.assert_same(ch, chain, c.finish_keep)  # ... and the pass goes on as if nothing had been refused
    ch.add_replacement(ptr, items, kinds, c.keep)
    RR.assert_same(ch, rep)
    refused(ch, INVALID, ch.add_replacement, ptr, items, kinds)  # a second one
    for pd, rd in ((0.0, 0.7), (0.8, 0.0), (-1.0, 0.7), (0.8, -1.0), (float("nan"), 0.7), (0.8, float("nan"))):
        refused(ch, INVALID, fm.rank_cand_decayed, ch, *users, 100, pd, rd)
    other = capi.CandidateChain(c.n_items + 1)  # another item numbering than the catalogue's
    other.begin(c.nq, c.k)
    other.finish()
    other.add_replacement(ptr, items, kinds)
    refused(other, INVALID, fm.rank_cand_decayed, other, *users, 100, 0.8, 0.7)
    check_ranking(c, ch, rep, fm, users, (0.8, 0.7))
    # a new begin clears the replacement rows; the next pass takes its own
    ch.begin(c.nq, c.k, *R.csr(c.base))
    assert ch.replacement_stats() == (0, 0, 0, 0.0)
    with pytest.raises(capi.GorseHipError) as e:
        ch.add_replacement(ptr, items, kinds)
    assert e.value.code == INVALID
    ch.finish()
    assert not ch.replacement()[0].any()
    ch.add_replacement(ptr, items, kinds)
    empty = R.Chain(c.nq, c.base)
    RR.assert_same(ch, RR.Replaced(empty, c.history))


def test_no_queries():
    ch = capi.CandidateChain(10)
    ch.begin(0, 4)
    ch.finish()
    ch.add_replacement(np.zeros(1, np.int64), [], [])
    assert ch.replacement()[0].tolist() == [0] and ch.get()[0].tolist() == [0] and ch.replacement_stats()[:3] == (0, 0, 0)


# ---- a whole chain ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("batch_size", [64, 1000])
def test_whole_chain(batch_size):
    """mf -> item-to-item -> shared list -> finish(keep) -> replacement -> decayed ranking on S-ml100k-sized data, the restatement
    fed from the public host-to-host calls"""
    from test_gpu_cand import NQ, fm_side, world
    w = world()
    rng = np.random.default_rng(21)
    k = 30
    ch, ref = capi.CandidateChain(w.I), R.Chain(NQ, w.base)
    ch.begin(NQ, 3 * k, *R.csr(w.base))
    ref.add(R.mf_lists(w.mf, w.users, k, None, ref), k)
    ch.add_mf(w.mf, w.users, k)
    ref.add(R.nbr_lists(w.i2i, None, k, ref), k)
    ch.add_nbr(w.i2i, None, k)
    ref.add_shared(w.latest, w.latest_scores, k)
    ch.add_shared(w.latest, w.latest_scores, k)
    ch.finish(w.keep)
    R.assert_same(ch, ref, w.keep)
    # the history: the users' positives (half of them are base rows, so no recommender offered them), every tenth entry read, and a
    # few of the user's own candidates, so that some are decayed in place
    fptr, fitems, _, _ = ref.finished(w.keep)
    history = []
    for t in range(NQ):
        row = [int(i) for i in w.base[t]] + fitems[fptr[t]:fptr[t + 1]][::9].tolist()
        history.append([(i, RR.READ if (t + j) % 10 == 0 else RR.POSITIVE) for j, i in enumerate(row)])
    exists = (rng.uniform(0, 1, w.I) > 0.05).astype(np.uint8)
    rep = RR.Replaced(ref, history, w.keep, exists)
    ch.add_replacement(*history_csr(history), exists)
    RR.assert_same(ch, rep)
    added, positive, read = rep.stats()
    in_place = sum(1 for kinds, row in zip(rep.kinds(), rep.cand) for kd, cd in zip(kinds, row) if kd and cd[2] != RR.STAGE)
    assert added > NQ and positive > read > 0 and in_place > NQ
    nf, d = 200, 8
    fm = capi.FM(nf, d)
    fm.set_params(np.float32(0.1), rng.normal(0, 0.3, nf).astype(np.float32), rng.normal(0, 0.3, (nf, d)).astype(np.float32))
    fm.set_items(*fm_side(w.I, 100, nf, rng))
    users = fm_side(NQ, 0, 120, rng)
    want_s, _ = fm.rank_cand(ch, *users, batch_size)
    s, f, o = fm.rank_cand_decayed(ch, *users, batch_size, 0.8, 0.7)
    assert np.array_equal(bits(s), bits(want_s))
    ef, eo = rep.decayed(s, 0.8, 0.7)
    assert np.array_equal(bits(f), bits(ef)) and np.array_equal(o, eo)
    assert np.any(f != s.astype(np.float64))
