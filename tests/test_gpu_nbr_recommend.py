"""gorse_nbr_recommend: item-to-item and user-to-user recommendation lists for many users at once (csrc/nbr_recommend.hip).

Expected rows never come from the code under test: tests/nbr_ref.py restates the contract of include/gorse_hip.h in plain Python (a dict
of floats added in stored order, sorted by (isnan, -sum, item)).  Every case compares items, counts, the -1 / 0 padding and the bits of
every sum, and the split between the LDS and the global path with the bound the header states."""
import functools

import numpy as np
import pytest

import nbr_ref as R
from gorse_amd import capi

pytestmark = pytest.mark.gpu

WAVE_SLOTS, MID_SLOTS = 512, 4096  # csrc/nbr_plan.hpp: tables up to 512 slots are walked by one wave, up to 4096 are the middle class


@pytest.fixture(autouse=True)
def _hooks_at_default():
    yield
    capi.set_nbr(0, 0)


def handle(hop1, hop2, n_items):
    h = capi.NbrRecommender(n_items)
    hop1.set_on(h, R.HOP1)
    hop2.set_on(h, R.HOP2)
    return h


def bounds(hop1, hop2, n_items, rows, seen_rows):
    """the header's bound per query: min(n_items, entries the walk meets) + the seen row's length"""
    out = []
    for t, r in enumerate(rows):
        met = sum(len(hop2.rows[s]) for s in hop1.rows[r]) if r >= 0 else 0
        out.append((min(n_items, met) + (len(seen_rows[t]) if seen_rows is not None else 0)) if r >= 0 else 0)
    return np.array(out)


def check(h, hop1, hop2, rows, k, seen_rows=None, want=None, what=""):
    want = want if want is not None else R.recommend(hop1, hop2, rows, k, seen_rows)
    sp, si = R.seen_csr(seen_rows) if seen_rows is not None else (None, None)
    got = h.recommend(rows, k, sp, si)
    R.assert_same(got, want, what)
    return want


def rand_rows(rng, n_rows, hi, lens, distinct):
    return [rng.choice(hi, int(n), replace=False) if distinct else rng.integers(0, hi, int(n)) for n in rng.choice(lens, n_rows)]


def rand_weights(rng, rows, lo=0.01, hi=0.99):
    return [rng.uniform(lo, hi, len(r)).astype(np.float32) for r in rows]


def rand_seen(rng, hop1, hop2, rows, n_items):
    """per query: none, unsorted with repeats and overlaps among the reached items, items never reached"""
    out = []
    for t, r in enumerate(rows):
        reached = sorted(R.sums(hop1, hop2, r)) if r >= 0 else []
        if t % 4 == 0 or not reached:
            out.append([])
            continue
        part = list(rng.choice(reached, max(1, len(reached) // 3)))
        rest = np.setdiff1d(np.arange(n_items), reached)
        part += part[:3] + (list(rng.choice(rest, min(5, rest.size))) if t % 4 == 2 else [])
        rng.shuffle(part)
        out.append(part)
    return out


N_ITEMS, N_USERS = 307, 48


@functools.lru_cache(maxsize=None)
def world(shape):
    """(hop1, hop2, n_items) of the three table shapes; 48 users, 307 items"""
    rng = np.random.default_rng(5)
    if shape.startswith("i2i"):  # hop 1: the users' positives (they repeat); hop 2: each item's weighted neighbour list
        transform, scale = {"i2i": (R.RAW, 1.0), "i2i_half": (R.RAW, 0.5), "i2i_recip": (R.RECIP, 1.0)}[shape]
        rows1 = rand_rows(rng, N_USERS, N_ITEMS, [0, 1, 2, 7, 30], False)
        rows2 = rand_rows(rng, N_ITEMS, N_ITEMS, [0, 5, 10, 10, 33], True)
        return R.Table(rows1), R.Table(rows2, rand_weights(rng, rows2), transform, scale), N_ITEMS
    rows1 = rand_rows(rng, N_USERS, N_USERS, [0, 1, 5, 10], True)
    rows2 = rand_rows(rng, N_USERS, N_ITEMS, [0, 3, 40, 90], shape == "both")
    hop1 = R.Table(rows1, rand_weights(rng, rows1), R.RECIP, 1.0)
    if shape == "u2u":  # hop 2: the neighbours' feedback rows, unweighted, with repeats inside rows
        return hop1, R.Table(rows2), N_ITEMS
    return hop1, R.Table(rows2, rand_weights(rng, rows2, -3.0, 3.0), R.RAW, 0.37), N_ITEMS


@pytest.mark.parametrize("shape", ["i2i", "i2i_half", "i2i_recip", "u2u", "both"])
def test_table_shapes_on_both_paths(shape):
    hop1, hop2, n_items = world(shape)
    rng = np.random.default_rng(1)
    rows = list(range(N_USERS))
    seen = rand_seen(rng, hop1, hop2, rows, n_items)
    h = handle(hop1, hop2, n_items)
    want = check(h, hop1, hop2, rows, 10, seen, what="lds")
    bd = bounds(hop1, hop2, n_items, rows, seen)
    assert h.recommend_stats()[:2] == (N_USERS, 0) and bd.max() + 1 <= WAVE_SLOTS
    if shape == "u2u":
        assert any(len(set(r.tolist())) < len(r) for r in hop2.rows)
    # every query with anything to add over a global table, then split at the median bound
    capi.set_nbr(1, 0)
    check(h, hop1, hop2, rows, 10, seen, want, "global")
    nl, ng, ms = h.recommend_stats()
    assert (nl, ng) == (int((bd + 1 <= 2).sum()), int((bd + 1 > 2).sum())) and ng > N_USERS // 2 and ms > 0.0
    cut = int(np.median(bd)) + 1
    capi.set_nbr(cut, 0)
    check(h, hop1, hop2, rows, 10, seen, want, "split")
    nl, ng, _ = h.recommend_stats()
    assert (nl, ng) == (int((bd + 1 <= cut).sum()), int((bd + 1 > cut).sum())) and nl > 0 and ng > 0
    # a chunk of 3 with 10 queries: four launches per class
    capi.set_nbr(cut, 3)
    check(h, hop1, hop2, rows[:10], 10, seen[:10], tuple(a[:10] for a in want), "chunks")
    capi.set_nbr(0, 3)
    check(h, hop1, hop2, rows[:10], 10, seen[:10], tuple(a[:10] for a in want), "chunks, lds")


def test_order_of_the_lists_is_the_references():
    """sums whose bits depend on the order in which the lists are added (tests/test_nbr_cpu.py shows that they do)"""
    hop1, hop2, n_items = R.order_sensitive_inputs()
    rows = list(range(32))
    h = handle(hop1, hop2, n_items)
    want = check(h, hop1, hop2, rows, 256, what="wave")  # bound 257: one wave per query, no barrier between two lists
    assert h.recommend_stats()[:2] == (32, 0) and bounds(hop1, hop2, n_items, rows, None).max() + 1 <= WAVE_SLOTS
    # the same tables under a larger n_items: bound 24 x 65, a workgroup per query with a barrier between two lists
    wide = handle(hop1, hop2, 4000)
    assert bounds(hop1, hop2, 4000, rows, None).min() + 1 > WAVE_SLOTS
    check(wide, hop1, hop2, rows, 256, None, want, "workgroup")
    assert wide.recommend_stats()[:2] == (32, 0)
    capi.set_nbr(1, 0)
    check(h, hop1, hop2, rows, 256, None, want, "global")
    assert h.recommend_stats()[:2] == (0, 32)


def test_ties_go_by_ascending_item():
    rng = np.random.default_rng(3)
    n_items = 211
    rows2 = rand_rows(rng, 60, n_items, [20, 40], True)
    hop2 = R.Table(rows2, [rng.choice(np.array([0.25, 0.5, 1.0], np.float32), len(r)) for r in rows2])
    hop1 = R.Table(rand_rows(rng, 40, 60, [1, 2, 3], False))
    rows = list(range(40))
    h = handle(hop1, hop2, n_items)
    for k in (5, 16):
        want = check(h, hop1, hop2, rows, k)
        # equal sums straddle the cut: the k-th and the (k + 1)-th of the full ranking are equal in most queries
        full = R.recommend(hop1, hop2, rows, 256)
        straddle = sum(1 for t in rows if full[2][t] > k and full[1][t, k - 1] == full[1][t, k])
        assert straddle >= 20, straddle
        capi.set_nbr(1, 0)
        check(h, hop1, hop2, rows, k, None, want, "global")
        capi.set_nbr(0, 0)


@functools.lru_cache(maxsize=None)
def long_world():
    """hop-2 rows of every length around the wave and the workgroup width, hop-1 rows of length 0, 1, 2 and 500"""
    rng = np.random.default_rng(9)
    n_items = 1200
    lens = [0, 1, 63, 64, 65, 255, 256, 257, 1000]
    rows2 = [rng.choice(n_items, n, replace=False) for n in lens]
    hop2 = R.Table(rows2, rand_weights(rng, rows2, -2.0, 0.9), R.RECIP, 1.0)
    rows1 = [[], [0], [8], [0, 4], [8, 7]] + [[s] for s in range(1, 8)] + [rng.integers(0, 9, 500)]
    return R.Table(rows1), hop2, n_items


@pytest.mark.parametrize("k", [1, 10, 100, 256])
def test_list_lengths_and_k(k):
    hop1, hop2, n_items = long_world()
    rows = list(range(len(hop1.rows)))
    h = handle(hop1, hop2, n_items)
    want = check(h, hop1, hop2, rows, k)
    nl, ng, _ = h.recommend_stats()
    assert (nl, ng) == (len(rows), 0)
    assert want[2][0] == 0 and want[2][1] == 0  # an empty hop-1 row; a source whose hop-2 row is empty
    assert k == 1 or ((want[2] > 0) & (want[2] < k)).any()  # k beyond the number of candidates in some query
    bd = bounds(hop1, hop2, n_items, rows, None)
    assert (bd + 1 <= WAVE_SLOTS).any() and ((bd + 1 > WAVE_SLOTS) & (bd + 1 <= MID_SLOTS)).any()  # one wave and a workgroup
    capi.set_nbr(300, 0)
    check(h, hop1, hop2, rows, k, None, want, "split")
    assert h.recommend_stats()[1] == int((bd + 1 > 300).sum()) > 0


def test_exclusion():
    hop1, hop2, n_items = world("i2i")
    rows = [r for r in range(N_USERS) if len(R.sums(hop1, hop2, r)) >= 12][:12]
    reached = [sorted(R.sums(hop1, hop2, r)) for r in rows]
    rest = [np.setdiff1d(np.arange(n_items), x) for x in reached]
    seen = []
    for t, x in enumerate(reached):
        seen.append([x[5], x[0], x[5], x[2], x[0]] if t % 3 == 0            # unsorted, repeated
                    else list(rest[t][:40]) + [x[1]] if t % 3 == 1          # items that are never reached
                    else list(reversed(x)) + x[:4] + list(rest[t][-3:]))    # everything: count 0
    h = handle(hop1, hop2, n_items)
    want = check(h, hop1, hop2, rows, 10, seen)
    assert [int(c) for c in want[2][2::3]] == [0] * len(want[2][2::3])
    assert all(set(want[0][t][:want[2][t]]).isdisjoint(seen[t]) for t in range(len(rows)))
    capi.set_nbr(1, 0)
    check(h, hop1, hop2, rows, 10, seen, want, "global")
    capi.set_nbr(0, 0)
    # no seen rows at all; seen rows that are all empty
    want = check(h, hop1, hop2, rows, 10, None)
    check(h, hop1, hop2, rows, 10, [[] for _ in rows], want)


def test_table_edges():
    rng = np.random.default_rng(13)
    # items 0 and n_items - 1 of 2^20, a few hundred items in use; items congruent modulo the slot count of each LDS class
    n_items = 1 << 20
    pool = np.setdiff1d(rng.choice(n_items, 200, replace=False), [0, n_items - 1])
    chain_w = 7 + WAVE_SLOTS * np.arange(120)
    chain_m = 3 + MID_SLOTS * np.arange(250)
    rows2 = [rng.choice(pool, 60, replace=False) for _ in range(10)] + [chain_w[:60], chain_w[40:], chain_m[:200], chain_m[100:]]
    rows2[0][:2] = [0, n_items - 1]
    hop2 = R.Table(rows2, rand_weights(rng, rows2))
    rows1 = [[0, 1, 2], list(range(10)), [10, 11, 10], [12, 13, 12, 3], list(range(10)) * 15]
    hop1 = R.Table(rows1)
    rows = list(range(len(rows1)))
    seen = [[0], [n_items - 1, 5], list(chain_w[:10]), list(chain_m[50:150]), []]
    h = handle(hop1, hop2, n_items)
    want = check(h, hop1, hop2, rows, 256, seen)
    assert 0 in want[0][1] and n_items - 1 in want[0][0] and 0 not in want[0][0]
    bd = bounds(hop1, hop2, n_items, rows, seen)
    assert bd[2] + 1 <= WAVE_SLOTS < bd[3] + 1 <= MID_SLOTS < bd[4] + 1  # the two chains in their classes, the last query in the largest
    assert h.recommend_stats()[:2] == (5, 0)
    capi.set_nbr(1, 0)
    check(h, hop1, hop2, rows, 256, seen, want, "global")
    # a table filled to its bound: every entry a different item, the seen items never reached, one slot left free
    capi.set_nbr(0, 0)
    rows2 = [np.arange(0, 70), np.arange(70, 100), np.arange(100, 101)]
    hop2 = R.Table(rows2, rand_weights(rng, rows2))
    hop1 = R.Table([[2, 0, 1]])
    seen = [list(range(150, 170))]
    assert bounds(hop1, hop2, 307, [0], seen)[0] == 121
    h = handle(hop1, hop2, 307)
    want = check(h, hop1, hop2, [0], 256, seen)
    for slots, n_global in ((122, 0), (121, 1)):
        capi.set_nbr(slots, 0)
        check(h, hop1, hop2, [0], 256, seen, want, "slots %d" % slots)
        assert h.recommend_stats()[1] == n_global
    # items congruent modulo a shrunk slot count
    capi.set_nbr(64, 0)
    rows2 = [5 + 64 * np.arange(40), 5 + 64 * np.arange(20, 50)]
    hop2 = R.Table(rows2, rand_weights(rng, rows2))
    hop1 = R.Table([[0], [1, 0]])
    h = handle(hop1, hop2, 64 * 64)
    check(h, hop1, hop2, [0, 1], 64, [[5 + 64 * 3] * 2, []])
    assert h.recommend_stats()[:2] == (1, 1)


def test_rows_argument():
    hop1, hop2, n_items = world("both")
    h = handle(hop1, hop2, n_items)
    want = R.recommend(hop1, hop2, list(range(20)), 7)
    R.assert_same(h.recommend(20, 7), want, "rows = NULL")
    rows = [5, 3, 5, -1, 47, 0, -1, 3, 3, 46]
    seen = [[], [1, 2, 3], list(range(100)), [4], [], [], [], [9], [], []]
    want = check(h, hop1, hop2, rows, 7, seen)
    assert want[2][3] == 0 and want[2][6] == 0 and (want[0][3] == -1).all()
    capi.set_nbr(1, 4)
    check(h, hop1, hop2, rows, 7, seen, want, "global, chunks")


def test_lifetime():
    hop1, hop2, n_items = world("i2i")
    other1, other2, _ = world("i2i_recip")
    u1, u2, _ = world("u2u")
    rows = list(range(16))
    a, b = handle(hop1, hop2, n_items), handle(u1, u2, n_items)
    wa, wb = check(a, hop1, hop2, rows, 10), check(b, u1, u2, rows, 10)
    check(a, hop1, hop2, rows, 10, None, wa)  # two handles side by side: neither disturbs the other
    check(b, u1, u2, rows, 10, None, wb)
    other2.set_on(a, R.HOP2)  # replace hop 2, then hop 1
    w2 = check(a, hop1, other2, rows, 10)
    assert not np.array_equal(w2[1], wa[1])
    shifted = R.Table(hop1.rows[1:] + hop1.rows[:1])
    shifted.set_on(a, R.HOP1)
    w3 = check(a, shifted, other2, rows, 10)
    assert np.array_equal(w3[0][0], w2[0][1]) and not np.array_equal(w3[0], w2[0])
    check(b, u1, u2, rows, 10, None, wb)
    a.close()
    check(b, u1, u2, rows, 10, None, wb)


def test_errors_leave_the_outputs_untouched():
    hop1, hop2, n_items = world("i2i")
    h = capi.NbrRecommender(n_items)

    def refused(code, rows, k, sp=None, si=None):
        kk = min(max(k, 1), 300)
        n = rows if isinstance(rows, int) else len(rows)
        out = (np.full((n, kk), -7, np.int32), np.full((n, kk), 3.5, np.float64), np.full(n, -7, np.int32))
        with pytest.raises(capi.GorseHipError) as e:
            h.recommend(rows, k, sp, si, out=out)
        assert e.value.code == code, (e.value, code)
        assert (out[0] == -7).all() and (out[1] == 3.5).all() and (out[2] == -7).all()

    def refused_table(code, which, table):
        with pytest.raises(capi.GorseHipError) as e:
            table.set_on(h, which)
        assert e.value.code == code, (e.value, code)

    refused(capi.ERR_INVALID, 4, 10)  # no table set
    hop1.set_on(h, R.HOP1)
    refused(capi.ERR_INVALID, 4, 10)  # hop 2 still missing
    hop2.set_on(h, R.HOP2)
    for k in (0, -1, 257):
        refused(capi.ERR_INVALID, 4, k)
    refused(capi.ERR_RANGE, [0, N_USERS], 10)  # rows[t] beyond the hop-1 table
    refused(capi.ERR_RANGE, N_USERS + 1, 10)
    refused(capi.ERR_RANGE, [0, 1], 10, np.array([0, 1, 2]), np.array([3, n_items]))  # a seen item outside [0, n_items)
    refused(capi.ERR_RANGE, [0, 1], 10, np.array([0, 1, 2]), np.array([-1, 3]))
    refused(capi.ERR_INVALID, [0, 1], 10, np.array([0, 2, 1]), np.array([1, 2]))
    want = check(h, hop1, hop2, list(range(8)), 10)
    # tables that are refused leave the previous one in place
    w = [np.ones(len(r), np.float32) for r in hop2.rows]
    first = next(i for i, r in enumerate(hop2.rows) if len(r))
    refused_table(capi.ERR_RANGE, R.HOP2, R.Table([[0, n_items]]))
    refused_table(capi.ERR_RANGE, R.HOP2, R.Table([[-1]]))
    refused_table(capi.ERR_RANGE, R.HOP1, R.Table([[-1]]))
    refused_table(capi.ERR_INVALID, R.HOP2, R.Table([[1, 2, 1]], [[0.5, 0.25, 0.5]]))  # a weighted hop-2 row repeats an index
    for bad in (np.inf, -np.inf, np.nan):
        w[first][0] = bad
        refused_table(capi.ERR_INVALID, R.HOP2, R.Table(hop2.rows, w))
        refused_table(capi.ERR_INVALID, R.HOP1, R.Table([[1, 2]], [[0.5, bad]]))
    refused_table(capi.ERR_INVALID, R.HOP2, R.Table(hop2.rows, hop2.weights, R.RAW, np.inf))
    refused_table(capi.ERR_INVALID, 2, hop2)
    check(h, hop1, hop2, list(range(8)), 10, None, want)
    R.Table([[1, 2, 1]], [[0.5, 0.25, 0.5]]).set_on(h, R.HOP1)  # a weighted hop-1 row may repeat: successive lists
    check(h, R.Table([[1, 2, 1]], [[0.5, 0.25, 0.5]]), hop2, [0], 10)
    # a hop-1 index outside the hop-2 table's rows shows at the call, whichever table came last
    R.Table([[0, n_items]]).set_on(h, R.HOP1)
    refused(capi.ERR_RANGE, 1, 10)
    hop1.set_on(h, R.HOP1)
    R.Table(hop2.rows[:5], hop2.weights[:5]).set_on(h, R.HOP2)
    refused(capi.ERR_RANGE, 1, 10)
