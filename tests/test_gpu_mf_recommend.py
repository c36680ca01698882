"""gorse_mf_recommend: every query's k best unseen items from the resident model (csrc/recommend.hip).

Expected rows never come from the code under test: the candidate lists are built in numpy from the contract in include/gorse_hip.h
(item filter, training row, seen row; ascending), ranked by the oracle's Rank + heap.TopKFilter (oracle.mf_rank) and scored by
oracle.mf_score.  Items, counts, the -1 / 0 padding and the score bits must be equal, and the split between the threshold kernel and
the literal path must be the one the tie rule states: a query is literal iff two of its k + 1 best candidate scores compare equal."""
import ctypes as C
import functools

import numpy as np
import pytest

from gorse_amd import capi
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

U, I = 300, 1031  # I is no multiple of any tile, slice or step of the kernels
FAST_CAP = 256    # the threshold kernel serves k <= 256


@functools.lru_cache(maxsize=None)
def _oracle():
    return orc.Oracle()


@functools.lru_cache(maxsize=None)
def base_rows():
    """training rows from empty to nearly full; 40 items nobody has touched (the default item filter drops them); user 1 has every
    other item (no candidate left), user 2 leaves 7 candidates (a short row for k >= 10)"""
    rng = np.random.default_rng(11)
    dead = rng.choice(I, 40, replace=False)
    live = np.setdiff1d(np.arange(I), dead)
    rows = []
    for u in range(U):
        if u == 0:
            n = 0
        elif u == 1:
            n = live.size
        elif u == 2:
            n = live.size - 7
        else:
            n = int(rng.integers(0, live.size - 300)) if u % 3 else int(rng.integers(0, 60))
        rows.append(rng.permutation(live)[:n].astype(np.int32))  # stored order: unsorted
    return rows


def csr(rows):
    ptr = np.zeros(len(rows) + 1, np.int64)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    idx = np.concatenate([np.asarray(r, np.int32) for r in rows] + [np.zeros(0, np.int32)]).astype(np.int32)
    return ptr, idx


@functools.lru_cache(maxsize=None)
def base_factors(d):
    rng = np.random.default_rng(1000 + d)
    return rng.standard_normal((U, d)).astype(np.float32), rng.standard_normal((I, d)).astype(np.float32)


def make_mf(P, Q, rows):
    ptr, idx = csr(rows)
    mf = capi.MF(P.shape[0], Q.shape[0], P.shape[1], ptr, idx if idx.size else np.zeros(1, np.int32))
    mf.set_factors(P, Q)
    return mf


def default_ok(rows, n_items):
    cnt = np.zeros(n_items, np.int64)
    for r in rows:
        np.add.at(cnt, r, 1)
    return (cnt > 0).astype(np.uint8)


def expected(P, Q, rows, users, k, ok=None, seen=None):
    """(items, scores, counts, tied): the contract, by numpy and the oracle; tied[t] = two of the k + 1 best candidate scores are equal"""
    o = _oracle()
    n_items = Q.shape[0]
    ok = default_ok(rows, n_items) if ok is None else np.asarray(ok, np.uint8)
    users = np.asarray(users, np.int32)
    n = users.size
    items = np.full((n, k), -1, np.int32)
    scores = np.zeros((n, k), np.float32)
    counts = np.zeros(n, np.int32)
    tied = np.zeros(n, bool)
    valid = [t for t in range(n) if users[t] >= 0]
    if not valid:
        return items, scores, counts, tied
    cands = []
    for t in valid:
        m = ok.astype(bool).copy()
        m[rows[users[t]]] = False
        if seen is not None:
            m[np.asarray(seen[t], np.int64)] = False
        cands.append(np.flatnonzero(m).astype(np.int32))
    ptr, cat = csr(cands)
    cat_safe = cat if cat.size else np.zeros(1, np.int32)
    vu = users[valid]
    rank, rlen = o.mf_rank(P, Q, vu, ptr, cat_safe, k)
    sc = o.mf_score(P, Q, np.repeat(vu, np.diff(ptr)).astype(np.int32), cat) if cat.size else np.zeros(0, np.float32)
    for j, t in enumerate(valid):
        ln = int(rlen[j])
        counts[t] = ln
        assert ln == min(k, cands[j].size)
        if ln:
            items[t, :ln] = rank[j, :ln]
            scores[t, :ln] = o.mf_score(P, Q, np.full(ln, vu[j], np.int32), rank[j, :ln])
        top = np.sort(sc[ptr[j]:ptr[j + 1]])[::-1][:k + 1]
        tied[t] = bool(np.any(top[:-1] == top[1:]))
    return items, scores, counts, tied


def check(mf, P, Q, rows, users, k, ok=None, seen=None, users_arg="same"):
    """one call against the oracle, path accounting included; users_arg lets a caller pass None / a count for `users`"""
    exp_i, exp_s, exp_c, tied = expected(P, Q, rows, users, k, ok, seen)
    sp = si = None
    if seen is not None:
        sp, si = csr(seen)
    got_i, got_s, got_c = mf.recommend(users if isinstance(users_arg, str) else users_arg, k, ok, sp, si)
    assert np.array_equal(got_c, exp_c), np.flatnonzero(got_c != exp_c)[:10]
    bad = np.flatnonzero((got_i != exp_i).any(axis=1))
    assert bad.size == 0, (bad[:10], got_i[bad[0]], exp_i[bad[0]])
    assert np.array_equal(got_s.view(np.uint32), exp_s.view(np.uint32))
    n_fast, n_lit, ms = mf.recommend_stats()
    n = len(users)
    assert n_fast + n_lit == n and ms >= 0.0
    if k <= FAST_CAP:
        assert n_lit == int(tied.sum()), (n_lit, int(tied.sum()))
        assert n_fast == n - int(tied.sum())
    return got_i, got_s, got_c, n_fast, n_lit


@pytest.fixture(autouse=True)
def _hooks_at_default():
    yield
    capi.lib().gorse_hip_test_set_recommend(0, 0, 0)


def base_seen(users, rng):
    """seen rows per query: empty, unsorted, with duplicates, overlapping the user's training row"""
    rows = base_rows()
    out = []
    for t, u in enumerate(users):
        if t % 4 == 0 or u < 0:
            out.append(np.zeros(0, np.int32))
            continue
        s = rng.integers(0, I, int(rng.integers(1, 120))).astype(np.int32)  # unsorted
        s = np.concatenate([s, s[: s.size // 3], rows[u][:5]]).astype(np.int32)  # repeats, and part of the training row
        out.append(s)
    return out


@pytest.mark.parametrize("d", [1, 8, 15, 16, 24, 32, 40, 48, 64, 80, 96, 100, 112, 128, 129, 256])
def test_every_width_all_users(d):
    """users = NULL: every chunk count of the register form (16, 32, ... 128: at 48, 80, 96 and 112 the kernel's register dot meets
    the LDS dot of gorse_mf_score's kernel, and the bits must still agree), the 8-lane tail (8, 24, 40), the scalar tail (1, 15, 100,
    129), the LDS form (everything that is no multiple of 16, and 256)"""
    P, Q = base_factors(d)
    rows = base_rows()
    mf = make_mf(P, Q, rows)
    _, _, cnt, n_fast, _ = check(mf, P, Q, rows, np.arange(U, dtype=np.int32), 10, users_arg=None)
    assert cnt[1] == 0 and cnt[2] == 7 and n_fast > 0


@pytest.mark.parametrize("k", [1, 10, 100, 256, 300])
def test_every_k_with_user_lists_and_seen_rows(k):
    """a user list with repeats and -1 entries, seen rows of every kind; k = 300 is above the threshold kernel's cap (all literal)"""
    P, Q = base_factors(64)
    rows = base_rows()
    rng = np.random.default_rng(5 + k)
    users = rng.integers(0, U, 120).astype(np.int32)
    users[:8] = [1, 2, 2, -1, 0, 17, 17, -1]
    seen = base_seen(users, rng)
    mf = make_mf(P, Q, rows)
    _, _, cnt, n_fast, n_lit = check(mf, P, Q, rows, users, k, seen=seen)
    assert cnt[0] == 0 and cnt[3] == 0
    if k <= FAST_CAP:
        assert n_fast > 0
    else:
        assert n_lit == int((users >= 0).sum())


def test_accounting_on_all_users_at_every_k():
    """the threshold kernel answers whoever the tie rule lets it answer: on random factors that is nearly everybody"""
    P, Q = base_factors(64)
    rows = base_rows()
    mf = make_mf(P, Q, rows)
    for k in (1, 10, 100, 256):
        _, _, _, n_fast, n_lit = check(mf, P, Q, rows, np.arange(U, dtype=np.int32), k)
        assert n_fast > 0 and n_lit <= 0.05 * U


def test_one_query_and_first_n_users():
    P, Q = base_factors(40)
    rows = base_rows()
    mf = make_mf(P, Q, rows)
    check(mf, P, Q, rows, np.array([5], np.int32), 10)
    check(mf, P, Q, rows, np.arange(1, dtype=np.int32), 10, users_arg=1)  # users = NULL, n_users = 1
    check(mf, P, Q, rows, np.arange(37, dtype=np.int32), 10, users_arg=37)


def test_item_filter():
    P, Q = base_factors(64)
    rows = base_rows()
    mf = make_mf(P, Q, rows)
    users = np.arange(U, dtype=np.int32)
    ok = np.zeros(I, np.uint8)
    ok[[3, 400, 401, 999, 1030]] = 1
    _, _, cnt, _, _ = check(mf, P, Q, rows, users, 10, ok=ok)
    assert cnt.max() <= 5 and cnt[0] == 5
    _, _, cnt, _, _ = check(mf, P, Q, rows, users, 10, ok=np.zeros(I, np.uint8))
    assert not cnt.any()
    # an explicit filter may admit items without feedback
    check(mf, P, Q, rows, users, 10, ok=np.ones(I, np.uint8))


def test_seen_rows_equal_training_rows_of_a_second_handle():
    P, Q = base_factors(64)
    rows = base_rows()
    rng = np.random.default_rng(77)
    users = np.arange(U, dtype=np.int32)
    seen = base_seen(users, rng)
    ok = default_ok(rows, I)
    mf = make_mf(P, Q, rows)
    a = check(mf, P, Q, rows, users, 25, ok=ok, seen=seen)
    rows2 = [np.concatenate([rows[u], seen[u]]).astype(np.int32) for u in range(U)]
    mf2 = make_mf(P, Q, rows2)
    b = mf2.recommend(users, 25, ok)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and np.array_equal(a[2], b[2])


def monotone_case():
    """user 0 / 1: P = +e_0 / -e_0 against Q[:, 0] strictly increasing: every item beats the running threshold (a compaction whenever
    the buffer fills) / nothing passes behind the first k + 1; users 2 / 3: the same with their 50 best items in the training row"""
    d, n_items = 16, I
    rng = np.random.default_rng(3)
    Q = rng.standard_normal((n_items, d)).astype(np.float32)
    Q[:, 0] = np.linspace(-3.0, 3.0, n_items).astype(np.float32)
    assert np.all(np.diff(Q[:, 0]) > 0)
    P = np.zeros((4, d), np.float32)
    P[[0, 2], 0] = 1.0
    P[[1, 3], 0] = -1.0
    rows = [np.array([7], np.int32), np.array([500], np.int32), np.arange(n_items - 50, n_items, dtype=np.int32)[::-1].copy(),
            np.arange(50, dtype=np.int32)]
    return P, Q, rows


@pytest.mark.parametrize("forced", [(0, 0), (1, 1), (3, 1), (8, 0)])
def test_ascending_and_descending_scores(forced):
    P, Q, rows = monotone_case()
    mf = make_mf(P, Q, rows)
    capi.lib().gorse_hip_test_set_recommend(forced[0], forced[1], 0)
    users = np.arange(4, dtype=np.int32)
    for k in (1, 10, 100):
        got_i, _, _, n_fast, _ = check(mf, P, Q, rows, users, k, ok=np.ones(I, np.uint8))
        assert n_fast == 4
        assert got_i[0, 0] == I - 1 and got_i[1, 0] == 0 and got_i[2, 0] == I - 51 and got_i[3, 0] == 50


@pytest.mark.parametrize("slices,buffer", [(1, 0), (2, 0), (3, 0), (4, 0), (5, 0), (6, 0), (7, 0), (8, 0), (0, 1), (8, 1), (1, 40)])
def test_forced_forms_equal_the_unforced_call(slices, buffer):
    """every slice count and the smallest survivor buffer (a compaction per survivor), on the base shape"""
    P, Q = base_factors(64)
    rows = base_rows()
    rng = np.random.default_rng(9)
    users = np.arange(U, dtype=np.int32)
    seen = base_seen(users, rng)
    sp, si = csr(seen)
    mf = make_mf(P, Q, rows)
    for k in (10, 100):
        plain = mf.recommend(users, k, None, sp, si)
        capi.lib().gorse_hip_test_set_recommend(slices, buffer, 0)
        forced = check(mf, P, Q, rows, users, k, seen=seen)
        capi.lib().gorse_hip_test_set_recommend(0, 0, 0)
        assert np.array_equal(plain[0], forced[0]) and np.array_equal(plain[2], forced[2])
        assert np.array_equal(plain[1].view(np.uint32), forced[1].view(np.uint32))


def test_forced_forms_lds_width():
    P, Q = base_factors(100)
    rows = base_rows()
    mf = make_mf(P, Q, rows)
    capi.lib().gorse_hip_test_set_recommend(4, 1, 0)
    check(mf, P, Q, rows, np.arange(U, dtype=np.int32), 10)


@pytest.mark.parametrize("literal_chunk", [0, 1500])
def test_ties_come_out_as_the_heap_orders_them(literal_chunk):
    d = 24
    rng = np.random.default_rng(21)
    P = rng.standard_normal((40, d)).astype(np.float32)
    Q = rng.standard_normal((I, d)).astype(np.float32)
    rows = [rng.choice(I, int(rng.integers(0, 300)), replace=False).astype(np.int32) for _ in range(40)]
    # identical rows among everybody's best: a large common component on items 100, 101, 900 (equal rows) and 350
    Q[100] = Q[101] = Q[900] = 4.0 * np.sign(P.mean(axis=0) + 1e-3)
    P[:20] = np.abs(P[:20]) * np.sign(Q[100])  # users 0..19 score the three identical rows highest
    # all-zero user rows: every score is +-0
    P[20:30] = 0.0
    # rows that differ only in the sign of zero: users 30..39 have zeros where these two rows differ
    Q[500] = Q[501] = 5.0 * np.sign(P[35] + 1e-3)
    Q[500, :4] = 0.0
    Q[501, :4] = -0.0
    P[30:40, :4] = np.float32(-0.0)
    P[30:40, 4:] = np.abs(P[30:40, 4:]) * np.sign(Q[500, 4:])
    for u in range(40):
        rows[u] = np.setdiff1d(rows[u], [100, 101, 900, 500, 501]).astype(np.int32)
    mf = make_mf(P, Q, rows)
    capi.lib().gorse_hip_test_set_recommend(0, 0, literal_chunk)
    users = np.arange(40, dtype=np.int32)
    ok = np.ones(I, np.uint8)
    for k in (1, 2, 10, 100):
        _, _, _, _, n_lit = check(mf, P, Q, rows, users, k, ok=ok)
        assert n_lit >= 10  # the all-zero rows at the least
    capi.lib().gorse_hip_test_set_recommend(2, 1, literal_chunk)
    check(mf, P, Q, rows, users, 10, ok=ok)


def item_csr(rows, n_items):
    u = np.repeat(np.arange(len(rows)), [len(r) for r in rows]).astype(np.int32)
    i = np.concatenate(rows).astype(np.int32)
    order = np.argsort(i, kind="stable")
    ptr = np.zeros(n_items + 1, np.int64)
    ptr[1:] = np.cumsum(np.bincount(i, minlength=n_items))
    return ptr, u[order]


def test_recommend_orders_itself_behind_enqueued_epochs():
    """gorse_bpr_epoch_enqueue followed at once by recommend equals recommend after gorse_mf_synchronize.  The sequential schedule
    refuses to be enqueued (GORSE_ERR_INVALID, asserted below) and two Hogwild epochs on two handles differ, so the comparison is
    made on ONE handle: the call issued behind the enqueued epoch, the call after the synchronize, and the oracle on the factors
    read back afterwards must all agree -- which also shows that recommend leaves the factors untouched."""
    d = 32
    rng = np.random.default_rng(8)
    rows = [rng.choice(200, int(rng.integers(3, 40)), replace=False).astype(np.int32) for _ in range(120)]
    P = (0.1 * rng.standard_normal((120, d))).astype(np.float32)
    Q = (0.1 * rng.standard_normal((200, d))).astype(np.float32)
    ptr, idx = csr(rows)
    iptr, iidx = item_csr(rows, 200)
    mf = capi.MF(120, 200, d, ptr, idx, iptr, iidx)
    mf.set_factors(P, Q)
    with pytest.raises(capi.GorseHipError) as e:
        mf.bpr_epoch_enqueue(int(ptr[-1]), 0.05, 0.01, 7, 1, mode=capi.BPR_SEQUENTIAL)
    assert e.value.code == capi.ERR_INVALID
    mf.bpr_epoch_enqueue(400000, 0.05, 0.01, 7, 1, mode=capi.BPR_HOGWILD_ATOMIC)
    first = mf.recommend(None, 10)
    capi.check(capi.lib().gorse_mf_synchronize(mf.h))
    gP, gQ = mf.get_factors()
    second = mf.recommend(None, 10)
    assert not np.array_equal(gQ, Q)  # the epoch moved the factors
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[2], second[2])
    assert np.array_equal(first[1].view(np.uint32), second[1].view(np.uint32))
    exp_i, exp_s, exp_c, _ = expected(gP, gQ, rows, np.arange(120, dtype=np.int32), 10)
    assert np.array_equal(first[0], exp_i) and np.array_equal(first[2], exp_c)
    assert np.array_equal(first[1].view(np.uint32), exp_s.view(np.uint32))
    hP, hQ = mf.get_factors()
    assert np.array_equal(hP.view(np.uint32), gP.view(np.uint32)) and np.array_equal(hQ.view(np.uint32), gQ.view(np.uint32))


def test_errors_leave_the_outputs_untouched():
    P, Q = base_factors(16)
    rows = base_rows()
    mf = make_mf(P, Q, rows)
    L = capi.lib()
    u8p = C.POINTER(C.c_uint8)

    def call(users, k, sp=None, si=None):
        kk = max(k, 1)
        items = np.full((len(users), kk), -7, np.int32)
        scores = np.full((len(users), kk), 3.5, np.float32)
        counts = np.full(len(users), -7, np.int32)
        rc = L.gorse_mf_recommend(mf.h, len(users), capi._p(users, capi._i32p), k, C.cast(None, u8p), capi._p(sp, capi._i64p),
                                  capi._p(si, capi._i32p), capi._p(items, capi._i32p), capi._p(scores, capi._f32p),
                                  capi._p(counts, capi._i32p))
        assert (items == -7).all() and (scores == 3.5).all() and (counts == -7).all()
        return rc

    good = np.array([0, 5], np.int32)
    assert call(good, 0) == capi.ERR_INVALID
    assert call(good, -3) == capi.ERR_INVALID
    assert call(np.array([0, U], np.int32), 5) == capi.ERR_RANGE
    assert call(good, 5, np.array([0, 1, 2], np.int64), np.array([4, I], np.int32)) == capi.ERR_RANGE
    assert call(good, 5, np.array([0, 1, 2], np.int64), np.array([-1, 4], np.int32)) == capi.ERR_RANGE
    # users = NULL with more queries than the handle has users
    assert L.gorse_mf_recommend(mf.h, U + 1, None, 5, C.cast(None, u8p), None, None, None, None, None) == capi.ERR_INVALID
    # and the handle still answers
    check(mf, P, Q, rows, good, 5)
