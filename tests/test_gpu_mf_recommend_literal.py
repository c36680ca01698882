"""gorse_mf_recommend under literal mode 1 (gorse_mf_set_recommend_literal(h, 1), csrc/recommend_literal.hip): one workgroup per literal
query, the heap in LDS, candidates below the root fast-forwarded where push + pop would move nothing.

The expected rows are test_gpu_mf_recommend's: numpy candidate lists ranked and scored by the oracle's Rank + heap.TopKFilter.  Every
case runs mode 1, asserts what the getter says, holds items, counts, padding and score bits to the oracle, and holds the threshold /
literal split to mode 0's on the same handle."""
import numpy as np
import pytest

from gorse_amd import capi
from test_gpu_mf_recommend import _hooks_at_default, csr, expected, make_mf  # noqa: F401 (the fixture resets the hooks)

pytestmark = pytest.mark.gpu


def run(mf, P, Q, rows, users, k, ok=None, seen=None, used=1):
    """mode 0 for the split, then mode 1 against the oracle; returns (mode 1's literal stats, mode 1's rows, the split)"""
    exp_i, exp_s, exp_c, _ = expected(P, Q, rows, users, k, ok, seen)
    sp, si = csr(seen) if seen is not None else (None, None)
    mf.set_recommend_literal(0)
    mf.recommend(users, k, ok, sp, si)
    split0 = mf.recommend_stats()[:2]
    assert mf.recommend_literal() == (0, 0) and mf.recommend_literal_stats() == (0, 0, 0)
    mf.set_recommend_literal(1)
    got = mf.recommend(users, k, ok, sp, si)
    assert mf.recommend_literal() == (1, used)
    assert np.array_equal(got[2], exp_c), (got[2], exp_c)
    bad = np.flatnonzero((got[0] != exp_i).any(axis=1))
    assert bad.size == 0, (bad[:10], got[0][bad[0]], exp_i[bad[0]])
    assert np.array_equal(got[1].view(np.uint32), exp_s.view(np.uint32))
    assert mf.recommend_stats()[:2] == split0
    stats = mf.recommend_literal_stats()
    assert stats[0] == (split0[1] if used else 0)
    return stats, got, split0


N_SEQ = 700  # two tiles and a ragged segment; longer than the longest plateau (k = 256)


def ranked(n, k, rng, equal=(), put=()):
    """distinct scores in random item order; the scores of the ranks (0 = best) in `equal` made one value, `put` = (rank, value) pairs"""
    order = rng.permutation(n)  # order[r] = the item of rank r
    s = np.empty(n, np.float32)
    s[order] = -np.arange(n, dtype=np.float32)
    if len(equal):
        s[order[np.asarray(equal)]] = s[order[equal[0]]]
    for r, v in put:
        s[order[r]] = v
    return s


NAN = np.float32(np.nan)
SEQUENCES = {
    "ascending": lambda n, k, g: np.arange(n, dtype=np.float32),
    "descending": lambda n, k, g: -np.arange(n, dtype=np.float32),
    "ascending_top_pair": lambda n, k, g: np.minimum(np.arange(n), n - 2).astype(np.float32),   # everything is pushed
    "descending_top_pair": lambda n, k, g: -np.maximum(np.arange(n), 1).astype(np.float32),     # everything behind the first k is below the root
    "all_equal": lambda n, k, g: np.full(n, 2.5, np.float32),
    "two_values": lambda n, k, g: np.where(np.arange(n) % 2 == 0, 1.0, 2.0).astype(np.float32),
    "plateau_across_the_cut": lambda n, k, g: ranked(n, k, g, equal=list(range(max(0, k - 3), 2 * k + 6))),
    "pair_at_the_top": lambda n, k, g: ranked(n, k, g, equal=[0, 1]),
    "pair_at_the_cut": lambda n, k, g: ranked(n, k, g, equal=[k - 1, k]),
    "pair_below_the_cut": lambda n, k, g: ranked(n, k, g, equal=[k, k + 1]),
    "signed_zeros": lambda n, k, g: np.where(np.arange(n) % 3 == 0, -np.arange(n) - 1.0, np.where(np.arange(n) % 2 == 0, 0.0, -0.0)).astype(np.float32),
    "infinities": lambda n, k, g: ranked(n, k, g, put=[(0, np.inf), (1, np.inf), (5, np.inf), (n - 1, -np.inf), (n - 2, -np.inf)]),
    "nan_first": lambda n, k, g: np.concatenate([[NAN], g.standard_normal(n - 1)]).astype(np.float32),
    "nan_middle": lambda n, k, g: np.concatenate([g.standard_normal(n // 2), [NAN], g.standard_normal(n - n // 2 - 1)]).astype(np.float32),
    "nan_last": lambda n, k, g: np.concatenate([g.standard_normal(n - 1), [NAN]]).astype(np.float32),
    "two_nans": lambda n, k, g: np.concatenate([g.standard_normal(300), [NAN], g.standard_normal(n - 302), [-NAN]]).astype(np.float32),
}


@pytest.mark.parametrize("k", [1, 2, 3, 4, 7, 8, 100, 256])
@pytest.mark.parametrize("name", sorted(SEQUENCES))
def test_scores_set_literally(name, k):
    """P[0] = e_0 and Q[:, 0] = the sequence, every other column -0: the score of item i is Q[i, 0] bit for bit (x + -0 = x, and
    -0 + -0 = -0), in item order.  k = 1, 2: the rule without a condition; odd and even k: left- and right-child path steps; ties on
    and off the ancestor path; a NaN at the root"""
    seq = SEQUENCES[name](N_SEQ, k, np.random.default_rng(k))
    Q = np.full((N_SEQ, 16), -0.0, np.float32)
    Q[:, 0] = seq
    P = np.zeros((1, 16), np.float32)
    P[0, 0] = 1.0
    rows = [np.zeros(0, np.int32)]
    (nq, pushed, skipped), got, _ = run(make_mf(P, Q, rows), P, Q, rows, np.zeros(1, np.int32), k, ok=np.ones(N_SEQ, np.uint8))
    assert pushed + skipped == nq * N_SEQ
    if name == "ascending_top_pair":
        assert (nq, skipped) == (1, 0)
    if name == "descending_top_pair" and k == 1:
        assert (nq, pushed) == (1, 2)


@pytest.mark.parametrize("k", [257, 1000, 1300])
@pytest.mark.parametrize("d", [8, 16, 24, 64, 129, 256])
def test_every_query_literal_without_ties(d, k):
    """k > 256: every query is literal; the user's row in registers (16, 64) and in LDS (8, 24, 129, 256).  k = 1300 is more than any
    query's candidates: the heap never fills and nothing can be skipped; below that the fast-forward must have skipped something"""
    n_items = 1200
    rng = np.random.default_rng(d + k)
    P = rng.standard_normal((6, d)).astype(np.float32)
    Q = rng.standard_normal((n_items, d)).astype(np.float32)
    rows = [rng.choice(n_items, int(rng.integers(0, 150)), replace=False).astype(np.int32) for _ in range(6)]
    users = np.arange(6, dtype=np.int32)
    ok = np.ones(n_items, np.uint8)
    total = sum(n_items - r.size for r in rows)
    mf = make_mf(P, Q, rows)
    (nq, pushed, skipped), got, _ = run(mf, P, Q, rows, users, k, ok=ok)
    assert nq == 6 and pushed + skipped == total and (skipped > 0) == (k < n_items - 150)
    capi.lib().gorse_hip_test_set_recommend_literal(1)
    try:
        (nq, pushed, skipped), serial, _ = run(mf, P, Q, rows, users, k, ok=ok)
    finally:
        capi.lib().gorse_hip_test_set_recommend_literal(0)
    assert (nq, pushed, skipped) == (6, total, 0)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got, serial))


def paired(n_users, n_items, d, seed):
    """items in identical pairs: every query with two candidates of one pair among its k + 1 best is tied"""
    rng = np.random.default_rng(seed)
    P = rng.standard_normal((n_users, d)).astype(np.float32)
    Q = rng.standard_normal((n_items, d)).astype(np.float32)
    Q[1::2] = Q[0:n_items - 1:2][: Q[1::2].shape[0]]
    return P, Q, rng


@pytest.mark.parametrize("k", [10, 100])
def test_every_query_tied(k):
    P, Q, rng = paired(40, 1031, 32, k)
    P[7] = 0.0  # every score is 0: the heap is one plateau and nothing may be skipped
    rows = [rng.choice(1031, int(rng.integers(0, 200)), replace=False).astype(np.int32) for _ in range(40)]
    rows[7] = np.zeros(0, np.int32)
    mf = make_mf(P, Q, rows)
    ok = np.ones(1031, np.uint8)
    (nq, _, skipped), _, _ = run(mf, P, Q, rows, np.arange(40, dtype=np.int32), k, ok=ok)
    assert nq >= 35 and skipped > 0
    assert run(mf, P, Q, rows, np.array([7], np.int32), k, ok=ok)[0] == (1, 1031, 0)


@pytest.mark.parametrize("n_items,k", [(255, 5), (256, 5), (257, 5), (4099, 257)])
def test_tile_and_candidate_count_edges(n_items, k):
    """catalogues around a segment and across tiles; a users array with repeats and a -1; an item filter and unsorted seen rows with
    repeats that leave queries 0, 1, k and k + 1 candidates (k = 257: every query is literal, the empty one included)"""
    P, Q, rng = paired(9, n_items, 48, n_items)
    rows = [rng.choice(n_items, 20, replace=False).astype(np.int32) for _ in range(9)]
    users = np.array([3, 3, -1, 0, 8, 5, 3, 1], np.int32)
    ok = np.ones(n_items, np.uint8)
    ok[rng.choice(n_items, n_items // 10, replace=False)] = 0
    seen = []
    for t, left in enumerate([0, 1, None, k, k + 1, None, None, 2]):
        if left is None or users[t] < 0:
            s = rng.integers(0, n_items, 30).astype(np.int32)
        else:  # everything but the first `left` admissible items outside the training row
            free = np.setdiff1d(np.flatnonzero(ok), rows[users[t]])
            s = rng.permutation(np.setdiff1d(np.arange(n_items), free[:left])).astype(np.int32)
        seen.append(np.concatenate([s, s[:7]]).astype(np.int32))
    _, got, split = run(make_mf(P, Q, rows), P, Q, rows, users, k, ok=ok, seen=seen)
    assert got[2].tolist()[:5] == [0, 1, 0, k, k] and split[1] >= (7 if k > 256 else 1)


def test_k_beyond_the_lds_budget_takes_mode_0():
    P, Q, rng = paired(4, 600, 16, 1)
    rows = [rng.choice(600, 30, replace=False).astype(np.int32) for _ in range(4)]
    stats, _, split = run(make_mf(P, Q, rows), P, Q, rows, np.arange(4, dtype=np.int32), 8000, used=0)
    assert stats == (0, 0, 0) and split == (0, 4)


def test_candidate_chain_follows_the_handle_and_bad_modes_are_refused():
    P, Q, rng = paired(140, 1000, 48, 2)
    rows = [rng.choice(1000, int(rng.integers(0, 300)), replace=False).astype(np.int32) for _ in range(140)]
    mf = make_mf(P, Q, rows)
    users = np.arange(0, 140, 3, dtype=np.int32)
    got = []
    for mode in (0, 1):
        mf.set_recommend_literal(mode)
        chain = capi.CandidateChain(1000)
        chain.begin(users.size, 20, *csr([rows[u][:30] for u in users]))
        chain.add_mf(mf, users, 15)
        chain.finish()
        got.append(chain.get())
        assert mf.recommend_literal() == (mode, mode) and mf.recommend_stats()[1] > 0
        assert (mf.recommend_literal_stats()[0] == mf.recommend_stats()[1]) == (mode == 1)
        chain.close()
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(*got)) and got[0][0][-1] > 0
    for bad in (2, -1):
        with pytest.raises(capi.GorseHipError) as e:
            mf.set_recommend_literal(bad)
        assert e.value.code == capi.ERR_INVALID and mf.recommend_literal()[0] == 1
