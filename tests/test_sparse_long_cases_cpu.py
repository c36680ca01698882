"""The inputs of tests/test_gpu_sparse_long_rows.py can fail a wrong kernel (no GPU): the builders of tests/sparse_cases.py give the
stated lengths, the scores of L's long rows depend on the order of their terms and every one of them is ranked, the hand-built query
has the stated matches per 64-entry step, and W is past the two bounds it is built for."""
import numpy as np

import sparse_cases as SC


def test_rows_with_lengths_gives_the_lengths_asked_for():
    rng = np.random.default_rng(3)
    lengths = [0, 1, 64, 0, 200, 7]
    for wide in (False, True):
        ptr, idx, val = SC.rows_with_lengths(rng, 200, lengths, wide=wide)
        assert np.diff(ptr).tolist() == lengths and ptr[0] == 0 and idx.dtype == np.uint32 and val.dtype == np.float32
        for r in range(len(lengths)):
            row = idx[ptr[r]:ptr[r + 1]].astype(np.int64)
            assert (np.diff(row) > 0).all() and (row < 200).all()
        assert idx[ptr[4]:ptr[5]].tolist() == list(range(200))  # a row that holds every index
        assert (val < 0).any() and (val > 0).any() and (val != 0).all()
        spread = np.abs(val).max() / np.abs(val).min()
        assert spread > 1e6 if wide else spread < 30


def test_long_rows_collection_has_the_stated_rows():
    for last in (False, True):
        ptr, idx, val, long_rows = SC.long_rows_case(long_row_last=last)
        lens = np.diff(ptr)
        assert lens.size == 600 and 28000 < lens.sum() < 34000
        assert [int(lens[r]) for r in long_rows] == SC.L_LONG
        assert sorted(x % 64 for x in SC.L_LONG[:6]) == [0, 0, 1, 1, 2, 63] and SC.L_LONG[9] == SC.L_DIMS
        assert int((lens > 1024).sum()) == 11 and int((lens == 1024).sum()) == 1  # both sides of the whole-wave walk's threshold
        others = np.delete(lens, long_rows)
        assert others.max() <= 40 and int((others == 0).sum()) >= 5
        assert (int(lens[-1]) > 1024) == last  # the look-ahead of the last step ends at the arrays' end
        assert long_rows != sorted(long_rows)  # shuffled
    qp, qi, qv = SC.long_rows_queries(ptr, idx, val, long_rows)
    assert np.diff(qp).tolist()[:-1] == SC.L_QUERY_LENGTHS
    assert int((np.diff(qp) > SC.L_THRESHOLD).sum()) == 6 and np.diff(qp)[0] <= SC.L_THRESHOLD


def test_hand_built_query_has_the_stated_matches_per_step():
    ptr, idx, val, long_rows = SC.long_rows_case()
    qp, qi, qv = SC.long_rows_queries(ptr, idx, val, long_rows)
    hand = qi[qp[-2]:qp[-1]]
    assert (np.diff(hand.astype(np.int64)) > 0).all() and hand.size > SC.L_THRESHOLD
    r = long_rows[SC.L_LONG.index(1089)]
    row = idx[ptr[r]:ptr[r + 1]]
    steps = SC.step_matches(row, hand)
    assert len(steps) == 18 and steps[:4] == [16, 17, 64, 0] and steps[17] == 1
    assert any(0 < s <= 16 for s in steps[4:17]) and any(s > 16 for s in steps[4:17])
    assert hand.size - sum(steps) == 40  # indices that the row lacks
    # the random queries: about 5, 16 and 31 matches per step of the longest rows -- the per-match form, both forms within one row, all lanes
    r = long_rows[SC.L_LONG.index(3000)]
    row = idx[ptr[r]:ptr[r + 1]]
    per_step = {n: SC.step_matches(row, qi[qp[t]:qp[t + 1]])[:-1] for t, n in enumerate(SC.L_QUERY_LENGTHS)}
    assert max(per_step[300]) <= 16
    assert min(per_step[1050]) <= 16 < max(per_step[1050])
    assert min(per_step[2000]) > 16
    assert set(per_step[4096]) == {64}


def test_long_row_scores_depend_on_the_order_of_their_terms(oracle):
    """the oracle's products added in reverse order (float32): at least half of the (query, long row) scores change their bits;
    with k = 1024 (at least the number of rows) every long row is in the result of every query that shares an index with it"""
    ptr, idx, val, long_rows = SC.long_rows_case()
    qp, qi, qv = SC.long_rows_queries(ptr, idx, val, long_rows)
    pairs = changed = 0
    for t in range(qp.size - 1):
        q_idx, q_val = qi[qp[t]:qp[t + 1]], qv[qp[t]:qp[t + 1]]
        rows, scores = oracle.sparse_search(ptr, idx, val, q_idx, q_val, 1024)
        got = dict(zip(rows.tolist(), scores.view(np.uint32).tolist()))
        for r in long_rows:
            r_idx, r_val = idx[ptr[r]:ptr[r + 1]], val[ptr[r]:ptr[r + 1]]
            _, at_q, at_r = np.intersect1d(q_idx, r_idx, assume_unique=True, return_indices=True)
            if at_q.size == 0:
                assert r not in got
                continue
            prod = q_val[at_q] * r_val[at_r]  # float32, ascending index
            assert prod.dtype == np.float32
            forward, backward = np.add.accumulate(prod)[-1], np.add.accumulate(prod[::-1])[-1]
            assert got[r] == int(forward.view(np.uint32)), (t, r)  # ranked, with the in-order sum
            pairs += 1
            changed += int(forward.view(np.uint32) != backward.view(np.uint32))
    print("(query, long row) scores: %d, of them changed by the reverse order: %d" % (pairs, changed))
    assert pairs >= 6 * 12 and 2 * changed >= pairs


def test_production_thresholds_collection_has_the_stated_rows():
    ptr, idx, val = SC.production_thresholds_case()
    lens = np.diff(ptr)
    assert 2140 <= lens.size <= 2160 and 340000 < lens.sum() < 410000
    assert sorted(lens[lens > 16383].tolist()) == sorted(SC.B_HEAVY)
    assert int((lens > 16384).sum()) == 11
    assert int((lens > 2048).sum()) == 12 + 2 + 30 and int((lens == 2048).sum()) == 1
    assert all(int((lens == n).sum()) >= 1 for n in SC.B_MIDDLE)
    assert int((lens <= 30).sum()) == 2100 and int((lens == 0).sum()) > 0
    assert np.unique(idx).size == SC.B_DIMS


def test_wide_directory_collection_is_past_both_bounds():
    ptr, idx, val, shared = SC.wide_directory_case()
    lens = np.diff(ptr)
    assert lens.size == SC.W_ROWS and 14 <= lens.min() and lens.max() <= 19 + 8 + 4
    for r in range(0, SC.W_ROWS, 499):
        assert (np.diff(idx[ptr[r]:ptr[r + 1]].astype(np.int64)) > 0).all()
    distinct, count = np.unique(idx, return_counts=True)
    private = ~np.isin(distinct, shared)
    assert (count[private] == 1).all() and shared.size == SC.W_SHARED and int((~private).sum()) == SC.W_SHARED
    assert np.diff(distinct.astype(np.int64)).max() > 1 and distinct.size < 0.6 * SC.W_SPACE  # gaps in the index space
    groups = -(-SC.W_ROWS // 256)
    cells = distinct.size * groups
    assert groups == 47 and cells + 1 > 1024 * 8192  # sparse_scan_top_kernel: two chunk sums per thread
    assert -(-(cells + 1) // 8192) > 1024
    n_long = int((lens > SC.W_LONG).sum())
    bound = SC.dense_copy_bound(distinct.size)
    assert bound < 32768 and n_long > 2 * bound and n_long % bound != 0  # several rounds, the last one partly full
    print("W: %d entries, %d distinct indices, %d rows longer than %d, %d long queries per round" %
          (idx.size, distinct.size, n_long, SC.W_LONG, bound))
