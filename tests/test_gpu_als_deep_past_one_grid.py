"""The Deep ALS form (csrc/als_deep.hip) past one grid, one Gram chunk and eight partials: what the 200 rows of
tests/test_gpu_als_deep.py cannot reach.  deep_launch and the long solve cap their grids at cf_cases.GRID_ALS_DEEP_ITEMS workgroups and
stride; als_build_plan cuts the rows with feedback into Gram chunks of cf_cases.ALS_GRAM_CHUNK_ROWS; als_deep_reduce_kernel adds eight
partials per step and then a tail (the literals are held against the source by tests/test_als_deep_grid_caps_cpu.py).

One tall dataset under the row plan (16, 16): 64 items; 8193 users with feedback and seven empty ones among them (fb_rows is not the
identity); 2100 users of 17..33 entries (long rows of two or three chunks: a last chunk of one entry, of exactly 16, and three chunks)
and 6093 of 1..16.  Every item row then has about 1600 entries, a hundred chunks of 16.  test_the_tall_data_is_past_every_cap (no GPU)
derives from the data and a restatement of the plan rule that the user side's row kernel makes three trips, that its chunk kernel and
long solve and the item side's chunk kernel make a second one, that every item row's reduce runs its eight-wide loop (with and without
a tail) and that the users' Gram is nine chunks with a last chunk of one row."""
import numpy as np
import pytest

from cf_cases import ALS_GRAM_CHUNK_ROWS, GRID_ALS_DEEP_ITEMS, assert_als_close, bits, make_mf
from gorse_amd import capi, synth

gpu = pytest.mark.gpu

W, REG = 0.05, 0.015
LONG_ROW, CHUNK_LEN = 16, 16
N_ITEMS = 64
N_FB_USERS = 8 * ALS_GRAM_CHUNK_ROWS + 1        # nine Gram chunks, the last of one row
N_LONG_USERS = GRID_ALS_DEEP_ITEMS + 52         # users of 17..33 entries
EMPTY_USERS = (3, 1000, 2047, 2048, 4100, 6000, 8190)
N_USERS = N_FB_USERS + len(EMPTY_USERS)
USER_PIECES = [(lo, min(lo + GRID_ALS_DEEP_ITEMS, N_USERS)) for lo in range(0, N_USERS, GRID_ALS_DEEP_ITEMS)]
ITEM_PIECES = [(lo, lo + 16) for lo in range(0, N_ITEMS, 16)]  # (all 64 items are within one grid as rows: 16 keep a piece's CHUNKS within one)


def plan(lengths):
    """als_build_plan's row rule restated: (short rows, long rows, chunks per long row) of rows of these lengths"""
    n = np.asarray(lengths, np.int64)
    long = n[n > LONG_ROW]
    chunk = np.maximum(CHUNK_LEN, (-(-long // 256) + 15) // 16 * 16)
    return int((n <= LONG_ROW).sum()), int(long.size), -(-long // chunk)


def gram_chunks(lengths):
    """the row counts of the S Gram's chunks over rows of these lengths"""
    fb = int((np.asarray(lengths) > 0).sum())
    return [min(ALS_GRAM_CHUNK_ROWS, fb - b) for b in range(0, fb, ALS_GRAM_CHUNK_ROWS)]


@pytest.fixture(scope="module")
def tall():
    rng = np.random.default_rng(11)
    fb = np.setdiff1d(np.arange(N_USERS), EMPTY_USERS)
    long = rng.choice(fb, N_LONG_USERS, replace=False)
    n = np.zeros(N_USERS, np.int64)
    n[fb] = rng.integers(1, LONG_ROW + 1, fb.size)
    n[long] = rng.integers(17, 34, long.size)
    n[long[:3]] = (17, 32, 33)
    R = rng.random((N_USERS, N_ITEMS)).argsort(axis=1).argsort(axis=1) < n[:, None]  # n[u] distinct items of user u
    u, i = np.nonzero(R)
    uptr, uidx = synth._csr_from_pairs(u, i, N_USERS)
    iptr, iidx = synth._csr_from_pairs(i, u, N_ITEMS)
    assert np.array_equal(np.diff(uptr), n)
    z, e = np.zeros(N_USERS + 1, np.int64), np.zeros(0, np.int32)
    return synth.CFData(N_USERS, N_ITEMS, uptr, uidx, iptr, iidx, z, e, z.copy(), e.copy())


@pytest.fixture
def tall_plan():
    """rows of more than 16 entries are long ones, cut into chunks of 16 (handles created inside the test)"""
    capi.lib().gorse_hip_test_set_als_plan(LONG_ROW, CHUNK_LEN)
    yield
    capi.lib().gorse_hip_test_set_als_plan(0, 0)


def test_the_tall_data_is_past_every_cap(tall):
    grid = GRID_ALS_DEEP_ITEMS
    users, items = np.diff(tall.uptr), np.diff(tall.iptr)
    # user side: three trips of the row kernel, a second of the chunk kernel and of the long solve
    n_short, n_long, nch = plan(users)
    assert n_short > 2 * grid and n_long == N_LONG_USERS > grid and nch.sum() > grid
    assert {17, 32, 33} <= set(users.tolist()) and users.max() == 33 and set(nch.tolist()) == {2, 3}
    assert (users == 0).sum() == len(EMPTY_USERS) and users[-1] > 0 and users[0] > 0
    fb_rows = np.flatnonzero(users)
    assert not np.array_equal(fb_rows, np.arange(fb_rows.size)) and fb_rows.size == N_FB_USERS
    # item side: every row is long, a second trip of the chunk kernel, the reduce's eight-wide loop with and without a tail
    n_short, n_long, nch = plan(items)
    assert (n_short, n_long) == (0, N_ITEMS) and nch.sum() > grid
    assert nch.min() >= 8 and (nch % 8 == 0).any() and (nch % 8 != 0).any()
    assert (items % CHUNK_LEN != 0).any()
    # the Grams: the users' is nine chunks with a last chunk of one row (the reduce's eight-wide step, then its tail; an odd last pair
    # of the accumulation), the items' is one
    assert gram_chunks(users) == [ALS_GRAM_CHUNK_ROWS] * 8 + [1] and gram_chunks(items) == [N_ITEMS]
    # the pieces of the bit-equality test: each within one grid in rows, long rows and chunks, together the whole side
    for pieces, lengths in ((USER_PIECES, users), (ITEM_PIECES, items)):
        assert pieces[0][0] == 0 and pieces[-1][1] == lengths.size and all(a[1] == b[0] for a, b in zip(pieces, pieces[1:]))
        for lo, hi in pieces:
            n_short, n_long, nch = plan(lengths[lo:hi])
            assert hi - lo <= grid and max(n_short, n_long, int(nch.sum())) <= grid, (lo, hi)
    assert len(USER_PIECES) == 5 and len(ITEM_PIECES) == 4


def gram_half_fp64(A, B, ptr, idx, bptr, w=W):
    """tests/test_gpu_als_deep.py's float64 Gram half-sweep -- M = (1 - w) G + w S per row, one coordinate sweep over it -- 32 rows
    at a time (a block's M stays in cache) with one einsum per coordinate step.  Rows are independent within a half-sweep."""
    A, B = np.asarray(A, np.float64).copy(), np.asarray(B, np.float64)
    d = A.shape[1]
    has = np.diff(bptr) > 0
    wS = w * (B[has].T @ B[has])
    for r0 in range(0, A.shape[0], 32):
        p = A[r0:r0 + 32]
        M, s = np.empty((p.shape[0], d, d)), np.empty((p.shape[0], d))
        for k in range(p.shape[0]):
            Bu = B[idx[ptr[r0 + k]:ptr[r0 + k + 1]]]
            np.matmul(Bu.T, Bu, out=M[k])
            s[k] = Bu.sum(axis=0)
        M *= 1 - w
        M += wS
        diag = np.einsum("kff->kf", M).copy()
        for f in range(d):
            p[:, f] = (s[:, f] - (np.einsum("kd,kd->k", M[:, f], p) - diag[:, f] * p[:, f])) / (diag[:, f] + REG)
    return A


def half_sweeps(data, d, ranges=None):
    """((P, Q) at the start, P after a user half-sweep, Q after an item half-sweep), each half-sweep from the start values, in the
    Deep form on one fresh handle.  A side whose range is empty is not run (None)."""
    mf, P, Q = make_mf(data, d, std=0.1)
    mf.set_als_form(1)
    if ranges:
        mf.als_set_ranges(*ranges)
    out = []
    for side in (0, 1):
        if ranges and ranges[2 * side] == ranges[2 * side + 1]:
            out.append(None)
            continue
        mf.set_factors(P, Q)
        mf.als_half_epoch(side, W, REG)
        assert mf.als_form() == (1, capi.ALS_FAMILY_DEEP)
        out.append(mf.get_factors()[side])
    mf.close()
    return (P, Q), out[0], out[1]


_full = {}


def full_half_sweeps(data, d):
    """half_sweeps over the whole of both sides, run once per width and shared (nobody writes to it)"""
    if d not in _full:
        _full[d] = half_sweeps(data, d)
    return _full[d]


@gpu
@pytest.mark.parametrize("d", [130, 256])
def test_tall_half_sweeps_meet_the_float64_gram_solve(tall, tall_plan, d):
    (P, Q), gotP, gotQ = full_half_sweeps(tall, d)
    print("tall nFactors %d worst / bar: users %.3f items %.3f" % (
        d, assert_als_close(gotP, gram_half_fp64(P, Q, tall.uptr, tall.uidx, tall.iptr), "tall nFactors %d users" % d),
        assert_als_close(gotQ, gram_half_fp64(Q, P, tall.iptr, tall.iidx, tall.uptr), "tall nFactors %d items" % d)))


@gpu
@pytest.mark.parametrize("d", [130, 256])
def test_rows_solved_on_a_later_trip_equal_the_rows_of_a_one_grid_range(tall, tall_plan, d):
    """Within a half-sweep a row's result depends on B and S alone, not on which trip of which workgroup solved it: a handle restricted
    to a piece that fits one grid (its Gram still covers every row) gives the full run's bits inside the piece and leaves the rest."""
    start, fullP, fullQ = full_half_sweeps(tall, d)
    for k, upiece in enumerate(USER_PIECES):
        ipiece = ITEM_PIECES[k] if k < len(ITEM_PIECES) else (0, 0)
        _, partP, partQ = half_sweeps(tall, d, ranges=upiece + ipiece)
        for (lo, hi), part, full, begin in ((upiece, partP, fullP, start[0]), (ipiece, partQ, fullQ, start[1])):
            if part is None:
                continue
            inside = np.zeros(full.shape[0], bool)
            inside[lo:hi] = True
            assert np.array_equal(bits(part[inside]), bits(full[inside])), (d, lo, hi)
            assert np.array_equal(bits(part[~inside]), bits(begin[~inside])), (d, lo, hi)
    moved = (bits(fullP) != bits(start[0])).any(axis=1)
    assert moved.all() and (bits(fullQ) != bits(start[1])).any(axis=1).all()  # (an empty user's row moves too: M = w S, sums of zero)


@gpu
def test_two_handles_one_tall_epoch_same_bits(tall, tall_plan):
    runs = []
    for _ in range(2):
        mf, _, _ = make_mf(tall, 256, std=0.1)
        mf.set_als_form(1)
        mf.als_epoch(W, REG)
        assert mf.als_form() == (1, capi.ALS_FAMILY_DEEP)
        runs.append(mf.get_factors())
        mf.close()
    assert np.isfinite(runs[0][0]).all() and np.isfinite(runs[0][1]).all()
    assert np.array_equal(bits(runs[0][0]), bits(runs[1][0])) and np.array_equal(bits(runs[0][1]), bits(runs[1][1]))


@gpu
def test_the_gram_skips_the_empty_users(tall, tall_plan):
    """S of the item half-sweep is over the users WITH feedback (fb_rows, not the identity here), and the seven empty users start
    from non-zero factors like everybody else.  Seven rows among 8200 are enough: the float64 half-sweep with S over every user is
    20 times the bar away from the one with S over fb_rows (held here, at once), and so would be a kernel that summed them."""
    d = 161
    (P, Q), _, got = half_sweeps(tall, d, ranges=(0, 0, 0, N_ITEMS))
    assert P[list(EMPTY_USERS)].any(axis=1).all()
    ref = gram_half_fp64(Q, P, tall.iptr, tall.iidx, tall.uptr)
    with pytest.raises(AssertionError):
        assert_als_close(gram_half_fp64(Q, P, tall.iptr, tall.iidx, np.arange(N_USERS + 1)), ref)
    print("tall nFactors %d S over fb_rows, items worst / bar %.3f" % (d, assert_als_close(got, ref, "S over fb_rows")))
