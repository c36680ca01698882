"""The per-bin finish of the binned BPR chunk preparation (csrc/bpr_prepare.hip: bpr_bin_finish_kernel).

One workgroup per bin of user ids sorts the bin's samples by user, draws their items and groups equal positives, all in LDS; it
replaces bpr_bin_sort_kernel, bpr_sample_items_kernel and bpr_group_positives_kernel, which variant bit 19 brings back.  Every case
goes through gorse_hip_test_bpr_prepare_chunk and compares the runs, as multisets per user, with gorse_bpr_sample_triplets; where
the three kernels fix the order inside a run (3 .. 1024 samples) the two paths must leave the same bits.  The sizes aim at the
kernel's own edges, which gorse_hip_test_bpr_finish_capacities reports: a bin over the sample capacity, a range of rows at and one
over what is staged in LDS, runs around the "fewer than three" rule, chunks around the tile of the count / scatter kernels."""
import ctypes as C

import numpy as np
import pytest

from gorse_amd import capi

pytestmark = pytest.mark.gpu

VARIANT_THREE_KERNELS, VARIANT_ARRIVAL_ORDER = 1 << 19, 1 << 20
GROUP_CAP = 1024  # csrc/bpr_prepare.hip kGroupCap: the longest run whose order is fixed
TILE = 4096       # csrc/bpr_bins.hpp prep_bins: samples per workgroup of the count / scatter kernels (chunks under 2M samples)
SEED, EPOCH, BASE = (1 << 32) + 12345, 3, 1 << 40


def _capacities():
    s, r = C.c_int32(0), C.c_int32(0)
    capi.lib().gorse_hip_test_bpr_finish_capacities(C.byref(s), C.byref(r))
    assert s.value >= GROUP_CAP and r.value > 0
    return s.value, r.value


def _csr(U, rows):
    """rows: {user: array of distinct items}; every other user is without feedback"""
    lens = np.zeros(U, np.int64)
    for u, r in rows.items():
        lens[u] = len(r)
    uptr = np.zeros(U + 1, np.int64)
    np.cumsum(lens, out=uptr[1:])
    uidx = np.concatenate([np.asarray(rows[u], np.int32) for u in sorted(rows)]).astype(np.int32)
    return uptr, uidx


def _sorted_triples(u, i, j):
    t = np.stack([u, i, j], axis=1)
    return t[np.lexsort((t[:, 2], t[:, 1], t[:, 0]))]


def _prepare(mf, n, variant, sampled, seed=SEED, epoch=EPOCH, base=BASE):
    """one chunk prepared under `variant`; the handle's device counter of samples given up on must rise by exactly the number of
    samples the per-sample sampler gave up on (`sampled`): once per sample without a user or without a negative"""
    L = capi.lib()
    L.gorse_hip_test_set_variant(variant)
    try:
        before = mf.bpr_fail_count()
        out = mf.bpr_prepare_chunk(n, seed, epoch, base)
        assert mf.bpr_fail_count() - before == int((sampled[0] < 0).sum()), variant
        return out
    finally:
        L.gorse_hip_test_set_variant(0)


def _check(U, I, n, prepared, sampled, grouped=True):
    """the prepared chunk holds exactly the sampled triplets, each in its user's run; a sample without a negative is a (-1, -1) in its
    run, once; with `grouped`: every positive of a run of at most GROUP_CAP samples in one stretch, the (-1, -1) last"""
    off, si, sj = prepared
    gu, gi, gj = sampled
    assert off[0] == 0 and off[U + 1] == n and (np.diff(off) >= 0).all()
    m = int(off[U])
    lens = np.diff(off)[:U]
    su = np.repeat(np.arange(U, dtype=np.int32), lens)
    si, sj = si[:m], sj[:m]
    ok = sj >= 0
    failed = gu < 0
    assert (si[~ok] == -1).all() and (sj[~ok] == -1).all()
    assert np.array_equal(_sorted_triples(su[ok], si[ok], sj[ok]), _sorted_triples(gu[~failed], gi[~failed], gj[~failed]))
    # every sample the sampler gave up on is either without a user (behind off[U]) or ONE (-1, -1) in its run
    assert int(failed.sum()) == int((~ok).sum()) + (n - m)
    first = ok.copy()
    first[1:] &= ~ok[:-1] | (su[1:] != su[:-1]) | (si[1:] != si[:-1])
    series = np.bincount(su[first], minlength=U)
    pairs = np.unique(su[ok].astype(np.int64) * I + si[ok])
    distinct = np.bincount(pairs // I, minlength=U)
    assert (series >= distinct).all()
    if grouped:
        within = lens <= GROUP_CAP
        assert np.array_equal(series[within], distinct[within]), "a positive of a run within the capacity lies in two stretches"
        # a failed sample is followed by failed samples to the end of its run
        nxt_same_run = su[1:] == su[:-1]
        assert not (within[su[:-1]] & nxt_same_run & ~ok[:-1] & ok[1:]).any()
    return lens


def _same_bits(U, a, b):
    """two preparations of one chunk: the same offsets; the same (i, j) at every position of a run of 3 .. GROUP_CAP samples; the
    same multiset in every other run"""
    (off, si, sj), (off2, si2, sj2) = a, b
    assert np.array_equal(off, off2)
    m = int(off[U])
    lens = np.diff(off)[:U]
    fixed = np.repeat((lens >= 3) & (lens <= GROUP_CAP), lens)
    assert np.array_equal(si[:m][fixed], si2[:m][fixed]) and np.array_equal(sj[:m][fixed], sj2[:m][fixed])
    su = np.repeat(np.arange(U, dtype=np.int32), lens)
    assert np.array_equal(_sorted_triples(su[~fixed], si[:m][~fixed], sj[:m][~fixed]),
                          _sorted_triples(su[~fixed], si2[:m][~fixed], sj2[:m][~fixed]))
    return lens, int(fixed.sum())


# ---- a handle of 4,200 users with a few dozen items each: bins of 16 ids, several bins per CU -------------------------------------
AU, AI = 4200, 3000


@pytest.fixture(scope="module")
def handle_a():
    rng = np.random.default_rng(5)
    lens = rng.integers(24, 49, AU)
    rows = {u: rng.choice(AI, lens[u], replace=False) for u in range(AU)}
    uptr, uidx = _csr(AU, rows)
    mf = capi.MF(AU, AI, 64, uptr, uidx)
    assert mf.bpr_user_runs()
    yield mf
    mf.close()


def test_same_bits_as_the_three_kernel_finish(handle_a):
    n = 40 * AU
    sampled = handle_a.bpr_sample_triplets(n, SEED, EPOCH, BASE)
    new = _prepare(handle_a, n, 0, sampled)
    old = _prepare(handle_a, n, VARIANT_THREE_KERNELS, sampled)
    _check(AU, AI, n, new, sampled)
    _check(AU, AI, n, old, sampled)
    lens, fixed = _same_bits(AU, new, old)
    print("runs %d .. %d samples, %d of %d positions in runs whose order is fixed" % (lens.min(), lens.max(), fixed, n))
    assert fixed > 0.99 * n


@pytest.mark.parametrize("n", [1, TILE + 1, 3 * TILE - 1])
def test_chunk_edges(handle_a, n):
    sampled = handle_a.bpr_sample_triplets(n, SEED, EPOCH, BASE)
    new = _prepare(handle_a, n, 0, sampled)
    _check(AU, AI, n, new, sampled)
    _same_bits(AU, new, _prepare(handle_a, n, VARIANT_THREE_KERNELS, sampled))


def test_arrival_order_variant_on_the_new_path(handle_a):
    n = 40 * AU
    sampled = handle_a.bpr_sample_triplets(n, SEED, EPOCH, BASE)
    plain = _prepare(handle_a, n, VARIANT_ARRIVAL_ORDER, sampled)
    _check(AU, AI, n, plain, sampled, grouped=False)
    assert np.array_equal(plain[0], _prepare(handle_a, n, 0, sampled)[0])


def test_run_lengths_around_three():
    U, I = 4100, 500
    rng = np.random.default_rng(9)
    rows = {u: rng.choice(I, 3, replace=False) for u in range(U)}
    uptr, uidx = _csr(U, rows)
    mf = capi.MF(U, I, 16, uptr, uidx)
    try:
        assert mf.bpr_user_runs()
        n = 3 * U
        sampled = mf.bpr_sample_triplets(n, SEED, EPOCH, BASE)
        new = _prepare(mf, n, 0, sampled)
        lens = _check(U, I, n, new, sampled)
        for want in (0, 1, 2, 3, 4):
            assert (lens == want).any(), want
        _same_bits(U, new, _prepare(mf, n, VARIANT_THREE_KERNELS, sampled))
    finally:
        mf.close()


@pytest.mark.parametrize("users, per_cap", [(8, 3.0), (16, 1.25)])
def test_one_bin_over_the_sample_capacity(users, per_cap):
    """5,000 users in bins of 16 ids, feedback only with the first `users`: bin 0 receives every sample of the chunk, more than the
    LDS pass holds, and is finished by its workgroup in slices.  Eight users, 3 x capacity samples: runs longer than GROUP_CAP, whose
    order is free; sixteen users, 1.25 x capacity: runs within GROUP_CAP, grouped all the same."""
    cap, _ = _capacities()
    U, I = 5000, 400
    rng = np.random.default_rng(13)
    rows = {u: rng.choice(I, 30, replace=False) for u in range(users)}
    uptr, uidx = _csr(U, rows)
    mf = capi.MF(U, I, 64, uptr, uidx)
    try:
        assert mf.bpr_user_runs()
        n = int(per_cap * cap)
        sampled = mf.bpr_sample_triplets(n, SEED, EPOCH, BASE)
        new = _prepare(mf, n, 0, sampled)
        lens = _check(U, I, n, new, sampled)
        # (a sample whose every user draw met a user without feedback has no run: a few dozen of them, behind off[U])
        assert int(lens[:16].sum()) == int(new[0][U]) > cap and n - int(new[0][U]) < n // 100
        assert (lens[:users] > GROUP_CAP).all() if users == 8 else (lens[:users] <= GROUP_CAP).all()
        _same_bits(U, new, _prepare(mf, n, VARIANT_THREE_KERNELS, sampled))
    finally:
        mf.close()


def test_staging_edge_and_a_user_holding_every_item():
    """Bins of 16 ids.  Bin 0: user 0 holds every item, a row one entry longer than what is staged (read from global memory; no
    negative exists: every sample (-1, -1)).  Bin 1: user 16 holds every item but one, a row of exactly the staged capacity (about
    half its samples find the one negative within the draw limit; the others end up last in the run).  Bins 2, 3: rows at and one
    over half the capacity, the edge of staging uidx next to uidx_sorted.  Bin 4: sixteen short rows staged together."""
    _, stage = _capacities()
    U, I = 5000, stage + 1
    rng = np.random.default_rng(17)
    rows = {0: rng.permutation(I), 16: rng.permutation(I)[:stage], 32: rng.choice(I, stage // 2, replace=False),
            48: rng.choice(I, stage // 2 + 1, replace=False)}
    for u in range(64, 80):
        rows[u] = rng.choice(I, 40, replace=False)
    uptr, uidx = _csr(U, rows)
    mf = capi.MF(U, I, 16, uptr, uidx)
    try:
        assert mf.bpr_user_runs()
        n = 60 * len(rows)
        sampled = mf.bpr_sample_triplets(n, SEED, EPOCH, BASE)
        new = _prepare(mf, n, 0, sampled)
        lens = _check(U, I, n, new, sampled)
        off, si, sj = new
        assert lens[0] > 0 and (sj[off[0]:off[1]] == -1).all()
        run16 = sj[off[16]:off[17]]
        assert 0 < (run16 < 0).sum() < run16.size  # both kinds of sample in the run of the staged long row
        _same_bits(U, new, _prepare(mf, n, VARIANT_THREE_KERNELS, sampled))
    finally:
        mf.close()
