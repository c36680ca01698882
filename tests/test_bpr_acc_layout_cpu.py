"""The accumulated tier of a BPR handle (gorse_amd/csrc/hot_rows.hpp acc_rows_eligible / acc_rows_layout, the header gorse_mf_create
includes, reached through the host library's hook gh_test_bpr_acc_layout): on an eligible handle -- at least 4096 users, nFactors in
{8, 16, 32, 64, 128}, no cold item, items x nFactors x 4 bytes <= 4 MiB -- every WARM item has exactly one accumulator row, the rows lie
contiguously behind the hot tier's replica rows in item order, and the hot tier is what gh_test_bpr_hot_layout gives without the tier.
At each edge of the rule the tier is empty and every class is what it is without it."""
import ctypes as C

import numpy as np
import pytest

from gorse_amd import cf, synth

ACC_BYTES = 4 << 20  # csrc/hot_rows.hpp kAccTableBytes
NO_COLD = 32768      # csrc/mf.hip kDefaultColdWindow


@pytest.fixture(scope="module")
def c2():
    return synth.synth_cf(6040, 3706, 994169, seed=42, min_len=19, n_neg=99, with_test=False)


def _lib():
    L = C.CDLL(cf.HOST_LIB)
    L.gh_test_bpr_hot_layout.restype = C.c_int32
    L.gh_test_bpr_hot_layout.argtypes = [C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_double, C.c_int32, C.c_void_p, C.c_void_p,
                                         C.c_void_p]
    L.gh_test_bpr_acc_layout.restype = C.c_int32
    L.gh_test_bpr_acc_layout.argtypes = [C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_double, C.c_int32, C.c_int64,
                                         C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def hot_layout(U, I, uptr, uidx, unit, max_r=8):
    items, meta, rows = np.zeros(1024, np.int32), np.zeros(1024, np.int32), np.zeros(1, np.int64)
    n = _lib().gh_test_bpr_hot_layout(U, I, uptr.ctypes.data, uidx.ctypes.data, unit, max_r, items.ctypes.data, meta.ctypes.data,
                                      rows.ctypes.data)
    return items[:n].copy(), meta[:n].copy(), int(rows[0])


def acc_layout(U, I, d, uptr, uidx, unit=0.001, max_r=8, window=NO_COLD):
    slot, acc_items, out3 = np.zeros(I, np.int32), np.zeros(I, np.int32), np.zeros(3, np.int64)
    n = _lib().gh_test_bpr_acc_layout(U, I, d, uptr.ctypes.data, uidx.ctypes.data, unit, max_r, window, slot.ctypes.data,
                                      acc_items.ctypes.data, out3.ctypes.data)
    return slot, acc_items[:n].copy(), int(out3[0]), int(out3[1]), int(out3[2])


def _csr(data):
    return np.ascontiguousarray(data.uptr, np.int64), np.ascontiguousarray(data.uidx, np.int32)


def _uniform(U, I, per, seed=1):
    rng = np.random.default_rng(seed)
    uidx = np.concatenate([np.sort(rng.choice(I, per, replace=False)) for _ in range(U)]).astype(np.int32)
    return np.arange(U + 1, dtype=np.int64) * per, uidx


def _check_no_tier(slot, acc_items, hot_items, hot_meta):
    assert acc_items.size == 0
    is_hot = np.zeros(slot.size, bool)
    is_hot[hot_items] = True
    assert np.array_equal(slot[hot_items], hot_meta)
    assert (slot[~is_hot] < 0).all()  # warm (-1) or cold (-2): nothing but the hot items has a row


@pytest.mark.parametrize("unit", [0.0005, 0.001, 0.002, 0.004])
@pytest.mark.parametrize("d", [8, 16, 32, 64, 128])
def test_tier_holds_exactly_the_warm_items_of_s_ml1m(c2, unit, d):
    uptr, uidx = _csr(c2)
    hot_items, hot_meta, hot_rows = hot_layout(c2.U, c2.I, uptr, uidx, unit)
    slot, acc_items, rows, n_hot, n_cold = acc_layout(c2.U, c2.I, d, uptr, uidx, unit)
    # the hot tier: bit for bit what the hook without the tier returns
    assert n_hot == hot_items.size == 926 and rows == hot_rows and n_cold == 0
    assert np.array_equal(slot[hot_items], hot_meta)
    # the tier: every other item, ids ascending, one row each (log2 R = 0), contiguous behind the replica rows
    warm = np.setdiff1d(np.arange(c2.I), hot_items)
    assert np.array_equal(acc_items, warm) and acc_items.size == 2780
    assert (slot[warm] & 15 == 0).all()
    assert np.array_equal(slot[warm] >> 4, hot_rows + np.arange(warm.size))
    assert (slot >= 0).all()


def test_tier_is_empty_at_each_edge_of_the_rule():
    I, per = 512, 8
    # the reference point: 4096 users, nFactors 64 -- eligible
    uptr, uidx = _uniform(4096, I, per)
    hot_items, hot_meta, hot_rows = hot_layout(4096, I, uptr, uidx, 0.001)
    slot, acc_items, rows, n_hot, n_cold = acc_layout(4096, I, 64, uptr, uidx)
    assert n_cold == 0 and rows == hot_rows and acc_items.size == I - n_hot and acc_items.size > 0
    assert np.array_equal(slot[hot_items], hot_meta)
    assert np.array_equal(slot[acc_items] >> 4, hot_rows + np.arange(acc_items.size)) and (slot[acc_items] & 15 == 0).all()
    # a width outside the set
    for d in (4, 24, 48, 65, 256):
        s, a, _, _, _ = acc_layout(4096, I, d, uptr, uidx)
        _check_no_tier(s, a, hot_items, hot_meta)
    # 4,095 users
    uptr2, uidx2 = uptr[:4096].copy(), uidx[:4095 * per].copy()
    h_items, h_meta, _ = hot_layout(4095, I, uptr2, uidx2, 0.001)
    s, a, _, _, _ = acc_layout(4095, I, 64, uptr2, uidx2)
    _check_no_tier(s, a, h_items, h_meta)
    # one cold item: a catalogue whose last item nobody holds, and a window between what makes that item cold ((0 + 1 / I) x window
    # < 1) and what makes the least held of the others cold ((cnt / nnz + 1 / I) x window < 1)
    I3 = 1024
    uptr3, uidx3 = _uniform(4096, I3 - 1, per, seed=2)  # item 1023 has no feedback
    cnt = np.bincount(uidx3, minlength=I3)
    nnz = int(uptr3[-1])
    window = int(1.0 / (1.0 / I3 + 0.5 * cnt[cnt > 0].min() / nnz))
    expect_cold = np.flatnonzero((cnt / nnz + 1.0 / I3) * window < 1.0)
    assert np.array_equal(expect_cold, [I3 - 1])
    h_items, h_meta, _ = hot_layout(4096, I3, uptr3, uidx3, 0.001)
    s, a, _, _, n_cold = acc_layout(4096, I3, 64, uptr3, uidx3, window=window)
    assert n_cold == 1 and s[I3 - 1] == -2
    _check_no_tier(s, a, h_items, h_meta)
    s, a, _, nh, n_cold = acc_layout(4096, I3, 64, uptr3, uidx3, window=0)  # the same handle without the cold item: eligible
    assert n_cold == 0 and a.size == I3 - nh
    # items x nFactors x 4 one row over the bound: 16,384 items of 64 floats are exactly 4 MiB
    for d in (64, 128):
        Ib = ACC_BYTES // (4 * d)
        rng = np.random.default_rng(5)
        for Ix, want in ((Ib, True), (Ib + 1, False)):
            uidx4 = np.sort(rng.integers(0, Ix, (4096, 4)), axis=1)
            uidx4[:, 1:] += (np.diff(uidx4, axis=1) == 0)  # (rows need not be duplicate-free for the rule; keep ids in range)
            uidx4 = np.minimum(uidx4, Ix - 1).astype(np.int32).ravel()
            uptr4 = np.arange(4097, dtype=np.int64) * 4
            s, a, _, nh, n_cold = acc_layout(4096, Ix, d, uptr4, uidx4, window=0)
            assert n_cold == 0
            assert (a.size == Ix - nh) if want else (a.size == 0), (d, Ix)
            assert ((s >= 0).all()) == want
