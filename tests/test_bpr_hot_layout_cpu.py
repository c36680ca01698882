"""The replica rows of the BPR schedules' hot items (gorse_amd/csrc/hot_rows.hpp, the header gorse_mf_create includes, reached through
the host library's hook): on the C2 shape (S-ml1m as bench.py draws it), the hot set is the rule's -- share of the feedback >= 1/8192,
>= 64 feedbacks, at most 1024 items and a quarter of the catalogue --, every slot has a power-of-two replica count R in 1 .. 8 that the
rule restated here gives (R = the smallest power of two >= the item's expected updates per sample / unit), and the rows are laid out
slot after slot with no overlap and no gap.  Reference semantics of the rates: model/cf/model.go:452-468 (user uniform among the users
with feedback, positive uniform in the user's row, negative uniform in the catalogue)."""
import ctypes as C

import numpy as np
import pytest

from gorse_amd import cf, synth


@pytest.fixture(scope="module")
def c2():
    return synth.synth_cf(6040, 3706, 994169, seed=42, min_len=19, n_neg=99, with_test=False)


def layout(data, unit, max_r=8):
    L = C.CDLL(cf.HOST_LIB)
    L.gh_test_bpr_hot_layout.restype = C.c_int32
    L.gh_test_bpr_hot_layout.argtypes = [C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_double, C.c_int32, C.c_void_p, C.c_void_p,
                                         C.c_void_p]
    uptr = np.ascontiguousarray(data.uptr, np.int64)
    uidx = np.ascontiguousarray(data.uidx, np.int32)
    items, meta, rows = np.zeros(1024, np.int32), np.zeros(1024, np.int32), np.zeros(1, np.int64)
    n = L.gh_test_bpr_hot_layout(data.U, data.I, uptr.ctypes.data, uidx.ctypes.data, unit, max_r, items.ctypes.data, meta.ctypes.data,
                                 rows.ctypes.data)
    return items[:n], (meta[:n] >> 4).astype(np.int64), (1 << (meta[:n] & 15)).astype(np.int64), int(rows[0])


def restated(data, unit, max_r=8):
    """the rule in numpy: hot set, then R per slot from the fixed-point positive share (2^-32 units per user) + 1 / I for negatives"""
    uptr, uidx = np.asarray(data.uptr, np.int64), np.asarray(data.uidx, np.int64)
    nnz, I = int(uptr[-1]), data.I
    cnt = np.bincount(uidx, minlength=I)
    thr = max(64, -(-nnz // 8192))
    cap = min(1024, max(1, I // 4))
    hot = np.flatnonzero(cnt >= thr)
    if hot.size > cap:
        hot = np.sort(sorted(hot, key=lambda i: (-cnt[i], i))[:cap])
    lens = np.diff(uptr)
    w = np.zeros(data.U, np.uint64)
    w[lens > 0] = (np.uint64(1) << np.uint64(32)) // lens[lens > 0].astype(np.uint64)
    per_entry = np.repeat(w, lens)
    acc = np.zeros(I, np.uint64)
    np.add.at(acc, uidx, per_entry)
    users = int((lens > 0).sum())
    share = acc[hot].astype(np.float64) / 4294967296.0 / users + (1.0 / I if hot.size * 64 >= I else 0.0)
    R = np.ones(hot.size, np.int64)
    while True:
        grow = (R < max_r) & (R * unit < share)
        if not grow.any():
            return hot, R
        R[grow] *= 2


@pytest.mark.parametrize("unit", [0.0005, 0.001, 0.002, 0.004])
def test_replica_counts_and_layout_on_s_ml1m(c2, unit):
    items, base, R, rows = layout(c2, unit)
    hot, R_expect = restated(c2, unit)
    assert np.array_equal(items, hot) and items.size == 926  # the C2 hot set: the cap of a quarter of the catalogue
    assert np.array_equal(R, R_expect)
    assert ((R >= 1) & (R <= 8)).all() and (R & (R - 1) == 0).all()
    assert base[0] == 0 and np.array_equal(base[1:], np.cumsum(R)[:-1]) and rows == R.sum()  # slot after slot: no overlap, no gap
    print("unit %g: rows %d of %d (eight per slot), R histogram %s" % (unit, rows, 8 * items.size,
                                                                       dict(zip(*np.unique(R, return_counts=True)))))


def test_replica_count_caps():
    """the counts stay in [1, max_r] at the extremes: a unit so small that every slot wants more than the cap, and one so large that
    none wants a second row"""
    data = synth.synth_cf(6040, 3706, 994169, seed=42, min_len=19, n_neg=99, with_test=False)
    for unit, expect in ((1e-9, 8), (1.0, 1)):
        items, base, R, rows = layout(data, unit)
        assert (R == expect).all() and rows == expect * items.size
        assert np.array_equal(base, np.arange(items.size) * expect)
