"""gorse_mf_rank and gorse_mf_evaluate take their (users, candidate CSR) through one validation and upload (csrc/mf_rank.hip
upload_user_lists): both reject the same malformed lists with the same code, and a rejected call leaves nothing behind -- the next
correct call on the same handle ranks as the oracle's Rank does."""
import ctypes as C

import numpy as np
import pytest

from gorse_amd import capi, synth

pytestmark = pytest.mark.gpu

U, I, D, TOPK = 8, 16, 16, 3


def good_lists():
    """three users with 4, 0 and 5 candidates; every user has one target"""
    users = np.array([2, 7, 0], np.int32)
    cptr = np.array([0, 4, 4, 9], np.int64)
    cand = np.array([3, 15, 0, 8, 1, 2, 14, 9, 5], np.int32)
    tptr = np.array([0, 1, 2, 3], np.int64)
    tgt = np.array([15, 4, 9], np.int32)
    return dict(users=users, cptr=cptr, cand=cand, tptr=tptr, tgt=tgt)


def edit(key, index, value):
    def change(lists):
        lists[key] = lists[key].copy()
        lists[key][index] = value
    return change


def no_candidates(lists):
    lists["cand"] = None


# (what is wrong, the change to the good lists, the code, whether gorse_mf_rank sees the field at all)
MALFORMED = [
    ("cand_indptr[0] != 0", edit("cptr", 0, 1), capi.ERR_INVALID, True),
    ("cand_indptr not monotone", edit("cptr", 1, 6), capi.ERR_INVALID, True),  # 0 6 4 9
    ("user = U", edit("users", 1, U), capi.ERR_RANGE, True),
    ("candidate = I", edit("cand", 8, I), capi.ERR_RANGE, True),
    ("candidate = -1", edit("cand", 0, -1), capi.ERR_RANGE, True),
    ("cand NULL with entries", no_candidates, capi.ERR_INVALID, True),
    ("target_indptr not monotone", edit("tptr", 1, 3), capi.ERR_INVALID, False),  # 0 3 2 3
]


@pytest.fixture(scope="module")
def model(oracle):
    P, Q = synth.init_factors(U, I, D, 0.0, 0.5, 11)
    mf = capi.MF(U, I, D, np.arange(U + 1, dtype=np.int64), (np.arange(U) % I).astype(np.int32))
    mf.set_factors(P, Q)
    g = good_lists()
    rank, rlen = oracle.mf_rank(P, Q, g["users"], g["cptr"], g["cand"], TOPK)
    assert rlen.tolist() == [3, 0, 3]
    yield mf, rank, rlen
    mf.close()


def call_rank(mf, lists):
    rank, rlen = np.full((3, TOPK), -2, np.int32), np.full(3, -2, np.int32)
    rc = capi.lib().gorse_mf_rank(mf.h, 3, capi._p(lists["users"], capi._i32p), capi._p(lists["cptr"], capi._i64p),
                                  capi._p(lists["cand"], capi._i32p), TOPK, capi._p(rank, capi._i32p), capi._p(rlen, capi._i32p))
    return rc, rank, rlen


def call_evaluate(mf, lists):
    sums, count = np.full(6, np.nan, np.float32), C.c_float(-1)
    rc = capi.lib().gorse_mf_evaluate(mf.h, 3, capi._p(lists["users"], capi._i32p), capi._p(lists["tptr"], capi._i64p),
                                      capi._p(lists["tgt"], capi._i32p), capi._p(lists["cptr"], capi._i64p),
                                      capi._p(lists["cand"], capi._i32p), TOPK, capi._p(sums, capi._f32p), C.byref(count), None)
    return rc, sums, count.value


@pytest.mark.parametrize("what,change,code,rank_sees_it", MALFORMED, ids=[m[0] for m in MALFORMED])
def test_rank_and_evaluate_reject_the_same_lists_with_the_same_code(model, what, change, code, rank_sees_it):
    mf, exp_rank, exp_rlen = model
    good = good_lists()
    rc, ok_sums, ok_count = call_evaluate(mf, good)
    assert rc == capi.OK
    bad = good_lists()
    change(bad)
    entries = [call_evaluate] + ([call_rank] if rank_sees_it else [])
    codes = []
    for entry in entries:
        out = entry(mf, bad)
        codes.append(out[0])
        assert capi.lib().gorse_hip_last_error() != b""
        # nothing half-uploaded: the correct lists rank and evaluate as before on the same handle
        rc, rank, rlen = call_rank(mf, good)
        assert rc == capi.OK
        assert np.array_equal(rlen, exp_rlen) and np.array_equal(rank, exp_rank), (what, entry.__name__)
        rc, sums, count = call_evaluate(mf, good)
        assert rc == capi.OK and count == ok_count == 3.0
        assert np.array_equal(np.isnan(sums), np.isnan(ok_sums))
        assert np.array_equal(sums.view(np.uint32)[~np.isnan(sums)], ok_sums.view(np.uint32)[~np.isnan(ok_sums)])
    assert codes == [code] * len(entries), (what, codes)
