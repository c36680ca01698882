"""The Deep ALS form (csrc/als_deep.hip; gorse_mf_set_als_form(h, 1)): nFactors 129..256 as a Gram solve on the matrix cores.

Every value is held to a float64 restatement of that solve, written here in numpy -- M = (1 - w) G + w S per row and one coordinate
sweep over it -- with the project's ALS bar (cf_cases.assert_als_close; DESIGN.md section 4 "ALS").  Form 0 at these widths (the
residual recurrence) is a second witness against the same reference.  The dataset has, on both sides, an empty row, a one-entry
row, rows of 31 / 32 / 33 entries (one short of, equal to and one past the kernel's gather batch) and a row of 150; with the row plan
(64, 64) that row is a long one of three chunks, so the chunk kernel, the partials' reduce and the long solve all run.  The widths are
both edges of every block count ceil(nFactors / 32) = 5 .. 8, each a kernel instance of its own.  What 200 rows cannot reach -- a
second trip of a grid-stride loop, a Gram of several chunks, a row of eight partials or more -- is
tests/test_gpu_als_deep_past_one_grid.py's."""
import numpy as np
import pytest

from cf_cases import assert_als_close, bits, make_mf
from gorse_amd import capi, synth

pytestmark = pytest.mark.gpu

W, REG = 0.05, 0.015
N, SPECIAL = 200, (0, 1, 31, 32, 33, 150)  # rows per side; the lengths of rows 0..5 of both sides


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(7)
    R = np.zeros((N, N), bool)
    R[8:, 8:] = rng.random((N - 8, N - 8)) < 0.05
    for k, n in enumerate(SPECIAL):
        R[k, 8 + rng.permutation(N - 8)[:n]] = True
        R[8 + rng.permutation(N - 8)[:n], k] = True
    u, i = np.nonzero(R)
    uptr, uidx = synth._csr_from_pairs(u, i, N)
    iptr, iidx = synth._csr_from_pairs(i, u, N)
    assert tuple(np.diff(uptr)[:6]) == SPECIAL and tuple(np.diff(iptr)[:6]) == SPECIAL
    z, e = np.zeros(N + 1, np.int64), np.zeros(0, np.int32)
    return synth.CFData(N, N, uptr, uidx, iptr, iidx, z, e, z.copy(), e.copy())


@pytest.fixture
def long_rows():
    """rows of more than 64 entries are long ones, cut into chunks of 64 (handles created inside the test)"""
    capi.lib().gorse_hip_test_set_als_plan(64, 64)
    yield
    capi.lib().gorse_hip_test_set_als_plan(0, 0)


def gram_half_fp64(A, B, ptr, idx, bptr, w=W):
    A, B = np.asarray(A, np.float64).copy(), np.asarray(B, np.float64)
    has = np.diff(bptr) > 0
    S = B[has].T @ B[has]
    for u in range(A.shape[0]):
        Bu = B[idx[ptr[u]:ptr[u + 1]]]
        M, s, p = (1 - w) * (Bu.T @ Bu) + w * S, Bu.sum(axis=0), A[u]
        for f in range(p.size):
            p[f] = (s[f] - (M[f] @ p - M[f, f] * p[f])) / (M[f, f] + REG)
    return A


def half(data, d, side, form, ranges=None, w=W):
    """factors of `side` after one half-sweep from the seeded start, on a fresh handle (form None: the setter is never called)"""
    mf, P, Q = make_mf(data, d, std=0.1)
    if form is not None:
        mf.set_als_form(form)
    if ranges:
        mf.als_set_ranges(*ranges)
    mf.als_half_epoch(side, w, REG)
    got, used = mf.get_factors()[side], mf.als_form()[1]
    mf.close()
    return (P, Q), got, used


def both_forms_meet_the_float64_gram_solve(data, d, w):
    for side in (0, 1):
        ptr, idx, bptr = (data.uptr, data.uidx, data.iptr) if side == 0 else (data.iptr, data.iidx, data.uptr)
        start, deep, used = half(data, d, side, 1, w=w)
        assert used == capi.ALS_FAMILY_DEEP
        _, plain, used0 = half(data, d, side, 0, w=w)
        assert used0 == capi.ALS_FAMILY_RESIDUAL
        ref = gram_half_fp64(start[side], start[1 - side], ptr, idx, bptr, w)
        label = "nFactors %d w %g side %d" % (d, w, side)
        print(label, "worst / bar: deep %.3f residual %.3f deep against residual %.3f" % (
            assert_als_close(deep, ref, label + " deep"), assert_als_close(plain, ref, label + " residual"),
            assert_als_close(deep, plain, label + " deep against residual")))


# both edges of every block count NB = ceil(d / 32): 5 for 129..160, 6 to 192, 7 to 224, 8 to 256 (a kernel instance each)
@pytest.mark.parametrize("d", [129, 160, 161, 192, 193, 224, 225, 255, 256])
def test_half_sweeps_meet_the_float64_gram_solve(data, long_rows, d):
    both_forms_meet_the_float64_gram_solve(data, d, W)


@pytest.mark.parametrize("d", [192, 224])
@pytest.mark.parametrize("w", [0.0, 1.0])
def test_half_sweeps_meet_the_float64_gram_solve_where_one_term_vanishes(data, long_rows, d, w):
    """M = (1 - w) G + w S at w = 0 and w = 1: swapped or misapplied factors show plainly.  At w = 0 the empty row's M is all zeros
    and its reference row exactly zero, so the bar there is zero and both forms must write exact zeros.  A float32 restatement of the
    Gram form on this data reaches 0.04 of the bar at w = 0 and 0.02 at w = 1 with the module's reg: the input stays well-conditioned."""
    both_forms_meet_the_float64_gram_solve(data, d, w)


@pytest.mark.parametrize("d", [160, 192, 224, 256])
def test_epoch_meets_the_float64_epoch(data, long_rows, d):
    """users first, then the items from the user factors just written"""
    mf, P, Q = make_mf(data, d, std=0.1)
    mf.set_als_form(1)
    mf.als_epoch(W, REG)
    assert mf.als_form() == (1, capi.ALS_FAMILY_DEEP)
    gotP, gotQ = mf.get_factors()
    mf.close()
    refP = gram_half_fp64(P, Q, data.uptr, data.uidx, data.iptr)
    refQ = gram_half_fp64(Q, refP, data.iptr, data.iidx, data.uptr)
    print("nFactors %d epoch worst / bar: users %.3f items %.3f" % (
        d, assert_als_close(gotP, refP, "nFactors %d epoch users" % d), assert_als_close(gotQ, refQ, "nFactors %d epoch items" % d)))


def test_two_handles_three_epochs_same_bits(data, long_rows):
    runs = []
    for _ in range(2):
        mf, _, _ = make_mf(data, 192, std=0.1)
        mf.set_als_form(1)
        for _ in range(3):
            mf.als_epoch(W, REG)
        assert mf.als_form() == (1, capi.ALS_FAMILY_DEEP)
        runs.append(mf.get_factors())
        mf.close()
    assert np.isfinite(runs[0][0]).all() and np.isfinite(runs[0][1]).all()
    assert np.array_equal(bits(runs[0][0]), bits(runs[1][0])) and np.array_equal(bits(runs[0][1]), bits(runs[1][1]))


@pytest.mark.parametrize("d, form, family", [(129, 1, "DEEP"), (256, 1, "DEEP"), (128, 1, "WIDE"), (257, 1, None), (200, 0, "RESIDUAL")])
def test_dispatch(d, form, family):
    small = synth.synth_cf(60, 40, 600, seed=13, min_len=3, n_neg=10)
    if family is None:  # no handle wider than 256 exists (gorse_mf_create refuses it for every trainer): form 1 has nothing to misroute there
        with pytest.raises(capi.GorseHipError) as wide:
            make_mf(small, d, std=0.1)
        assert wide.value.code == capi.ERR_INVALID
        return
    mf, _, _ = make_mf(small, d, std=0.1)
    assert mf.als_form() == (0, capi.ALS_FAMILY_NONE)
    mf.set_als_form(form)
    with pytest.raises(capi.GorseHipError) as bad:
        mf.set_als_form(2)
    assert bad.value.code == capi.ERR_INVALID
    mf.als_epoch(W, REG)
    assert mf.als_form() == (form, getattr(capi, "ALS_FAMILY_" + family))
    got = mf.get_factors()
    mf.close()
    if form == 0:  # the bits of a handle whose setter was never called
        mf, _, _ = make_mf(small, d, std=0.1)
        mf.als_epoch(W, REG)
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got, mf.get_factors()))
        mf.close()


def test_row_ranges(data, long_rows):
    lo, hi = 3, 120  # rows 0..2 and 120.. stay out: the long row 5 and the batch-edge rows are inside
    for side in (0, 1):
        start, full, _ = half(data, 160, side, 1)
        _, part, used = half(data, 160, side, 1, ranges=(lo, hi, lo, hi))
        assert used == capi.ALS_FAMILY_DEEP
        inside = np.zeros(N, bool)
        inside[lo:hi] = True
        assert np.array_equal(bits(part[inside]), bits(full[inside]))
        assert np.array_equal(bits(part[~inside]), bits(start[side][~inside]))
        assert not np.array_equal(bits(full[~inside]), bits(start[side][~inside]))
