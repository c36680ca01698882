"""One ALS epoch at EVERY nFactors the kernel tables serve.  The other ALS tests pick widths (7, 8, 16, 24, 32, 33, 40, 48, 50, 56, 64,
65, 96, 128, ...); which kernel a width takes is looked up in tables (csrc/als.hip: als_form, tile_kernels, wide_kernel, the long
solve's width list), and a table can have a hole between the widths somebody happened to pick."""
import numpy as np
import pytest

from cf_cases import assert_als_close, bits, make_mf
from gorse_amd import capi, synth

pytestmark = pytest.mark.gpu

RETIRED_BITS = 4 | 16 | 32 | 256


@pytest.fixture
def als_paths():
    """restores the automatic ALS row-solve choice and the default row plan after a test"""
    yield
    capi.lib().gorse_hip_test_set_als_path(0)
    capi.lib().gorse_hip_test_set_als_plan(0, 0)


def test_als_epoch_at_every_width_and_retired_switch_bits_do_nothing(oracle, als_paths):
    """nFactors 7 (the narrowest the suite creates) .. 128, then 129 and 200 (the residual sweep), path 0, one epoch against the oracle
    with test_als_epoch_parity's bar.  The row plan (16, 16) makes a row of more than 16 entries a long one, so that at every width the
    short-row kernel, the chunk kernel and the long rows' solve (als_long_solve_kernel / als_wide_long_kernel) all launch.  (No row of
    60 x 40 can reach the nine chunks that send a long row through als_partial_reduce_kernel first; that kernel is one kernel for every
    width and has test_als_long_row_partials_added_per_element_equal_the_solve_kernels_own_sum.)

    Then nFactors 24 and 96 with bits 4 | 16 | 32 | 256 of gorse_hip_test_set_als_path: they once asked for probes (lockstep waves,
    "no sweep" / "S not added" timing forms of als_wide_kernel whose results were garbage by design, eight waves per workgroup) and are
    now ignored, so both factor matrices equal path 0's in every bit.  A build that still has the probes fails this at nFactors 96
    (bits 16 / 32): it is the one assertion here that tells the two builds apart."""
    L = capi.lib()
    data = synth.synth_cf(60, 40, 600, seed=13, min_len=3, n_neg=10)
    L.gorse_hip_test_set_als_plan(16, 16)
    rows = np.concatenate([np.diff(data.uptr), np.diff(data.iptr)])
    assert rows.max() > 16 and (rows[rows > 0] <= 16).any()  # both kinds of row on the plan

    def epoch(d, path):
        L.gorse_hip_test_set_als_path(path)
        mf, P, Q = make_mf(data, d, std=0.1)
        mf.als_epoch(0.05, 0.015)
        got = mf.get_factors()
        mf.close()
        return P, Q, got

    plain = {}
    for d in list(range(7, 129)) + [129, 200]:
        P, Q, (gP, gQ) = epoch(d, 0)
        plain[d] = (gP, gQ)
        eP, eQ = oracle.als_epoch(P, Q, data.uptr, data.uidx, data.iptr, data.iidx, 0.05, 0.015)
        assert np.isfinite(gP).all() and np.isfinite(gQ).all(), d
        scale = max(np.abs(eP).max(), np.abs(eQ).max())
        assert np.abs(gP - eP).max() < 1e-4 * scale and np.abs(gQ - eQ).max() < 1e-4 * scale, d
        assert_als_close(gP, eP, "P, nFactors %d" % d)
        assert_als_close(gQ, eQ, "Q, nFactors %d" % d)
    for d in (24, 96):
        _, _, (gP, gQ) = epoch(d, RETIRED_BITS)
        assert np.array_equal(bits(gP), bits(plain[d][0])) and np.array_equal(bits(gQ), bits(plain[d][1])), d
