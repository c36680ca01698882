"""gorse_mf_recommend on the matrix route (gorse_mf_set_recommend_route(h, 1), csrc/recommend_mfma.hip): rec_mfma_kernel forms the
scores on v_mfma_f32_32x32x1_2b_f32 and must hand rec_finish_kernel exactly what the vector kernel hands it.

The expected rows are test_gpu_mf_recommend's: numpy candidate lists ranked and scored by the oracle.  Every case sets route 1,
asserts which kernel served the call, and holds items, counts, padding, score bits and the threshold / literal split to them.  No
query of a case without a deliberate tie or NaN is tied at these seeds (asserted), so the threshold path is what is tested."""
import numpy as np
import pytest

import test_gpu_mf_recommend as MR
from gorse_amd import capi
from test_gpu_mf_recommend import _hooks_at_default, base_factors, base_rows, expected, make_mf  # noqa: F401 (the fixture resets the hooks)

pytestmark = pytest.mark.gpu

U, I = MR.U, MR.I


def run(mf, P, Q, rows, users, k, ok=None, seen=None, used=1, literal=None):
    """one route-1 call against the oracle; literal = the queries the literal path must answer (None: the tied ones, and no others)"""
    exp_i, exp_s, exp_c, tied = expected(P, Q, rows, users, k, ok, seen)
    sp, si = MR.csr(seen) if seen is not None else (None, None)
    mf.set_recommend_route(1)
    got_i, got_s, got_c = mf.recommend(users, k, ok, sp, si)
    assert mf.recommend_route() == (1, used)
    assert np.array_equal(got_c, exp_c) and np.array_equal(got_i, exp_i), np.flatnonzero((got_i != exp_i).any(axis=1))[:10]
    assert np.array_equal(got_s.view(np.uint32), exp_s.view(np.uint32))
    n_fast, n_lit, _ = mf.recommend_stats()
    if k <= MR.FAST_CAP:
        want = int(tied.sum()) if literal is None else literal
        assert (n_fast, n_lit) == (len(users) - want, want)
    return got_s, tied


@pytest.mark.parametrize("d,used", [(16, 1), (32, 1), (48, 1), (80, 1), (128, 1), (256, 1), (24, 0), (100, 0), (272, 0)])
def test_every_served_width_and_the_fallbacks(d, used):
    """one chain step, even and odd chunk counts, the widest; widths with an 8-lane or scalar tail fall back.  No multiple of 16 above
    256 can fall back: gorse_mf_create refuses nFactors > 256, so 272 reaches neither kernel, and that refusal is what is held"""
    P, Q = base_factors(d)
    rows = base_rows()
    if d > 256:
        with pytest.raises(capi.GorseHipError) as e:
            make_mf(P, Q, rows)
        assert e.value.code == capi.ERR_INVALID
        return
    _, tied = run(make_mf(P, Q, rows), P, Q, rows, np.arange(U, dtype=np.int32), 10, used=used)
    assert not tied.any()


@pytest.mark.parametrize("nq,k,slices,buffer,own_ok", [(1, 10, 0, 0, False), (31, 1, 1, 0, True), (33, 100, 3, 0, False), (129, 256, 0, 1, True),
                                                       (300, 10, 3, 1, False), (300, 100, 1, 1, True), (129, 257, 0, 0, False)])
def test_query_counts_k_and_hooks(nq, k, slices, buffer, own_ok):
    """user lists with -1 entries and repeats across the 32-query wave edge and the 128-query workgroup edge, seen rows, an explicit
    item filter; user 1 has no candidate, user 2 fewer than k; slices 1 and 3 (ragged), the buffer at k + 2 and at its default"""
    P, Q = base_factors(64)
    rows = base_rows()
    rng = np.random.default_rng(100 + nq + k)
    users = rng.integers(0, U, nq).astype(np.int32)
    users[:8] = np.array([1, 2, 2, -1, 0, 17, 17, -1], np.int32)[:nq]
    ok = (rng.random(I) < 0.7).astype(np.uint8) if own_ok else None
    capi.lib().gorse_hip_test_set_recommend(slices, buffer, 0)
    _, tied = run(make_mf(P, Q, rows), P, Q, rows, users, k, ok=ok, seen=MR.base_seen(users, rng), used=1 if k <= MR.FAST_CAP else 0)
    assert not tied.any()


@pytest.mark.parametrize("d", [16, 48])
def test_bit_edges(d):
    rng = np.random.default_rng(40 + d)
    P = rng.standard_normal((8, d)).astype(np.float32)
    Q = rng.standard_normal((I, d)).astype(np.float32)
    P[0] = 0.0
    Q[5] = -np.abs(Q[5])
    rows = [np.array([u], np.int32) for u in range(8)]
    ones = np.ones(I, np.uint8)
    one = np.zeros(I, np.uint8)
    one[5] = 1
    mf = make_mf(P, Q, rows)
    # +0 times a negative row: every product, lane sum and the total are -0, on the threshold path
    s, tied = run(mf, P, Q, rows, np.array([0], np.int32), 3, ok=one)
    assert s.view(np.uint32)[0, 0] == 0x80000000 and not tied.any()
    # subnormal products and lane sums
    Ps, Qs = (P * np.float32(2.0 ** -66)).astype(np.float32), (Q * np.float32(2.0 ** -66)).astype(np.float32)
    mf.set_factors(Ps, Qs)
    s, tied = run(mf, Ps, Qs, rows, np.arange(1, 8, dtype=np.int32), 10, ok=ones)
    assert not tied.any() and (np.abs(s) < np.float32(1.1754944e-38)).all() and (s != 0).all()
    # a NaN in an admissible item's row sends its queries to the literal path, in an excluded item's row nobody
    Qn = Q.copy()
    Qn[700, 3] = np.nan
    users = np.array([1, 2, 3], np.int32)
    mf.set_factors(P, Qn)
    run(mf, P, Qn, rows, users, 3, ok=ones, literal=3)
    ok = ones.copy()
    ok[700] = 0
    _, tied = run(mf, P, Qn, rows, users, 3, ok=ok)
    assert not tied.any()
    # two identical rows among user 1's best: literal by the tie rule, the others stay on the threshold path
    Qt = Q.copy()
    Qt[100] = Qt[101] = 4.0 * np.sign(P[1])
    mf.set_factors(P, Qt)
    _, tied = run(mf, P, Qt, rows, users, 3, ok=ones)
    assert tied.tolist() == [True, False, False]


@pytest.mark.parametrize("slices,buffer", [(1, 0), (3, 1)])
def test_every_item_beats_the_running_threshold(slices, buffer):
    """user 0's scores ascend with the item index over a whole slice: every row of every tile is staged and drained"""
    P, Q, rows = MR.monotone_case()
    capi.lib().gorse_hip_test_set_recommend(slices, buffer, 0)
    run(make_mf(P, Q, rows), P, Q, rows, np.arange(4, dtype=np.int32), 10, ok=np.ones(I, np.uint8))


def test_candidate_chain_follows_the_handle_and_bad_routes_are_refused():
    P, Q = base_factors(48)
    rows = base_rows()
    mf = make_mf(P, Q, rows)
    users = np.arange(0, U, 3, dtype=np.int32)
    got = []
    for route in (0, 1):
        mf.set_recommend_route(route)
        chain = capi.CandidateChain(I)
        chain.begin(users.size, 20, *MR.csr([rows[u][:30] for u in users]))
        chain.add_mf(mf, users, 15)
        chain.finish()
        got.append(chain.get())
        assert mf.recommend_route() == (route, route)
        chain.close()
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(*got)) and got[0][0][-1] > 0
    for bad in (2, -1):
        with pytest.raises(capi.GorseHipError) as e:
            mf.set_recommend_route(bad)
        assert e.value.code == capi.ERR_INVALID and mf.recommend_route()[0] == 1
