"""GPU parity: floats.MM (csrc/sgemm.hip) in the forms the other sgemm tests never launch -- the 128 x 128 tile form of the MFMA
kernel (what bench.py's `mm` times), operands used in place with and without padded leading dimensions, the striding launch of
the odd last step, and the NT case at long rows, padded leading dimensions and past its grid cap.

The contract is the project's own, with no tolerance: every element has the bits of oracle.mm (the C restatement of _mm512_mm,
of floats.Dot for NT), the NN / TN / TT cases also the bits of the vector-ALU chain kernel.  Every case asserts, through
gorse_hip_test_sgemm_last_form, the kernel family it was written for: a moved threshold fails the test instead of emptying it.
Everything outside the m x n view of C (padding columns, and guard rows around a device-resident C) must keep its bit pattern;
those elements carry a NaN payload."""
import ctypes as C

import numpy as np
import pytest

from gorse_amd import capi
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

NN, TN, TT, NT = (0, 0), (1, 0), (1, 1), (0, 1)
CHAINS = (NN, TN, TT)
GUARD = np.uint32(0x7FC12345)  # a quiet NaN with a payload: no arithmetic produces it, and a == comparison of floats would miss it


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(autouse=True)
def _reset(oracle):
    oracle.set_isa(orc.ISA_AVX512)
    yield


def values(rng, rows, cols, pad):
    """24 binary orders of magnitude (test_sgemm_on_the_matrix_cores_is_the_same_chain); the padding columns hold the guard"""
    x = np.ldexp(rng.uniform(-1, 1, (rows, cols + pad)), rng.integers(-12, 12, (rows, cols + pad))).astype(np.float32)
    x.view(np.uint32)[:, cols:] = GUARD
    return x


def operands(rng, tA, tB, m, n, k, pad):
    a = values(rng, *((k, m) if tA else (m, k)), pad)
    b = values(rng, *((n, k) if tB else (k, n)), pad)
    c = values(rng, m, n, pad)
    c[::3, :n:5] = -0.0
    return a, b, c


def flat(x):
    """(an operand with no rows, k = 0, still needs an address)"""
    return x.ravel() if x.size else np.zeros(1, np.float32)


def run(entry, tA, tB, m, n, k, a, b, c):
    """one call through the host-buffer or the device-pointer entry point; a, b, c are 2-d arrays whose row length is the leading
    dimension.  Returns C as the call left it (padding included) and the form the call ran.  The device-resident C lies between
    two guard rows, which must come back untouched."""
    lda, ldb, ldc = a.shape[1], b.shape[1], c.shape[1]
    if entry == "host":
        got = capi.sgemm(tA, tB, m, n, k, flat(a), lda, flat(b), ldb, c.ravel(), ldc).reshape(m, ldc)
    else:
        import torch
        guard = np.full((1, ldc), GUARD, np.uint32).view(np.float32)
        ta, tb = torch.from_numpy(flat(a)).cuda(), torch.from_numpy(flat(b)).cuda()
        tc = torch.from_numpy(np.concatenate([guard, c, guard])).cuda()
        torch.cuda.synchronize()
        capi.sgemm_device(tA, tB, m, n, k, ta.data_ptr(), lda, tb.data_ptr(), ldb, tc[1:].data_ptr(), ldc)
        out = tc.cpu().numpy()
        assert (bits(out[0]) == GUARD).all() and (bits(out[-1]) == GUARD).all(), "rows around C were written"
        got = out[1:-1]
    return got, capi.lib().gorse_hip_test_sgemm_last_form()


def check(oracle, entry, tA, tB, m, n, k, a, b, c, form):
    """the call against the oracle, in the expected form; a chain case against the vector-ALU kernel as well"""
    tag = (entry, tA, tB, m, n, k, a.shape[1] - (m if tA else k))
    got, ran = run(entry, tA, tB, m, n, k, a, b, c)
    assert ran == form, (tag, ran)
    exp = oracle.mm(tA, tB, m, n, k, flat(a), a.shape[1], flat(b), b.shape[1], c.ravel(), c.shape[1]).reshape(c.shape)
    assert (bits(exp[:, n:]) == GUARD).all()  # (the reference leaves the padding alone)
    assert np.array_equal(bits(got), bits(exp)), (tag, int((bits(got) != bits(exp)).sum()))
    if (tA, tB) != NT and k > 0:
        L = capi.lib()
        L.gorse_hip_test_set_sgemm_valu(1)
        try:
            valu, ran = run(entry, tA, tB, m, n, k, a, b, c)
        finally:
            L.gorse_hip_test_set_sgemm_valu(0)
        assert ran == capi.SGEMM_VALU, (tag, ran)
        assert np.array_equal(bits(got), bits(valu)), tag
    return exp


# ---- the 128 x 128 tile form: >= 512 tiles of 128 --------------------------------------------------------------------------------------
# (m, n, k, padding of every leading dimension, form).  65409 x 3 is 512 x 1 tiles with one live column block: k = 1 skips the MFMA
# loop (k2 == 0) and runs the last step alone.  65408 x 3 is 511 tiles, the other side of the threshold.  32705 x 129: odd k over
# blocks of 16 + 16 + 1, all four quarters of the tile live, and 8.4M padded elements for a last-step launch capped at 4096 x 256
# threads: it strides.  129 x 32705: a wide grid, even k with a partial last block.
TILE128 = [
    (65409, 3, 1, 1, capi.SGEMM_MFMA128),
    (65409, 3, 2, 1, capi.SGEMM_MFMA128),
    (65409, 3, 3, 1, capi.SGEMM_MFMA128),
    (65408, 3, 3, 1, capi.SGEMM_MFMA64),
    (32705, 129, 33, 2, capi.SGEMM_MFMA128),
    (129, 32705, 66, 0, capi.SGEMM_MFMA128),
]


@pytest.mark.parametrize("trans", CHAINS, ids=("NN", "TN", "TT"))
@pytest.mark.parametrize("m,n,k,pad,form", TILE128, ids=lambda v: str(v))
def test_128_tile_form_is_the_same_chain(oracle, m, n, k, pad, form, trans):
    tA, tB = trans
    rng = np.random.default_rng([m, n, k, tA, tB])
    a, b, c = operands(rng, tA, tB, m, n, k, pad)
    check(oracle, "host", tA, tB, m, n, k, a, b, c, form)


@pytest.mark.parametrize("trans", CHAINS, ids=("NN", "TN", "TT"))
@pytest.mark.parametrize("k", [4, 5])
def test_128_tile_form_takes_no_padded_zero_step(oracle, k, trans):
    """Every product is -0 (one factor +0, the other -0, which one alternating with l), so an element that starts as -0 stays -0
    through the true chain and an element that starts as +0 stays +0; a single extra step on padded zeros (+0 * +0) would turn the
    -0 into +0.  k = 4: pairs only, a partial block; k = 5: the odd last step."""
    tA, tB = trans
    m, n = 65409, 3
    a = np.zeros((k, m) if tA else (m, k), np.float32)
    b = np.zeros((n, k) if tB else (k, n), np.float32)
    (a.T if tA else a)[:, 1::2] = -0.0  # A(i, l) = -0 at odd l
    (b if tB else b.T)[:, 0::2] = -0.0  # B(l, j) = -0 at even l
    c = np.full((m, n), -0.0, np.float32)
    c[::7] = 0.0
    exp = check(oracle, "host", tA, tB, m, n, k, a, b, c, capi.SGEMM_MFMA128)
    assert np.array_equal(bits(exp), bits(c))  # (what the chain gives by the argument above, whoever computes it)


# ---- operands used in place: whole tiles, k a multiple of 16, device-resident --------------------------------------------------------
IN_PLACE = [
    (2048, 4096, 48, capi.SGEMM_MFMA128),   # 16 x 32 tiles of 128
    (65536, 128, 16, capi.SGEMM_MFMA128),   # 512 x 1: one block of l
    (256, 256, 64, capi.SGEMM_MFMA64),
]


@pytest.mark.parametrize("trans", CHAINS, ids=("NN", "TN", "TT"))
@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("m,n,k,form", IN_PLACE, ids=lambda v: str(v))
def test_operands_in_place(oracle, m, n, k, form, pad, trans):
    """no re-layout: the kernel reads A and B and updates C through the caller's leading dimensions (ld == columns, and views into
    tensors 5 columns wider); nothing of the C tensor outside the m x n view changes"""
    tA, tB = trans
    rng = np.random.default_rng([m, n, k, pad, tA, tB])
    a, b, c = operands(rng, tA, tB, m, n, k, pad)
    check(oracle, "device", tA, tB, m, n, k, a, b, c, form | capi.SGEMM_IN_PLACE)


# ---- NT: one floats.Dot per element ----------------------------------------------------------------------------------------------------
# k mod 16 in {0, 1, 7, 8, 15}: the 16-lane body alone, with the scalar tail, with the 8-lane tail, with both -- on both sides of
# k = 512 (128 k bytes of LDS staging reach the 64 KB a kernel gets without asking) and of k = 1280 (they reach a CU's 160 KB), and
# at the bound of 8192.  363 x 363 = 131,769 elements > 8192 blocks x 16 groups: the grid strides.
NT_CASES = [(4, 4, 512), (4, 4, 513), (17, 3, 519), (6, 6, 1280), (40, 33, 1281), (9, 5, 1288), (3, 4, 8191), (5, 7, 8192),
            (363, 363, 19)]


@pytest.mark.parametrize("entry", ["host", "device"])
@pytest.mark.parametrize("m,n,k", NT_CASES, ids=lambda v: str(v))
def test_nt_long_rows_padded(oracle, m, n, k, entry):
    rng = np.random.default_rng([m, n, k])
    a, b, c = operands(rng, 0, 1, m, n, k, 3)
    form = capi.SGEMM_NT | (capi.SGEMM_NT_LONG if k > 512 else 0)
    check(oracle, entry, 0, 1, m, n, k, a, b, c, form)


@pytest.mark.parametrize("entry", ["host", "device"])
def test_k_zero(oracle, entry):
    """NT overwrites C with the dot of two empty rows, as the oracle does; NN accumulates nothing and launches nothing"""
    rng = np.random.default_rng(3)
    m = n = 3
    a, b, c = operands(rng, 0, 1, m, n, 0, 2)
    exp = check(oracle, entry, 0, 1, m, n, 0, a, b, c, capi.SGEMM_NT)
    assert (bits(exp[:, :n]) == 0).all()
    a, b, c = operands(rng, 0, 0, m, n, 0, 2)
    got, ran = run(entry, 0, 0, m, n, 0, a, b, c)
    assert ran == capi.SGEMM_NONE
    assert np.array_equal(bits(got), bits(c))


def test_nt_k_past_the_bound_is_refused():
    """k = 8193: GORSE_ERR_INVALID from both entry points, C untouched, nothing launched"""
    import torch
    rng = np.random.default_rng(4)
    m, n, k = 3, 4, 8193
    a, b, c = operands(rng, 0, 1, m, n, k, 3)
    L = capi.lib()
    f32p = C.POINTER(C.c_float)
    mine = c.copy()
    rc = L.gorse_hip_sgemm(0, 0, 1, m, n, k, a.ctypes.data_as(f32p), a.shape[1], b.ctypes.data_as(f32p), b.shape[1],
                           mine.ctypes.data_as(f32p), c.shape[1])
    assert rc == capi.ERR_INVALID and b"8192" in L.gorse_hip_last_error()
    assert L.gorse_hip_test_sgemm_last_form() == capi.SGEMM_NONE
    assert np.array_equal(bits(mine), bits(c))
    ta, tb, tc = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), torch.from_numpy(c.copy()).cuda()
    torch.cuda.synchronize()
    with pytest.raises(capi.GorseHipError) as e:
        capi.sgemm_device(0, 1, m, n, k, ta.data_ptr(), a.shape[1], tb.data_ptr(), b.shape[1], tc.data_ptr(), c.shape[1])
    assert e.value.code == capi.ERR_INVALID
    assert L.gorse_hip_test_sgemm_last_form() == capi.SGEMM_NONE
    assert np.array_equal(bits(tc.cpu().numpy()), bits(c))
