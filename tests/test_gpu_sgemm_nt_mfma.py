"""GPU parity: floats.MM's NT case as tiles on the matrix cores (csrc/sgemm_nt.hip sgemm_nt_mfma_kernel).  Every element has the bits
of oracle.mm under ISA_AVX512 (floats.Dot of two rows), with no tolerance; operands, guards and the form assertion are those of
test_gpu_sgemm_forms.py."""
import numpy as np
import pytest

from gorse_amd import capi
from oracle import oracle as orc
from test_gpu_sgemm_forms import GUARD, bits, check, operands, run

pytestmark = pytest.mark.gpu

NT_MFMA = capi.SGEMM_NT | capi.SGEMM_NT_MFMA


@pytest.fixture
def nt_mode(oracle):
    oracle.set_isa(orc.ISA_AVX512)
    L = capi.lib()
    yield L.gorse_hip_test_set_sgemm_nt
    L.gorse_hip_test_set_sgemm_nt(0)


def old_form(k):
    return capi.SGEMM_NT | (capi.SGEMM_NT_LONG if k > 512 else 0)


# k: one chain step; each tail alone and both; both sides of a k block of 32, 64 or 128; an odd number of chunks; the bound.
# (m, n, pad): ragged tiles on both sides with rows off 16 bytes; several wave tiles with aligned rows; a single element.
@pytest.mark.parametrize("entry", ["host", "device"])
@pytest.mark.parametrize("m,n,pad", [(33, 31, 3), (130, 65, 0), (1, 1, 3)], ids=lambda v: str(v))
@pytest.mark.parametrize("k", [16, 17, 24, 31, 32, 33, 63, 64, 65, 127, 128, 129, 272, 8191, 8192])
def test_bits(oracle, nt_mode, k, m, n, pad, entry):
    nt_mode(2)
    a, b, c = operands(np.random.default_rng([m, n, k]), 0, 1, m, n, k, pad)
    check(oracle, entry, 0, 1, m, n, k, a, b, c, NT_MFMA)


@pytest.mark.parametrize("k", [16, 48, 80, 88])
def test_no_padded_step(oracle, nt_mode, k):
    """Every product is -0 (one factor +0, the other -0, which one alternating with the element), so every lane chain, tree and
    tail sum is -0; one step on padded zeros (+0 * +0) anywhere would leave +0."""
    nt_mode(2)
    m, n = 33, 31
    a, b = np.zeros((m, k), np.float32), np.zeros((n, k), np.float32)
    a[:, 1::2] = -0.0
    b[:, 0::2] = -0.0
    c = np.full((m, n), GUARD, np.uint32).view(np.float32)
    exp = check(oracle, "host", 0, 1, m, n, k, a, b, c, NT_MFMA)
    assert (bits(exp) == 0x80000000).all()


def test_subnormals(oracle, nt_mode):
    """products and partial sums in the subnormal range: the MFMA chain, the tile tree and the tails must round as fmaf and add do"""
    nt_mode(2)
    m, n, k = 65, 33, 40
    rng = np.random.default_rng(19)
    a = np.ldexp(rng.uniform(-1, 1, (m, k)), rng.integers(-80, -60, (m, k))).astype(np.float32)
    b = np.ldexp(rng.uniform(-1, 1, (n, k)), rng.integers(-80, -60, (n, k))).astype(np.float32)
    a[::7, ::3] = -0.0
    c = np.full((m, n), GUARD, np.uint32).view(np.float32)
    exp = check(oracle, "host", 0, 1, m, n, k, a, b, c, NT_MFMA)
    assert (np.abs(exp[exp != 0]) < 1.17e-38).any()


@pytest.mark.parametrize("m,n,k,mfma", [(1024, 256, 64, True), (512, 512, 15, False), (8200, 31, 64, False), (511, 512, 64, False)],
                         ids=lambda v: str(v))
def test_automatic_rule(oracle, nt_mode, m, n, k, mfma):
    """k >= 16, min(m, n) >= 32 and m n >= 2^18 take the tiles; one short of any of the three keeps the per-element kernels"""
    nt_mode(0)
    a, b, c = operands(np.random.default_rng([m, n, k]), 0, 1, m, n, k, 0)
    check(oracle, "device", 0, 1, m, n, k, a, b, c, NT_MFMA if mfma else old_form(k))


def test_modes_agree(oracle, nt_mode):
    m, n, k = 1024, 256, 64
    a, b, c = operands(np.random.default_rng(5), 0, 1, m, n, k, 0)
    nt_mode(1)
    old, ran_old = run("device", 0, 1, m, n, k, a, b, c)
    nt_mode(2)
    new, ran_new = run("device", 0, 1, m, n, k, a, b, c)
    assert (ran_old, ran_new) == (old_form(k), NT_MFMA)
    assert np.array_equal(bits(old), bits(new))
