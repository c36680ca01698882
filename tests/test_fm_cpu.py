"""CPU checks of the factorization machine: the numpy restatement the GPU tests measure against (its closed-form gradient
against finite differences, its fp32 FMA), the reference's classification-metric KATs through the host mirror, and the
handle's refusal to run without a device."""
from fractions import Fraction

import numpy as np
import pytest

import fm_ref as R


def test_restated_gradient_matches_finite_differences():
    rng = np.random.default_rng(3)
    nf, d = 9, 4
    rows = [(rng.choice(nf, k, replace=False), rng.normal(1, 0.7, k)) for k in (1, 3, 5, 2, 4, 5)]
    rows.append((np.array([0, 2]), np.array([1.5, -0.5])))  # feature 0 in use next to padding
    idx, val = R.pad(rows, 6)
    val = val.astype(np.float64)
    t = np.array([1, -1, 1, 1, -1, -1, 1], np.float64)
    B, W, V = 0.3, rng.normal(0, 0.5, nf), rng.normal(0, 0.5, (nf, d))
    dB, dW, dV, _ = R.grads64(B, W, V, idx, val, t)
    h = 1e-6

    def L(B_, W_, V_):
        return R.loss64(B_, W_, V_, idx, val, t)

    assert abs((L(B + h, W, V) - L(B - h, W, V)) / (2 * h) - dB) < 1e-7
    for i in range(nf):
        e = np.zeros(nf)
        e[i] = h
        assert abs((L(B, W + e, V) - L(B, W - e, V)) / (2 * h) - dW[i]) < 1e-7
        for f in range(d):
            E = np.zeros((nf, d))
            E[i, f] = h
            assert abs((L(B, W, V + E) - L(B, W, V - E)) / (2 * h) - dV[i, f]) < 1e-7


def test_restated_fma_is_correctly_rounded():
    rng = np.random.default_rng(5)
    a = rng.normal(0, 1, 3000).astype(np.float32)
    b = rng.normal(0, 1e-3, 3000).astype(np.float32)
    c = (rng.normal(0, 1e-3, 3000) * np.where(rng.random(3000) < 0.5, 1, 1e-4)).astype(np.float32)
    # operands whose exact sum lies next to a halfway point of fp32
    a[:8], b[:8], c[:8] = np.float32(1 + 2 ** -12), np.float32(1 + 2 ** -12), np.float32(-(2 ** -24))
    got = R.fma32(a, b, c)
    for i in range(a.size):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        r = np.float32(got[i])
        lo, hi = np.nextafter(r, np.float32(-np.inf)), np.nextafter(r, np.float32(np.inf))
        err = abs(Fraction(float(r)) - exact)
        assert err <= abs(Fraction(float(lo)) - exact) and err <= abs(Fraction(float(hi)) - exact), i


def test_adam_lr_first_steps():
    f = np.float32
    assert R.adam_lr(0.01, 1) == f(f(f(0.01) * np.sqrt(f(1) - f(0.999))) / (f(1) - f(0.9)))
    assert R.pow32(f(0.9), 2) == f(f(0.9) * f(0.9))


def test_classification_metric_kats():
    """model/ctr/evaluator_test.go:22-45"""
    from gorse_amd import ctr
    assert ctr.Precision([1, 1, 1], [1]) == np.float32(0.75)
    assert ctr.Precision([], []) == 0
    assert ctr.Recall([1, -1, -1, -1], []) == np.float32(0.25)
    assert ctr.Recall([], []) == 0
    assert ctr.Accuracy([1, 1, -1, -1], [1, 1, -1, -1]) == np.float32(0.5)
    assert ctr.Accuracy([], []) == 0
    assert ctr.AUC([0.9, 0.8, 0.3], [0.1, 0.5, 0.85]) == np.float32(6 / 9)
    assert ctr.AUC([], [0.5]) == 0


def test_fm_create_fails_without_device():
    from gorse_amd import capi
    if capi.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(capi.GorseHipError) as e:
        capi.FM(10, 8)
    assert e.value.code == capi.ERR_NO_DEVICE


def test_fm_create_argument_validation():
    from gorse_amd import capi
    for nf, d in ((10, 0), (10, 129), (0, 8)):
        with pytest.raises(capi.GorseHipError) as e:
            capi.FM(nf, d)
        assert e.value.code == capi.ERR_INVALID
