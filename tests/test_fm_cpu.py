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


# ---- the helpers of test_gpu_fm_train_shapes.py ---------------------------------------------------------------------------

def _small_model(nf, d, seed, sd=0.1):
    rng = np.random.default_rng(seed)
    return np.float32(0.1), rng.normal(0, sd, nf).astype(np.float32), rng.normal(0, sd, (nf, d)).astype(np.float32)


def test_position_weights_and_gradient_scale():
    idx, val, tgt, _ = R.shape_batch(8, 61, 70, seed=1)
    B, W, V = _small_model(61, 8, 2)
    base = R.grads64(B, W, V, idx, val, tgt)
    ones = R.grads64(B, W, V, idx, val, tgt, np.ones(idx.shape), np.ones(idx.shape + (8,)))
    assert all(np.array_equal(a, b) for a, b in zip(base, ones))
    r = 13
    j = int(np.flatnonzero((idx[r] == 7) & (val[r] != 0))[0])
    wW, wV = np.ones(idx.shape), np.ones(idx.shape + (8,))
    wW[r, j], wV[r, j, 3] = 0, 2
    g, cw, c, _ = R._contrib64(B, W, V, idx, val, tgt)
    _, dW, dV, loss = R.grads64(B, W, V, idx, val, tgt, wW, wV)
    assert loss == base[3]  # the forward pass does not see the weights
    eW, eV = np.zeros(61), np.zeros((61, 8))
    eW[7], eV[7, 3] = -cw[r, j], c[r, j, 3]
    assert np.allclose(dW - base[1], eW, rtol=0, atol=1e-15) and np.allclose(dV - base[2], eV, rtol=0, atol=1e-15)
    assert eW[7] != 0 and eV[7, 3] != 0
    aW, aV = R.grad_scale64(B, W, V, idx, val, tgt)
    assert np.all(aW >= np.abs(base[1])) and np.all(aV >= np.abs(base[2]) * (1 - 1e-12))
    once = np.array([f for f in range(61) if len(R.rows_of(idx, val, f)) == 1])
    assert len(once) >= 8 and np.allclose(aW[once], np.abs(base[1][once]), rtol=1e-12)
    assert np.all(aW[~R.touched_rows(idx, val, 61)] == 0)


@pytest.mark.parametrize("d,lanes", [(1, 8), (8, 8), (9, 16), (16, 16), (17, 32), (32, 32), (33, 64), (64, 64), (65, 64), (128, 64)])
def test_shape_batch_keeps_its_promised_lists(d, lanes):
    assert R.lanes_for(d) == lanes and R.trip(d) == 4 * (64 // lanes)
    T, n, nf = R.trip(d), 272, 211
    idx, val, tgt, lists = R.shape_batch(d, nf, n, seed=d)
    assert (lists[7], lists[1], lists[2], lists[4]) == (n, T, T + 1, 2 * T - 1)
    for f, c in lists.items():
        assert len(R.rows_of(idx, val, f)) == c and ((idx == f) & (val != 0)).sum() == c, f  # once per row at most
    assert sum(c == 1 for c in lists.values()) == 8 and lists[nf - 2] == 1
    assert sum(1 for f, c in lists.items() if c == 1 and R.rows_of(idx, val, f)[0] == 5) == 3
    assert lists[0] == len(R.rows_of(idx, val, 0)) > 0               # feature 0 as a real feature ...
    assert np.all(val[:, -1] == 0) and np.all(idx[:, -1] == 0)       # ... next to padding in every row
    assert np.all((val != 0).sum(1) >= 2)
    t = R.touched_rows(idx, val, nf)
    assert not t[nf - 1] and t[nf - 2] and not t[3::5].any() and t.sum() > 100
    with pytest.raises(ValueError):
        R.shape_batch(d, nf, 2 * T - 2, seed=d)


def test_drift_set_features_come_and_go():
    nf, n, bs = 163, 230, 64
    idx, val, tgt = R.drift_set(n, nf, bs, seed=8)
    slots = R.batch_slots(idx, val, bs)
    assert len(slots) == 4 and n % bs == 38
    for f in range(10, 20):
        assert f in slots[0] and all(f not in s for s in slots[1:])
    for f in range(20, 30):
        assert f in slots[-1] and all(f not in s for s in slots[:-1])
    for f in (0, 100, 120, 140):
        assert all(f in s for s in slots)
    for f in (100, 120, 140):
        assert len({s[f] for s in slots}) >= 3, f  # the slot moves
    assert len(R.rows_of(idx, val, 140)) == n
    t = R.touched_rows(idx, val, nf)
    assert not t[1:10].any() and not t[nf - 6:].any()
    with pytest.raises(ValueError):
        R.drift_set(128, nf, 64, seed=8)  # no partial last batch


@pytest.mark.parametrize("adam", [False, True])
def test_step_trainer_is_trainer_one_step_at_a_time(adam):
    nf, d, n, bs = 163, 8, 230, 64
    idx, val, tgt = R.drift_set(n, nf, bs, seed=5)
    B, W, V = _small_model(nf, d, 6)
    a, b = R.Trainer(B, W, V), R.StepTrainer(B, W, V)
    for ep in range(2):
        ca = a.epoch(idx, val, tgt, bs, adam, 0.01, 0.01)
        cb = np.float32(0)
        for i in range(0, n, bs):
            sl = slice(i, i + bs)
            prev = [x.copy() for x in b.params[1:]]
            zero = [b.zero_step(k, prev[k - 1], adam, 0.01, 0.01) for k in (1, 2)]
            cb = np.float32(cb + np.float32(b.step(idx[sl], val[sl], tgt[sl], adam, 0.01, 0.01)))
            un = ~b.touched  # a zero gradient is what an untouched row's float64 gradient rounds to
            assert un.any() and not un.all()
            assert np.array_equal(b.params[1][un], zero[0][un])
            assert np.array_equal(b.params[2][un].reshape(-1), zero[1].reshape(nf, d)[un].reshape(-1))
        assert ca == cb and a.t == b.t == (4 * (ep + 1) if adam else 0)  # four batches per epoch
        for x, y in zip(a.params, b.params):
            assert np.array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32))
    assert b.ever.sum() > b.touched.sum()
    # a trainer that starts at t = 4 takes Adam's fifth step
    c = R.StepTrainer(B, W, V, t=4)
    c.step(idx[:bs], val[:bs], tgt[:bs], adam, 0.01, 0.01)
    assert c.t == (5 if adam else 4)


def test_recorded_divergence_from_float64_holds():
    """what K_MULTI stands on: the fp32-step reference against the all-float64 run, every schedule of the multi-step tests"""
    worst = {False: 0.0, True: 0.0}
    for d in (8, 64, 100):
        idx, val, tgt = R.drift_set(230, 163, 64, seed=d)
        B, W, V = _small_model(163, d, d + 7)
        for adam in (False, True):
            lr = 0.01 if adam else 0.1
            a, b = R.StepTrainer(B, W, V), R.StepTrainer(B, W, V, dtype=np.float64)
            for _ in range(3):
                a.epoch(idx, val, tgt, 64, adam, lr, 0.01)
                b.epoch(idx, val, tgt, 64, adam, lr, 0.01)
                worst[adam] = max(worst[adam], R.params_report(a.params, b.params, lr, 1.0))
    for adam in (False, True):
        assert 0.5 * R.DIVERGENCE[adam] <= worst[adam] <= R.DIVERGENCE[adam], worst
        assert R.K_MULTI[adam] == 4 * R.DIVERGENCE[adam]


def test_float64_step_agrees_with_the_fp32_step():
    rng = np.random.default_rng(9)
    p, g = rng.normal(0, 0.1, 50).astype(np.float32), rng.normal(0, 0.01, 50).astype(np.float32)
    z = np.zeros(50, np.float32)
    for adam in (False, True):
        a = R.opt_step32(p, g, z, z, 0.01, 0.01, adam)
        b = R.opt_step64(p, g, z, z, 0.01, np.float64(np.float32(0.01)), adam)
        for x, y in zip(a, b):
            assert np.allclose(x, y, rtol=1e-6, atol=1e-9)
    assert R.ulp_diff(np.float32(1), np.nextafter(np.float32(1), np.float32(2)))[0] == 1
    assert R.straddles(np.array([1, 1, 1, 1, 0, 1, 1, 1, 0, 0, 0, 0, 1], bool)) == 1
    got, want = np.arange(1, 20, dtype=np.float32), np.arange(1, 20, dtype=np.float32)
    got[2], got[17] = np.nextafter(got[2], np.float32(99)), np.nextafter(got[17], np.float32(99))
    assert R.untouched_report(got, want, np.ones(19, bool)) == (1, 1, 16, 3)


# one d per instantiation of fm_forward_kernel / fm_accum_kernel: <8,1> <16,1> <32,1> <64,1> <64,2>
@pytest.mark.parametrize("d", [8, 16, 32, 64, 100])
def test_one_step_bars_exclude_a_lost_position_and_a_mis_scaled_lane(d):
    """test_gpu_fm_train_shapes.py's one-step case under SGD with the fp32 reference's own step as the device: clean it
    passes; with any one position of the longest list dropped (or, at every 16th, doubled) in the reference's sums it is >= 10 bars out, on the
    parameters and on the carried gradient; with the last lane's share of one position dropped or doubled it fails both as well"""
    nf, n, lr, wd = 211, 272, 0.25, 0.01
    idx, val, tgt, _ = R.shape_batch(d, nf, n, seed=d)
    B, W, V = _small_model(nf, d, d + 50)
    dev = R.StepTrainer(B, W, V)
    cost = np.float32(dev.step(idx, val, tgt, False, lr, wd))

    def report(wW=None, wV=None):
        return R.one_step_report(B, W, V, idx, val, tgt, dev.params, cost, False, lr, wd, wW, wV)

    rep = report()
    assert max(rep[k] for k in ("cost", "B", "W", "V", "gW", "gV")) <= 1 and rep["gV"] <= 0.6, rep
    assert rep["W_unt"][:2] == (0, 0) and rep["V_unt"][:2] == (0, 0)
    for r in range(n):  # every position of the list dropped; doubled (the mirror image) at every 16th
        j = int(np.flatnonzero((idx[r] == 7) & (val[r] != 0))[0])
        for w in (0.0, 2.0) if r % 16 == 0 else (0.0,):
            wW, wV = np.ones(idx.shape), np.ones(idx.shape + (1,))
            wW[r, j], wV[r, j, 0] = w, w
            rp = report(wW, wV)
            assert max(rp["W"], rp["V"]) >= 10 and max(rp["gW"], rp["gV"]) >= 10, (r, w, rp)
    # one lane alone: the last lane in use (at d = 100 its second factor), its share of one position doubled or dropped
    c = R._contrib64(B, W, V, idx, val, tgt)[2][..., d - 1] * ((idx == 7) & (val != 0))
    r, j = np.unravel_index(np.argmax(np.abs(c)), c.shape)
    for w in (0.0, 2.0):
        wV = np.ones(idx.shape + (d,))
        wV[r, j, d - 1] = w
        rp = report(None, wV)
        assert rp["V"] > 1 and rp["gV"] >= 10 and rp["W"] <= 1 and rp["gW"] <= 1, (w, rp)


def test_multi_step_bar_excludes_a_lost_position_under_adam():
    """under Adam a lost position shows from the second step on: one position of feature 140's list dropped in the second
    batch of the first epoch leaves the parameters >= 10 K_MULTI bars apart at the end of that epoch"""
    nf, d, n, bs, lr, wd = 163, 8, 230, 64, 0.01, 0.01
    idx, val, tgt = R.drift_set(n, nf, bs, seed=d)
    B, W, V = _small_model(nf, d, d + 7)
    a, b = R.StepTrainer(B, W, V), R.StepTrainer(B, W, V)
    for i in range(0, n, bs):
        sl = slice(i, i + bs)
        a.step(idx[sl], val[sl], tgt[sl], True, lr, wd)
        wW = np.ones(idx[sl].shape)
        if i == bs:
            wW[9, int(np.flatnonzero(idx[sl][9] == 140)[0])] = 0
        b.step(idx[sl], val[sl], tgt[sl], True, lr, wd, wW, wW[..., None])
    assert R.params_report(b.params, a.params, lr, R.K_MULTI[True], a.slack) >= 10


def test_adam_slack_covers_gradients_within_their_bar():
    # the slack covers what gradients within a tenth of their bar do: every position's share off by 1e-6, four Adam steps
    nf, d, bs = 163, 8, 64
    idx, val, tgt = R.drift_set(230, nf, bs, seed=8)
    B, W, V = _small_model(nf, d, 15)
    a, b = R.StepTrainer(B, W, V), R.StepTrainer(B, W, V)
    for i in range(0, 230, bs):
        sl = slice(i, i + bs)
        a.step(idx[sl], val[sl], tgt[sl], True, 0.01, 0.01)
        w = np.full(idx[sl].shape, 1 + 1e-6)
        b.step(idx[sl], val[sl], tgt[sl], True, 0.01, 0.01, w, w[..., None])
    assert all(s.min() >= 0 for s in a.slack) and a.slack[2].max() > 0
    assert R.params_report(b.params, a.params, 0.01, 1e-7, a.slack) <= 1
    assert R.params_report(b.params, a.params, 0.01, 1e-7) > R.params_report(b.params, a.params, 0.01, 1e-7, a.slack)
    sgd = R.StepTrainer(B, W, V)
    sgd.step(idx[:bs], val[:bs], tgt[:bs], False, 0.1, 0.01)
    assert all(not s.any() for s in sgd.slack)
    worst = R.params_report([np.float32([1.0])], [np.float32([1.0 + 1e-3])], 0.0, 1e-4, [np.array([9e-4])])
    assert abs(worst - 1.0) < 1e-3
    # the slack counts up to SLACK_CAP bars and no further
    worst = R.params_report([np.float32([1.0])], [np.float32([2.0])], 0.0, 1e-4, [np.array([1e9])])
    assert abs(worst - 1.0 / (2e-4 * (1 + R.SLACK_CAP))) < 1e-3 * worst


# one d per instantiation, as above
@pytest.mark.parametrize("d", [8, 16, 32, 64, 100])
def test_one_step_adam_case_sees_the_gradient(d):
    """test_gpu_fm_train_shapes.py's one-step case under Adam with stand-in devices: the fp32 reference's own step passes, with
    few elements counted as ill-conditioned; a device that gives a touched row a zero gradient (a tag it does not match), the
    negated gradient, or another slot's gradient fails on that row"""
    nf, n, lr, wd = 211, 272, 0.01, 0.01
    idx, val, tgt, _ = R.shape_batch(d, nf, n, seed=d)
    B, W, V = _small_model(nf, d, d + 50)
    dB, dW, dV, loss = R.grads64(B, W, V, idx, val, tgt)

    def report(gW, gV):
        z = lambda x: np.zeros(x.size, np.float32)
        lr_t = R.adam_lr(lr, 1)
        got = (R.opt_step32(np.array([B]), np.array([dB], np.float32), z(dW[:1]), z(dW[:1]), wd, lr_t, True)[0][0],
               R.opt_step32(W, gW.astype(np.float32), z(W), z(W), wd, lr_t, True)[0],
               R.opt_step32(V, gV.astype(np.float32), z(V), z(V), wd, lr_t, True)[0].reshape(nf, d))
        return R.one_step_report(B, W, V, idx, val, tgt, got, np.float32(loss), True, lr, wd)

    rep = report(dW, dV)
    assert max(rep[k] for k in ("cost", "B", "W", "V")) <= 1 and rep["W_unt"][:2] == (0, 0) and rep["V_unt"][:2] == (0, 0)
    for name in ("W_ill", "V_ill"):
        n_ill, n_touched, ratio = rep[name]
        assert n_ill <= 0.011 * n_touched + 1 and ratio <= 1, rep  # measured: at most 1.04 % (d = 8, nf = 212)
    for f in (7, 4):  # the list of every row, the list of 2 U NG - 1 rows
        for what in ("zero", "negated", "wrong slot"):
            gW, gV = dW.copy(), dV.copy()
            if what == "zero":
                gW[f], gV[f] = 0, 0
            elif what == "negated":
                gW[f], gV[f] = -dW[f], -dV[f]
            else:
                gW[f], gV[f] = dW[1], dV[1]  # feature 1's sums: the neighbouring slot's
            rp = report(gW, gV)
            assert rp["V"] > 1, (f, what, rp)
            assert rp["W"] > 1 or what == "zero" or np.sign(gW[f] + wd * W[f]) == np.sign(dW[f] + wd * W[f]), (f, what, rp)
