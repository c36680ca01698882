"""The factorization machine on the MI355X (gorse_fm_*, ctr.AFM without the embedding branch) against the numpy
restatement in fm_ref.py: scoring, one optimizer step bit for bit where the reference's op sequence allows it, determinism,
ten-epoch training parity, the host mirror's Fit loop and the error paths."""
import numpy as np
import pytest

import fm_ref as R
from gorse_amd import capi

pytestmark = pytest.mark.gpu
f32 = np.float32


def _model(nf, d, seed, sd=0.3):
    rng = np.random.default_rng(seed)
    return f32(rng.normal(0, 0.5)), rng.normal(0, sd, nf).astype(f32), rng.normal(0, sd, (nf, d)).astype(f32)


@pytest.mark.parametrize("d", [1, 8, 16, 64, 128])
def test_scoring_parity(d):
    rng = np.random.default_rng(d)
    nf = 500
    rows = []
    for i in range(700):
        k = int(rng.integers(1, 33))
        a = rng.choice(nf, k, replace=False).astype(np.int32)
        if i % 5 == 0:
            a[0] = 0  # feature 0 is a real feature
        rows.append((a, rng.normal(0.5, 1.0, k).astype(f32)))
    idx, val = R.pad(rows, 40)  # wider than any row
    B, W, V = _model(nf, d, d + 100)
    fm = capi.FM(nf, d)
    fm.set_params(B, W, V)
    got = fm.predict(idx, val)
    want, _, scale = R.forward64(B, W, V, idx, val)
    assert np.all(np.abs(got - want) <= 1e-5 * scale + 1e-30), np.max(np.abs(got - want) / scale)


@pytest.mark.parametrize("adam", [False, True])
def test_one_step_parity(adam):
    nf, d, n = 203, 5, 64  # W: 203 = 12 x 16 + 11, V: 1015 = 63 x 16 + 7 elements; rows >= 150 are never touched
    rng = np.random.default_rng(11)
    rows = [(rng.choice(150, int(rng.integers(1, 7)), replace=False).astype(np.int32),
             rng.normal(1, 0.5, 6).astype(f32)) for _ in range(n)]
    rows = [(a, b[:len(a)]) for a, b in rows]
    idx, val = R.pad(rows, 6)
    tgt = np.where(rng.random(n) < 0.5, 1, -1).astype(f32)
    B, W, V = _model(nf, d, 12, sd=0.2)
    lr, wd = (0.01, 0.01) if adam else (0.05, 0.01)
    fm = capi.FM(nf, d)
    fm.set_params(B, W, V)
    fm.set_train(idx, val, tgt)
    cost = fm.epoch(n, capi.OPT_ADAM if adam else capi.OPT_SGD, lr, wd)
    gB, gW, gV = fm.get_params()

    dB, dW, dV, loss = R.grads64(B, W, V, idx, val, tgt)
    assert abs(cost - loss) <= 1e-5 * loss
    lr_t = R.adam_lr(lr, 1) if adam else f32(lr)
    touched = np.zeros(nf, bool)
    touched[np.unique(idx[val != 0])] = True
    for p0, g64, got, row_of in ((W, dW, gW, np.arange(nf)), (V.reshape(-1), dV.reshape(-1), gV.reshape(-1), np.arange(nf * d) // d)):
        L = p0.size
        zero = np.zeros(L, f32)
        ref_untouched = R.opt_step32(p0, zero, zero, zero, wd, lr_t, adam)[0]  # grad 0: what every untouched element gets
        ref_touched = R.opt_step32(p0, g64.astype(f32), zero, zero, wd, lr_t, adam)[0]
        un = ~touched[row_of]
        body = np.arange(L) < L - L % 16
        assert un[~body].any() and (un & body).any()
        assert np.array_equal(got[un & body].view(np.uint32), ref_untouched[un & body].view(np.uint32))
        ulp = np.abs(got[un & ~body].view(np.int32).astype(np.int64) - ref_untouched[un & ~body].view(np.int32).astype(np.int64))
        assert ulp.max() <= 1
        tol = 1e-5 * (np.abs(ref_touched[~un]) + lr)
        assert np.all(np.abs(got[~un] - ref_touched[~un]) <= tol)
    refB = R.opt_step32(np.array([B]), np.array([dB], f32), np.zeros(1, f32), np.zeros(1, f32), wd, lr_t, adam)[0][0]
    assert abs(gB - refB) <= 1e-5 * (abs(refB) + lr)


def test_determinism():
    idx, val, tgt = R.synth_ctr(6000, 300, 8, seed=4)
    idx[:, 0], val[:, 0] = 7, 1.0  # a feature in every row: a long position list per batch
    B, W, V = _model(300, 16, 5, sd=0.01)
    runs = []
    for _ in range(2):
        fm = capi.FM(300, 16)
        fm.set_params(B, W, V)
        fm.set_train(idx, val, tgt)
        costs = [fm.epoch(512, capi.OPT_ADAM, 0.01, 1e-4) for _ in range(3)]
        runs.append((np.array(costs, f32),) + tuple(np.asarray(x) for x in fm.get_params()))
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(np.asarray(a, f32).view(np.uint32), np.asarray(b, f32).view(np.uint32))


@pytest.mark.parametrize("adam", [True, False])
def test_training_parity(adam):
    nf, d = 2000, 8
    idx, val, tgt = R.synth_ctr(20000 + 500, nf, d, seed=21)  # 20 batches of 1024, the last one partial
    tidx, tval, ttgt = R.synth_ctr(4000, nf, d, seed=22)
    rng = np.random.default_rng(23)
    B, W, V = f32(0), rng.normal(0, 0.01, nf).astype(f32), rng.normal(0, 0.01, (nf, d)).astype(f32)
    lr, wd = (0.01, 1e-4) if adam else (0.1, 1e-4)
    fm = capi.FM(nf, d)
    fm.set_params(B, W, V)
    fm.set_train(idx, val, tgt)
    ref = R.Trainer(B, W, V)
    costs = []
    for _ in range(10):
        c_dev = fm.epoch(1024, capi.OPT_ADAM if adam else capi.OPT_SGD, lr, wd)
        c_ref = ref.epoch(idx, val, tgt, 1024, adam, lr, wd)
        assert abs(c_dev - c_ref) <= 1e-4 * abs(c_ref), (c_dev, c_ref)
        costs.append(c_dev)
    pos, neg = ttgt > 0, ttgt <= 0
    p_dev = fm.predict(tidx, tval)
    p_ref = R.forward64(*ref.params, tidx, tval)[0]
    a_dev, a_ref = R.auc(p_dev[pos], p_dev[neg]), R.auc(p_ref[pos], p_ref[neg])
    assert abs(a_dev - a_ref) <= 0.005
    assert costs[-1] < costs[0]  # the model learns at all


def _split(idx, val, tgt, nf):
    from gorse_amd import ctr
    lens = (val != 0).sum(1)
    indptr = np.concatenate([[0], np.cumsum(lens)])
    ii = np.concatenate([idx[i, :lens[i]] for i in range(len(lens))])
    vv = np.concatenate([val[i, :lens[i]] for i in range(len(lens))])
    return ctr.Dataset(nf, (indptr, ii, vv, tgt))


def test_host_twin_fit():
    from gorse_amd import ctr
    nf, d = 500, 8
    train = _split(*R.synth_ctr(5000, nf, d, seed=31), nf)
    test = _split(*R.synth_ctr(1000, nf, d, seed=32), nf)
    # evaluation schedule: epoch 0, every Verbose epochs, the last epoch
    m = ctr.FM(nFactors=d, nEpochs=7, batchSize=256, lr=0.01, reg=1e-4, optimizer=ctr.Adam, seed=1)
    s = m.Fit(train, test, Verbose=3)
    lg = m.log()
    assert [e for e, _, _ in lg] == [0, 3, 6, 7]
    assert lg[0][1] == 0 and all(c > 0 for _, c, _ in lg[1:])
    assert s.AUC == lg[-1][2] and s == m.Evaluate(test)
    # patience: with lr 0 the AUC never improves on epoch 0, so the Fit stops at epoch Patience + 1
    m = ctr.FM(nFactors=d, nEpochs=10, batchSize=256, lr=0.0, reg=0.0, optimizer=ctr.Adam, seed=1)
    m.Fit(train, test, Verbose=1, Patience=2)
    assert [e for e, _, _ in m.log()] == [0, 1, 2, 3]
    # a diverging lr: the first NaN cost ends the Fit
    m = ctr.FM(nFactors=d, nEpochs=10, batchSize=256, lr=1e30, reg=0.0, optimizer=ctr.SGD, seed=1)
    m.Fit(train, test, Verbose=1)
    lg = m.log()
    assert np.isnan(lg[-1][1]) and len(lg) < 11 and not any(np.isnan(c) for _, c, _ in lg[:-1])
    # cancel: Score{}
    m = ctr.FM(nFactors=d, nEpochs=5, batchSize=256, lr=0.01, optimizer=ctr.Adam, seed=1)
    s = m.Fit(train, test, Verbose=1, cancel=np.ones(1, np.int32))
    assert s == ctr.Score([0, 0, 0, 0]) and [e for e, _, _ in m.log()] == [0]


def test_error_paths():
    fm = capi.FM(10, 4)
    idx = np.array([[1, 2], [3, 10]], np.int32)
    val = np.ones((2, 2), f32)
    with pytest.raises(capi.GorseHipError) as e:
        fm.set_train(idx, val, np.ones(2, f32))
    assert e.value.code == capi.ERR_RANGE
    with pytest.raises(capi.GorseHipError) as e:
        fm.predict(idx, val)
    assert e.value.code == capi.ERR_RANGE
    with pytest.raises(capi.GorseHipError) as e:
        fm.predict(np.zeros((2, 0), np.int32), np.zeros((2, 0), f32))
    assert e.value.code == capi.ERR_INVALID
    with pytest.raises(capi.GorseHipError) as e:
        fm.set_train(np.zeros((2, 0), np.int32), np.zeros((2, 0), f32), np.ones(2, f32))
    assert e.value.code == capi.ERR_INVALID
    fm.set_train(idx % 10, val, np.ones(2, f32))
    with pytest.raises(capi.GorseHipError) as e:
        fm.epoch(0, capi.OPT_SGD, 0.1, 0.0)
    assert e.value.code == capi.ERR_INVALID
    with pytest.raises(capi.GorseHipError) as e:
        fm.epoch(2, 7, 0.1, 0.0)
    assert e.value.code == capi.ERR_INVALID
    assert np.isfinite(fm.epoch(2, capi.OPT_SGD, 0.1, 0.0))


def test_epoch_cancel_on_the_device_path():
    """gorse_fm_epoch itself sees a raised flag (before its first batch) and returns ERR_CANCELLED; the handle keeps working"""
    idx, val, tgt = R.synth_ctr(3000, 200, 8, seed=41)
    B, W, V = _model(200, 8, 42, sd=0.01)
    fm = capi.FM(200, 8)
    fm.set_params(B, W, V)
    fm.set_train(idx, val, tgt)
    flag = np.ones(1, np.int32)
    with pytest.raises(capi.GorseHipError) as e:
        fm.epoch(256, capi.OPT_ADAM, 0.01, 1e-4, cancel=flag)
    assert e.value.code == capi.ERR_CANCELLED
    gB, gW, gV = fm.get_params()  # cancelled before any step: nothing moved
    assert gB == B and np.array_equal(gW, W) and np.array_equal(gV, V)
    flag[0] = 0
    cost = fm.epoch(256, capi.OPT_ADAM, 0.01, 1e-4, cancel=flag)
    assert np.isfinite(cost) and cost > 0
    # the same handle, fresh: the epoch after the cancelled call is the first epoch of an untouched model
    ref = capi.FM(200, 8)
    ref.set_params(B, W, V)
    ref.set_train(idx, val, tgt)
    assert ref.epoch(256, capi.OPT_ADAM, 0.01, 1e-4) == cost
    assert np.array_equal(fm.predict(idx, val), ref.predict(idx, val))
