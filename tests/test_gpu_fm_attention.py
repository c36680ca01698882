"""The factorization machine's item-embedding branch on the MI355X (gorse_fm_* with embedding fields) against the numpy
restatement in fm_attention_ref.py, which indexes the Softmax's maxima and sums the way the reference does (flat index % n).
Bars are those of test_gpu_fm.py: 1e-5 of a row's scale for logits and parameters, 1e-4 relative for an epoch's cost, 0.005
for AUC.  The float32 restatement lies within a tenth of the logit bar of the float64 one on every scoring input (asserted), so
the reference's own rounding sits well inside the bar."""
import numpy as np
import pytest

import fm_attention_ref as A
import fm_ref as R
from gorse_amd import capi

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
BAR = 1e-5


def _model(nf, d, dims, seed, sd=0.3, h_sd=0.3, bias_sd=0.1):
    rng = np.random.default_rng(seed)
    B, W, V = f32(rng.normal(0, 0.5)), rng.normal(0, sd, nf).astype(f32), rng.normal(0, sd, (nf, d)).astype(f32)
    fields = []
    for D in dims:
        H, Wa, ba, We, be = A.init_field(rng, D, d, h_sd)
        fields.append((H, Wa, rng.normal(0, bias_sd, d).astype(f32), We, rng.normal(0, bias_sd, d).astype(f32)))
    return B, W, V, fields


def _embs(n, dims, seed, absent_every=7):
    rng = np.random.default_rng(seed)
    out = []
    for D in dims:
        e = rng.normal(0, 1, (n, D)).astype(f32)
        if absent_every:
            e[::absent_every] = 0  # samples without an embedding carry an all-zero row (fm.go:555-561)
        out.append(A.to_bf16(e))
    return out


def _handle(nf, d, dims, B, W, V, fields):
    fm = capi.FM(nf, d, embedding_dims=dims)
    fm.set_params(B, W, V)
    for k, fld in enumerate(fields):
        fm.set_embedding_params(k, *fld)
    return fm


def _rows(n, nf, seed, wmax=12):
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(n):
        k = int(rng.integers(1, wmax + 1))
        rows.append((rng.choice(nf, k, replace=False).astype(np.int32), rng.normal(0.5, 1.0, k).astype(f32)))
    return R.pad(rows, wmax + 2)


@pytest.mark.parametrize("d", [1, 16, 128])
@pytest.mark.parametrize("dims,batch_sizes", [((3, 4), (5, 2, 12)), ((768,), (64, 50)), ((1536, 64), (64, 37))])
def test_scoring_parity(d, dims, batch_sizes):
    """batch lengths that divide D and that do not, a partial last batch (157 rows), absent embeddings"""
    nf, n = 300, 157
    idx, val = _rows(n, nf, d + len(dims))
    B, W, V, fields = _model(nf, d, dims, 100 + d)
    embs = _embs(n, dims, 200 + d)
    fm = _handle(nf, d, dims, B, W, V, fields)
    for bs in batch_sizes:
        want, scale = A.predict(B, W, V, fields, idx, val, embs, bs)
        w32, _ = A.predict(B, W, V, fields, idx, val, embs, bs, dtype=f32)
        assert np.all(np.abs(w32 - want) <= 0.1 * BAR * scale), ("the restatement's own fp32 error", bs)
        got = fm.predict_embeddings(idx, val, embs, bs)
        err = np.max(np.abs(got - want) / scale)
        print("d %d dims %s bs %d: max err / scale %.3g" % (d, dims, bs, err))
        assert np.all(np.abs(got - want) <= BAR * scale + 1e-30), (bs, err)
    # the branch is in the result at all
    plain = R.forward64(B, W, V, idx, val)[0]
    assert np.max(np.abs(want - plain) / scale) > 100 * BAR


def test_softmax_indexing_is_the_reference_s():
    nf, d, dims, n = 200, 16, (64,), 96
    idx, val = _rows(n, nf, 3)
    B, W, V, fields = _model(nf, d, dims, 5, h_sd=1.0)
    embs = _embs(n, dims, 6)
    fm = _handle(nf, d, dims, B, W, V, fields)
    outs = {}
    for bs in (32, 48):
        want, scale = A.predict(B, W, V, fields, idx, val, embs, bs)
        usual, _ = A.predict(B, W, V, fields, idx, val, embs, bs, softmax=A.row_softmax)
        assert np.max(np.abs(want - usual) / scale) >= 100 * BAR  # the two softmaxes are far apart on this input
        got = fm.predict_embeddings(idx, val, embs, bs)
        assert np.all(np.abs(got - want) <= BAR * scale), np.max(np.abs(got - want) / scale)
        assert np.max(np.abs(got - usual) / scale) >= 50 * BAR
        outs[bs] = (got, want, scale)
    # the batch length is part of the result, on the device as in the restatement
    assert np.max(np.abs(outs[32][1] - outs[48][1]) / outs[32][2]) >= 100 * BAR
    assert np.max(np.abs(outs[32][0] - outs[48][0]) / outs[32][2]) >= 50 * BAR


def _one_step_inputs(zero_embeddings):
    # tensor lengths with a non-empty FMA body and a non-empty tail: ba, be 21 = 16 + 5; H, Wa, We 21 x 5 = 96 + 9 and 21 x 9 = 176 + 13
    nf, d, dims, n = 203, 21, (5, 9), 64
    rng = np.random.default_rng(11)
    rows = [(rng.choice(150, int(rng.integers(1, 7)), replace=False).astype(np.int32), rng.normal(1, 0.5, 6).astype(f32))
            for _ in range(n)]
    idx, val = R.pad([(a, b[:len(a)]) for a, b in rows], 6)
    tgt = np.where(rng.random(n) < 0.5, 1, -1).astype(f32)
    B, W, V, fields = _model(nf, d, dims, 12, sd=0.2)
    embs = _embs(n, dims, 13)
    if zero_embeddings:
        embs = [np.zeros_like(e) for e in embs]
    return nf, d, dims, n, idx, val, tgt, B, W, V, fields, embs


@pytest.mark.parametrize("adam", [False, True])
def test_one_step_parity(adam):
    nf, d, dims, n, idx, val, tgt, B, W, V, fields, embs = _one_step_inputs(False)
    lr, wd = (0.01, 0.01) if adam else (0.05, 0.01)
    fm = _handle(nf, d, dims, B, W, V, fields)
    fm.set_train(idx, val, tgt)
    for k, e in enumerate(embs):
        fm.set_train_embeddings(k, e)
    cost = fm.epoch(n, capi.OPT_ADAM if adam else capi.OPT_SGD, lr, wd)
    ref = A.Trainer(B, W, V, fields)
    loss = ref.step(idx, val, embs, tgt, adam, lr, wd)
    assert abs(cost - loss) <= 1e-5 * loss
    gB, gW, gV = fm.get_params()
    rB, rW, rV = ref.params
    # V's touched rows carry g * sum enc: the plain machine's step is far from the restated one there
    plain = R.Trainer(B, W, V)
    plain.epoch(idx, val, tgt, n, adam, lr, wd)
    if not adam:
        assert np.max(np.abs(plain.params[2] - rV)) > 100 * BAR * lr
    named = [("B", np.array([gB]), np.array([rB])), ("W", gW, rW), ("V", gV, rV)]
    for k in range(len(dims)):
        got = fm.get_embedding_params(k)
        for name, g_, r_, p0 in zip(A.NAMES, got, ref.fields[k], fields[k]):
            named.append(("%s[%d]" % (name, k), g_, r_))
            assert not np.array_equal(r_, p0), name  # every tensor of the branch moves
    for name, g_, r_ in named:
        g_, r_ = np.asarray(g_, f64).reshape(-1), np.asarray(r_, f64).reshape(-1)
        tol = BAR * (np.abs(r_) + lr)
        worst = np.max(np.abs(g_ - r_) / tol)
        print("%s %s: worst error / bar %.3g" % ("adam" if adam else "sgd", name, worst))
        assert np.all(np.abs(g_ - r_) <= tol), (name, worst)


@pytest.mark.parametrize("adam", [False, True])
def test_zero_embeddings_leave_a_zero_gradient(adam):
    """all rows without an embedding: H, Wa, ba, We get exactly zero gradient (the dense step with g = 0, bit for bit, FMA body
    and unfused tail), be still moves"""
    nf, d, dims, n, idx, val, tgt, B, W, V, fields, embs = _one_step_inputs(True)
    lr, wd = (0.01, 0.01) if adam else (0.05, 0.01)
    fm = _handle(nf, d, dims, B, W, V, fields)
    fm.set_train(idx, val, tgt)
    for k, e in enumerate(embs):
        fm.set_train_embeddings(k, e)
    fm.epoch(n, capi.OPT_ADAM if adam else capi.OPT_SGD, lr, wd)
    lr_t = R.adam_lr(lr, 1) if adam else f32(lr)
    for k in range(len(dims)):
        got = fm.get_embedding_params(k)
        for name, g_, p0 in zip(A.NAMES, got, fields[k]):
            L = p0.size
            assert L % 16 != 0 and L > 16, name
            zero = np.zeros(L, f32)
            still = R.opt_step32(p0, zero, zero, zero, wd, lr_t, adam)[0]
            same = np.array_equal(g_.reshape(-1).view(np.uint32), still.view(np.uint32))
            if name == "be":
                assert not same
            else:
                assert same, (name, k)


def _train_set(n, nf, d, dims, seed):
    idx, val, tgt = R.synth_ctr(n, nf, d, seed=seed)
    return idx, val, tgt, _embs(n, dims, seed + 1000, absent_every=11)


def test_determinism():
    nf, d, dims = 300, 16, (64, 40)
    idx, val, tgt, embs = _train_set(6000, nf, 8, dims, 4)
    idx[:, 0], val[:, 0] = 7, 1.0
    B, W, V, fields = _model(nf, d, dims, 5, sd=0.01)
    runs = []
    for _ in range(2):
        fm = _handle(nf, d, dims, B, W, V, fields)
        fm.set_train(idx, val, tgt)
        for k, e in enumerate(embs):
            fm.set_train_embeddings(k, e)
        costs = [fm.epoch(512, capi.OPT_ADAM, 0.01, 1e-4) for _ in range(3)]
        out = [np.array(costs, f32)] + [np.asarray(x) for x in fm.get_params()]
        for k in range(len(dims)):
            out += list(fm.get_embedding_params(k))
        runs.append(out)
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(np.asarray(a, f32).view(np.uint32), np.asarray(b, f32).view(np.uint32))
    assert not np.array_equal(runs[0][-2], fields[-1][3])  # We of the last field was trained


@pytest.mark.parametrize("adam", [True, False])
def test_training_parity(adam):
    nf, d, dims = 2000, 8, (64, 256)
    idx, val, tgt, embs = _train_set(20000 + 500, nf, d, dims, 21)  # 20 batches of 1024, the last one partial
    tidx, tval, ttgt, tembs = _train_set(4000, nf, d, dims, 22)
    rng = np.random.default_rng(23)
    B, W, V = f32(0), rng.normal(0, 0.01, nf).astype(f32), rng.normal(0, 0.01, (nf, d)).astype(f32)
    fields = [A.init_field(rng, D, d) for D in dims]
    lr, wd = (0.01, 1e-4) if adam else (0.1, 1e-4)
    fm = _handle(nf, d, dims, B, W, V, fields)
    fm.set_train(idx, val, tgt)
    for k, e in enumerate(embs):
        fm.set_train_embeddings(k, e)
    ref = A.Trainer(B, W, V, fields)
    costs = []
    for ep in range(10):
        c_dev = fm.epoch(1024, capi.OPT_ADAM if adam else capi.OPT_SGD, lr, wd)
        c_ref = ref.epoch(idx, val, embs, tgt, 1024, adam, lr, wd)
        print("epoch %d cost device %.7g restated %.7g rel %.3g" % (ep, c_dev, c_ref, abs(c_dev - c_ref) / abs(c_ref)))
        assert abs(c_dev - c_ref) <= 1e-4 * abs(c_ref), (c_dev, c_ref)
        costs.append(c_dev)
    pos, neg = ttgt > 0, ttgt <= 0
    p_dev = fm.predict_embeddings(tidx, tval, tembs, 1024)
    p_ref = A.predict(*ref.params, ref.fields, tidx, tval, tembs, 1024)[0]
    a_dev, a_ref = R.auc(p_dev[pos], p_dev[neg]), R.auc(p_ref[pos], p_ref[neg])
    print("AUC device %.5f restated %.5f" % (a_dev, a_ref))
    assert abs(a_dev - a_ref) <= 0.005
    assert costs[-1] < costs[0]


def test_error_paths():
    for dims in ((0,), (4097,), (4,) * 9):
        with pytest.raises(capi.GorseHipError) as e:
            capi.FM(10, 4, embedding_dims=dims)
        assert e.value.code == capi.ERR_INVALID
    fm = capi.FM(10, 4, embedding_dims=(3, 4096))
    idx = np.array([[1, 2], [3, 9]], np.int32)
    val = np.ones((2, 2), f32)
    one = np.zeros(4, f32)
    fp = capi._p(one, capi._f32p)
    for field in (-1, 2):
        assert capi.lib().gorse_fm_set_embedding_params(fm.h, field, fp, fp, fp, fp, fp) == capi.ERR_INVALID
        assert capi.lib().gorse_fm_get_embedding_params(fm.h, field, None, None, None, None, None) == capi.ERR_INVALID
        assert capi.lib().gorse_fm_set_train_embeddings(fm.h, field, capi._p(np.zeros(8, np.uint16), capi.C.POINTER(capi.C.c_uint16))) \
            == capi.ERR_INVALID
    with pytest.raises(capi.GorseHipError) as e:  # no training set yet
        fm.set_train_embeddings(0, np.zeros((2, 3), np.uint16))
    assert e.value.code == capi.ERR_INVALID
    with pytest.raises(capi.GorseHipError) as e:  # a handle with fields is not scored without embeddings
        fm.predict(idx, val)
    assert e.value.code == capi.ERR_INVALID
    fm.set_train(idx, val, np.ones(2, f32))
    fm.set_train_embeddings(0, np.zeros((2, 3), np.uint16))
    with pytest.raises(capi.GorseHipError) as e:  # field 1 has no training embeddings
        fm.epoch(2, capi.OPT_SGD, 0.1, 0.0)
    assert e.value.code == capi.ERR_INVALID
    fm.set_train_embeddings(1, np.zeros((2, 4096), np.uint16))
    assert np.isfinite(fm.epoch(2, capi.OPT_SGD, 0.1, 0.0))
    fm.set_train(idx, val, np.ones(2, f32))  # a new training set drops the old set's embeddings
    with pytest.raises(capi.GorseHipError) as e:
        fm.epoch(2, capi.OPT_SGD, 0.1, 0.0)
    assert e.value.code == capi.ERR_INVALID
    with pytest.raises(capi.GorseHipError) as e:
        fm.predict_embeddings(idx, val, [np.zeros((2, 3), np.uint16), np.zeros((2, 4096), np.uint16)], 0)
    assert e.value.code == capi.ERR_INVALID
    fm.set_embedding_dims(())  # back to the plain machine
    assert np.isfinite(fm.epoch(2, capi.OPT_SGD, 0.1, 0.0))
    assert np.all(np.isfinite(fm.predict(idx, val)))


def test_cancel_with_the_branch_active():
    nf, d, dims = 200, 8, (32,)
    idx, val, tgt, embs = _train_set(3000, nf, d, dims, 41)
    B, W, V, fields = _model(nf, d, dims, 42, sd=0.01)

    def fresh():
        fm = _handle(nf, d, dims, B, W, V, fields)
        fm.set_train(idx, val, tgt)
        fm.set_train_embeddings(0, embs[0])
        return fm

    fm = fresh()
    flag = np.ones(1, np.int32)
    with pytest.raises(capi.GorseHipError) as e:
        fm.epoch(8, capi.OPT_ADAM, 0.01, 1e-4, cancel=flag)  # 375 steps: more than the in-flight window
    assert e.value.code == capi.ERR_CANCELLED
    assert np.array_equal(fm.get_params()[2], V)  # seen before the first batch: nothing moved
    for got, p0 in zip(fm.get_embedding_params(0), fields[0]):
        assert np.array_equal(got, p0)
    flag[0] = 0
    cost = fm.epoch(256, capi.OPT_ADAM, 0.01, 1e-4, cancel=flag)
    ref = fresh()
    assert ref.epoch(256, capi.OPT_ADAM, 0.01, 1e-4) == cost
    assert np.array_equal(fm.predict_embeddings(idx, val, embs, 256), ref.predict_embeddings(idx, val, embs, 256))


def test_a_handle_without_fields_is_unchanged():
    idx, val, tgt = R.synth_ctr(3000, 300, 8, seed=4)
    rng = np.random.default_rng(5)
    B, W, V = f32(0.1), rng.normal(0, 0.01, 300).astype(f32), rng.normal(0, 0.01, (300, 16)).astype(f32)
    outs = []
    for configure in (False, True, "after fields"):
        fm = capi.FM(300, 16)
        if configure == "after fields":
            fm.set_embedding_dims((12, 5))
        if configure:
            fm.set_embedding_dims(())
        fm.set_params(B, W, V)
        fm.set_train(idx, val, tgt)
        cost = fm.epoch(1000, capi.OPT_ADAM, 0.01, 1e-4)  # three Adam steps
        outs.append((np.array([cost], f32),) + tuple(np.asarray(x, f32) for x in fm.get_params()) + (fm.predict(idx, val),))
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _planted(n, nf, d, D, seed):
    """labels that depend on the embedding alone: a logistic draw around 2.5 u.x / sqrt(D)"""
    idx, val, _ = R.synth_ctr(n, nf, d, seed=seed)
    idx[:, 0], val[:, 0] = 0, 1.0  # a feature every row carries: vx has a common part the branch can use
    rng = np.random.default_rng(seed + 500)
    bits = A.to_bf16(rng.normal(0, 1, (n, D)).astype(f32))
    u = np.random.default_rng(77).normal(0, 1, D)
    logit = 2.5 * (A.from_bf16(bits) @ u) / np.sqrt(D)
    tgt = np.where(rng.random(n) < 1 / (1 + np.exp(-logit)), 1.0, -1.0).astype(f32)
    return idx, val, tgt, [bits]


def _dataset(idx, val, tgt, embs, nf):
    from gorse_amd import ctr
    lens = (val != 0).sum(1)
    indptr = np.concatenate([[0], np.cumsum(lens)])
    ii = np.concatenate([idx[i][val[i] != 0] for i in range(len(lens))])
    vv = np.concatenate([val[i][val[i] != 0] for i in range(len(lens))])
    ds = ctr.Dataset(nf, (indptr, ii, vv, tgt))
    if embs:
        ds.set_embeddings(embs)
    return ds


def test_host_twin_fit_with_embeddings():
    from gorse_amd import ctr
    nf, d, D = 100, 8, 16
    tr, te = _planted(4000, nf, d, D, 31), _planted(1000, nf, d, D, 32)
    # what the restatement reaches with and without the embeddings (its own draw of the initial tensors)
    aucs = []
    for with_emb in (True, False):
        rng = np.random.default_rng(1)
        B, W, V = f32(0), rng.normal(0, 0.01, nf).astype(f32), rng.normal(0, 0.01, (nf, d)).astype(f32)
        T = A.Trainer(B, W, V, [A.init_field(rng, D, d)] if with_emb else [])
        for _ in range(12):
            T.epoch(tr[0], tr[1], tr[3] if with_emb else [], tr[2], 256, True, 0.003, 1e-4)
        p = A.predict(*T.params, T.fields, te[0], te[1], te[3] if with_emb else [], 256)[0]
        aucs.append(R.auc(p[te[2] > 0], p[te[2] <= 0]))
    margin = (aucs[0] - aucs[1]) / 2
    assert margin > 0.05, aucs  # the signal is planted in the embeddings
    train, test = _dataset(*tr, nf), _dataset(*te, nf)
    # lr 0.003: at 0.01 this model diverges within twenty epochs for some initial draws (the wrapped Softmax subtracts another
    # row's maximum), which would make the margin a matter of the draw
    m = ctr.FM(nFactors=d, nEpochs=12, batchSize=256, lr=0.003, reg=1e-4, optimizer=ctr.Adam, seed=1)
    s = m.Fit(train, test, Verbose=5)
    lg = m.log()
    assert [e for e, _, _ in lg] == [0, 5, 10, 12]  # epoch 0, every Verbose epochs, the last epoch (fm.go:360-416)
    assert lg[0][1] == 0 and all(c > 0 for _, c, _ in lg[1:])
    assert s.AUC == lg[-1][2] and s == m.Evaluate(test)
    H, Wa, ba, We, be = m.field_params(0)
    assert H.shape == (d, D) and np.abs(We).max() > 0 and np.abs(be).max() > 0 and np.abs(ba).max() > 0
    plain = ctr.FM(nFactors=d, nEpochs=12, batchSize=256, lr=0.003, reg=1e-4, optimizer=ctr.Adam, seed=1)
    s0 = plain.Fit(_dataset(*tr[:3], None, nf), _dataset(*te[:3], None, nf), Verbose=5)
    print("AUC with embeddings %.4f, withheld %.4f; restated %.4f / %.4f" % (s.AUC, s0.AUC, aucs[0], aucs[1]))
    assert s.AUC - s0.AUC >= margin
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
