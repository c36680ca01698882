"""CPU checks of the item-embedding branch's yardstick (fm_attention_ref.py): the vectorised restatement of the reference's
Softmax against a loop-by-loop transcription, the restated gradients against finite differences where that Softmax is a true
softmax (n = 1), and the new entry points' behaviour without a device."""
import ctypes as C

import numpy as np
import pytest

import fm_attention_ref as A
import fm_ref as R

f32, f64 = np.float32, np.float64


@pytest.mark.parametrize("n,D", [(4, 6), (5, 3), (7, 10), (3, 6), (4, 4), (2, 8), (1, 7)])  # n does not divide D, n | D, n = 1
def test_vectorised_softmax_equals_the_literal_transcription(n, D):
    rng = np.random.default_rng(n * 100 + D)
    s = rng.normal(0, 1.5, (n, D)).astype(f32)
    da = rng.normal(0, 1, (n, D)).astype(f32)
    a = A.softmax_fwd(s)
    assert a.dtype == f32
    assert np.array_equal(a.view(np.uint32), A.softmax_fwd_literal(s).view(np.uint32))
    ds = A.softmax_bwd(a, da)
    assert ds.dtype == f32
    assert np.array_equal(ds.view(np.uint32), A.softmax_bwd_literal(a, da).view(np.uint32))


def test_reference_softmax_is_a_row_softmax_only_for_one_row():
    rng = np.random.default_rng(1)
    s = rng.normal(0, 1, (1, 9))
    assert np.allclose(A.softmax_fwd(s), A.row_softmax(s), rtol=1e-14, atol=0)
    s = rng.normal(0, 1, (6, 9))
    a = A.softmax_fwd(s)
    assert np.abs(a - A.row_softmax(s)).max() > 1e-2
    assert np.abs(a.sum(1) - 1).max() > 1e-2  # its rows do not sum to one
    # element (r, c) uses row (r D + c) % n's maximum and sum
    e = np.exp(s - s.max(1)[A.wrap_index(6, 9)])
    assert np.allclose(a[2, 5], e[2, 5] / e[(2 * 9 + 5) % 6].sum(), rtol=1e-14)


def test_bf16_round_trip():
    x = np.array([0.0, 1.0, -2.5, 0.1, 3.14159, 1e-3, 1 + 2 ** -8, 1 + 3 * 2 ** -9], f32)
    b = A.to_bf16(x)
    back = A.from_bf16(b, f32)
    assert np.all(np.abs(back - x) <= np.abs(x) * 2 ** -8)
    assert np.array_equal(A.to_bf16(back), b)
    assert back[6] == 1.0 and back[7] == f32(1 + 2 ** -7)  # ties to even, both ways


def _small_model(rng, nf, d, dims):
    B, W, V = 0.3, rng.normal(0, 0.5, nf), rng.normal(0, 0.5, (nf, d))
    fields = []
    for D in dims:
        fields.append((rng.normal(0, 0.7, (d, D)), rng.normal(0, 0.6, (D, d)), rng.normal(0.5, 0.3, d),
                       rng.normal(0, 0.6, (D, d)), rng.normal(0, 0.3, d)))
    return B, W, V, fields


def test_restated_gradients_match_finite_differences_for_one_row():
    """at n = 1 the reference's Softmax is the usual one, so the restated backward must be the loss's true gradient"""
    rng = np.random.default_rng(12)
    nf, d, dims = 9, 4, (3, 4)
    B, W, V, fields = _small_model(rng, nf, d, dims)
    idx, val = R.pad([(np.array([0, 2, 5]), np.array([1.5, -0.5, 0.8]))], 5)
    val = val.astype(f64)
    embs = [A.to_bf16(rng.normal(0, 1, (1, D))) for D in dims]
    t = np.array([1.0])
    dB, dW, dV, fg, _ = A.grads(B, W, V, fields, idx, val, embs, t)
    h = 1e-6

    def L(B_=B, W_=W, V_=V, F_=fields):
        return A.loss(B_, W_, V_, F_, idx, val, embs, t)

    assert abs((L(B_=B + h) - L(B_=B - h)) / (2 * h) - dB) < 1e-7
    for i in range(nf):
        e = np.zeros(nf)
        e[i] = h
        assert abs((L(W_=W + e) - L(W_=W - e)) / (2 * h) - dW[i]) < 1e-7
        for f in range(d):
            E = np.zeros((nf, d))
            E[i, f] = h
            assert abs((L(V_=V + E) - L(V_=V - E)) / (2 * h) - dV[i, f]) < 1e-7
    assert np.abs(dV[[0, 2, 5]]).min() > 1e-4  # the rows in use carry a gradient worth checking
    for k, fld in enumerate(fields):
        for ti, tensor in enumerate(fld):
            assert np.abs(fg[k][ti]).max() > 1e-5, (k, A.NAMES[ti])
            for pos in np.ndindex(tensor.shape):
                def moved(delta):
                    t2 = tensor.copy()
                    t2[pos] += delta
                    f2 = list(fields)
                    f2[k] = fld[:ti] + (t2,) + fld[ti + 1:]
                    return f2
                num = (L(F_=moved(h)) - L(F_=moved(-h))) / (2 * h)
                assert abs(num - fg[k][ti][pos]) < 1e-7, (k, A.NAMES[ti], pos, num, fg[k][ti][pos])


def test_trainer_without_fields_is_the_plain_trainer():
    idx, val, tgt = R.synth_ctr(300, 40, 4, seed=3)
    rng = np.random.default_rng(4)
    B, W, V = f32(0), rng.normal(0, 0.01, 40).astype(f32), rng.normal(0, 0.01, (40, 4)).astype(f32)
    a, b = A.Trainer(B, W, V, []), R.Trainer(B, W, V)
    for _ in range(2):
        assert a.epoch(idx, val, [], tgt, 128, True, 0.01, 1e-4) == b.epoch(idx, val, tgt, 128, True, 0.01, 1e-4)
    for x, y in zip(a.params, b.params):
        assert np.array_equal(np.asarray(x), np.asarray(y))


NEW_SYMBOLS = ("gorse_fm_set_embedding_dims", "gorse_fm_set_embedding_params", "gorse_fm_get_embedding_params",
               "gorse_fm_set_train_embeddings", "gorse_fm_predict_embeddings")


def test_new_symbols_are_exported_and_declared():
    from gorse_amd import capi
    L = C.CDLL(capi.LIB_PATH)
    for n in NEW_SYMBOLS:
        assert hasattr(L, n), n
        assert n in capi.SIGNATURES, n


def test_new_entry_points_validate_a_null_handle():
    from gorse_amd import capi
    L = capi.lib()
    dims = np.array([3, 4], np.int32)
    one = np.zeros(4, f32)
    fp = one.ctypes.data_as(C.POINTER(C.c_float))
    assert L.gorse_fm_set_embedding_dims(None, 2, dims.ctypes.data_as(C.POINTER(C.c_int32))) == capi.ERR_INVALID
    assert L.gorse_fm_set_embedding_params(None, 0, fp, fp, fp, fp, fp) == capi.ERR_INVALID
    assert L.gorse_fm_get_embedding_params(None, 0, fp, fp, fp, fp, fp) == capi.ERR_INVALID
    assert L.gorse_fm_set_train_embeddings(None, 0, None) == capi.ERR_INVALID
    assert L.gorse_fm_predict_embeddings(None, 0, 1, None, None, None, 1, None) == capi.ERR_INVALID
    assert b"handle is NULL" in L.gorse_hip_last_error()


def test_fm_with_embedding_fields_needs_a_device():
    """without a GPU the handle cannot exist (no CPU path); with one, the caps are enforced"""
    from gorse_amd import capi
    if capi.device_count() == 0:
        with pytest.raises(capi.GorseHipError) as e:
            capi.FM(10, 8, embedding_dims=(3, 4))
        assert e.value.code == capi.ERR_NO_DEVICE
        return
    for dims in ((0,), (4097,), (4,) * 9):
        with pytest.raises(capi.GorseHipError) as e:
            capi.FM(10, 8, embedding_dims=dims)
        assert e.value.code == capi.ERR_INVALID
    assert capi.FM(10, 8, embedding_dims=(4096,) + (4,) * 7).dims[0] == 4096


# ---- the bars of test_gpu_fm_attention_shapes.py, checked on its own inputs ------------------------------------------------------
_CASES = {}


def _case(c):
    if c not in _CASES:
        _CASES[c] = A.case(*c)
    return _CASES[c]


def _report_of(c, adam, dtype=f64, fault=None):
    B, W, V, fields, idx, val, tgt, embs = _case(c)
    lr, wd = A.rates(adam)
    got, loss = A.ref_step(B, W, V, fields, idx, val, embs, tgt, adam, lr, wd, dtype, fault)
    return A.one_step_report(B, W, V, fields, idx, val, embs, tgt, got, loss, adam, lr, wd)


def test_one_step_inputs_are_what_the_gpu_tests_promise():
    assert len(set(A.ONE_STEP)) == len(A.ONE_STEP) == 28
    B, W, V, fields, idx, val, tgt, embs = _case(A.BASE)
    c = A.forward(B, W, V, fields, idx, val, embs)[3][0]
    assert (c["pre"] > 0).any(0).all() and (c["pre"] < 0).any()  # both signs of pre; every relu opens in some row
    assert np.all(A.from_bf16(embs[0])[4] == 0) and np.abs(A.from_bf16(embs[0])[3]).min() > 0
    assert np.abs(fields[0][2]).min() > 0 and np.abs(fields[0][4]).min() > 0 and fields[0][0].std() > 0.25
    a = c["a"]
    assert a.max() > 20 * a.min()  # far from the uniform softmax


def test_headroom_of_the_one_step_bars():
    """the fp32 restatement of the gradients against the float64 one, through the same report the device is held to: at most
    half of every bar; and the share of Adam's ill-conditioned elements, which depends on the reference alone"""
    worst, share = {}, {}
    for adam in (False, True):
        for c in A.ONE_STEP:
            rep = _report_of(c, adam, f32)
            assert not rep["still"], (c, rep["still"])
            for k, v in rep.items():
                if k.endswith("_zero"):
                    assert v[0] == 0 and v[1] == 0, (c, k, v)  # a zero gradient is zero in fp32 too
                elif k.endswith("_ill"):
                    worst[("ill", adam)] = max(worst.get(("ill", adam), 0), v[2])
                elif k == "ill":
                    share[c] = v[0] / v[1]
                    assert share[c] <= 0.05, (c, v)
                elif k != "still":
                    kind = "cost" if k == "cost" else "carried" if k[0] == "g" else "param"
                    worst[(kind, adam)] = max(worst.get((kind, adam), 0), v)
    top = max(share, key=share.get)
    print("fp32 restatement, worst error over bar:", {k: float("%.3g" % v) for k, v in worst.items()})
    print("largest share of ill-conditioned elements %.4f at %s" % (share[top], top))
    assert max(worst.values()) <= 0.5, worst
    assert set(worst) == set(A.HEADROOM)
    for k, v in worst.items():  # the recorded figures are the measured ones, rounded up
        assert A.HEADROOM[k] / 2 <= v <= A.HEADROOM[k], (k, v)
    assert 2 * share[top] <= A.ILL_SHARE, (share[top], top)


def _one_step_faults(c):
    d, dims, n = c
    out = [("lost_row", n - 1), ("no_bias", "be"), ("lost_col", max(dims) - 1)]
    if max(dims) > 1:  # at D = 1 the softmax is 1 whatever s is: ds, dpre, dH, dWa and dba are exactly zero, nothing to lose
        out += [("no_bias", "ba"), ("no_relu", None)]
    if n > 1:
        out.append(("lost_row", -(-n // 8)))  # the first row of segment 1
        if max(dims) > 1:
            out.append(("row_softmax", None))
    if max(dims) > 64:
        out.append(("lost_col", 64))
    if len(dims) > 1:
        out += [("esum_first", None)] + [("shared_gx", k) for k in range(1, min(len(dims), 3))]
    return out


def test_every_planted_fault_is_ten_bars_out():
    """one SGD step (the carried gradient is what sees a gradient that is merely a little off, as in the plain machine's
    test); the weakest case of every fault is printed"""
    weakest = {}
    for c in A.ONE_STEP:
        for fault in _one_step_faults(c):
            r = A.worst(_report_of(c, False, f64, fault))
            key = fault[0] + (" " + fault[1] if fault[0] == "no_bias" else "")
            if key not in weakest or r < weakest[key][0]:
                weakest[key] = (r, c, fault)
            assert r >= 10, (c, fault, r)
    for k, v in weakest.items():
        print("fault %-12s weakest at (d, dims, n) = %s %s: %.3g bars" % (k, v[1], v[2], v[0]))
    assert {k.split()[0] for k in weakest} == {"row_softmax", "lost_row", "no_bias", "no_relu", "lost_col", "esum_first", "shared_gx"}


def test_adam_sees_the_faults_that_change_a_sign():
    """Adam's first step keeps the sign of grad + wd p and little of its size: a gradient set to zero or formed from another
    field's buffer fails it at once, a lost row shows from the second step on (the multi-step test)"""
    for c in ((20, (129, 5, 64), 13), A.BASE):
        for fault in _one_step_faults(c):
            if fault[0] in ("no_bias", "shared_gx", "lost_col", "no_relu"):
                r = A.worst(_report_of(c, True, f64, fault))
                assert r >= 10, (c, fault, r)


def _schedules():
    """(name, d, dims, [(idx, val, tgt, embs, bs, restart)] per epoch) of every multi-step and life-cycle case"""
    out = []
    for d, dims in A.MULTI:
        data = A.rows(A.MULTI_N, dims, 7 + d)
        out.append(("multi d=%d" % d, d, dims, [(data, A.MULTI_BS, False)] * 3))
    d, dims = A.LIFE
    S, S2 = A.rows(45, dims, 71), A.rows(40, dims, 72)
    out.append(("life cycle", d, dims, [(data, bs, fit) for _, data, bs, _, fit in A.life_stages(S, S2)]))
    return out


@pytest.mark.parametrize("adam", [False, True])
def test_multi_step_divergence_scale_and_the_partial_batch_modulus(adam):
    K = A.K_MULTI[adam]
    worst = 0.0
    for name, d, dims, epochs in _schedules():
        lr, wd = A.rates(adam, d)
        B, W, V, fields = A.model(d, dims, 5 + d)
        a, b = A.StepTrainer(B, W, V, fields), A.StepTrainer(B, W, V, fields, dtype=f64)
        bad = A.StepTrainer(B, W, V, fields)
        first = None
        for e, ((idx, val, tgt, embs), bs, fit) in enumerate(epochs):
            if fit:
                B, W, V, fields = A.model(d, dims, 6 + d)
                a, b = A.StepTrainer(B, W, V, fields), A.StepTrainer(B, W, V, fields, dtype=f64)
            for i in range(0, len(tgt), bs):
                sl = slice(i, i + bs)
                for t in (a, b):
                    t.step(idx[sl], val[sl], [x[sl] for x in embs], tgt[sl], adam, lr, wd)
                first = first or a.max_scale
                dv = A.divergence(a.p, b.p, lr)
                assert np.isfinite(dv) and all(np.all(np.isfinite(x)) for x in a.p)
                if dv > worst:
                    worst, where = dv, (name, e, i)
            if name.startswith("multi"):
                # the wrapped modulus taken from the full batch size: only the partial last batch differs
                bad.epoch(idx, val, embs, tgt, bs, adam, lr, wd, fault=("full_modulus", None) if e == 0 else None)
                if e == 0:
                    r = A.params_report(bad.p, a.p, lr, K, a.slack if adam else None)
                    print("%s %s: full-batch modulus in the partial batch, bars out %s" % (name, "adam" if adam else "sgd",
                                                                                        {k: float("%.3g" % v) for k, v in r.items()}))
                    assert max(r.values()) >= 10, r
        # the wrapped softmax subtracts another row's maximum and can run away: here it does not
        print("%s %s: logit scale %.3g at the first step, %.3g at most" % (name, "adam" if adam else "sgd", first, a.max_scale))
        assert a.max_scale <= A.SCALE_GROWTH * first
    print("%s: largest divergence of the fp32-step reference from the float64 twin %.3g at %s" % ("adam" if adam else "sgd", worst, where))
    assert worst <= A.DIVERGENCE[adam], (worst, where)
    assert worst >= A.DIVERGENCE[adam] / 2  # the recorded value is the measured one, rounded up
