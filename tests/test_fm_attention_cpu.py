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
