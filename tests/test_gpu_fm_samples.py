"""gorse_fm_set_train_samples / gorse_fm_set_test_samples on the MI355X: training and evaluating the FM ranker from
(user, item) samples and the resident item catalogue.

The yardstick is the padded route on the rows this file materialises itself with numpy (fm_samples_ref.World.materialise: the
composed rows, zero-padded, the embeddings gathered per sample): every bit must agree -- each epoch's cost, B, W, V and every
field tensor, the seven counts, auc_sum and the logits -- because the operation order is the same by contract.  No tolerance.
One case is independent of the device's padded route: a single SGD and a single Adam step from the sample route alone against
fm_ref / fm_attention_ref's float64 gradients, with those modules' own bars (every ratio of one_step_report <= 1, ILL_SHARE).

The small world (fm_samples_ref.World): 37 users, 23 items, 150 samples, batch 64 (the last batch holds 22 rows); a user with no
entries, an item with an empty row, lead 0 and 1 mixed, zero-valued entries, an item whose embedding row is all zero, a feature
on both sides of one row, one label on every user (64 positions of one feature in a batch) and items repeated inside a batch."""
import numpy as np
import pytest

import fm_attention_ref as A
import fm_ref as R
import fm_samples_ref as S
from gorse_amd import capi

pytestmark = pytest.mark.gpu
f32, u32 = np.float32, np.uint32
_WORLDS = {}


def _world(dims):
    if dims not in _WORLDS:
        _WORLDS[dims] = S.World(dims)
    return _WORLDS[dims]


def _model(d, dims, seed):
    """fm_attention_ref.model's recipe (it needs at least one field)"""
    rng = np.random.default_rng(seed)
    B, W, V = f32(rng.normal(0, 0.5)), rng.normal(0, 0.2, S.NF).astype(f32), rng.normal(0, 0.2, (S.NF, d)).astype(f32)
    fields = []
    for D in dims:
        H, Wa, _, We, _ = A.init_field(rng, D, d, 0.3)
        fields.append((H, Wa, rng.normal(0, 0.1, d).astype(f32), We, rng.normal(0, 0.1, d).astype(f32)))
    return B, W, V, fields


def _handle(d, dims, model):
    fm = capi.FM(S.NF, d, embedding_dims=dims)
    _set(fm, model)
    return fm


def _set(fm, model):
    B, W, V, fields = model
    fm.set_params(B, W, V)
    for k, fld in enumerate(fields):
        fm.set_embedding_params(k, *fld)


def _load_padded(fm, w, extra=0):
    idx, val, tgt, embs = w.materialise(extra)
    fm.set_train(idx, val, tgt)
    for k, e in enumerate(embs):
        fm.set_train_embeddings(k, e)


def _set_items(fm, w):
    fm.set_items(*w.item_csr(), lead=w.ilead, embs=w.embs)


def _load_samples(fm, w, items=True):
    if items:
        _set_items(fm, w)
    fm.set_train_samples(*w.user_csr(), w.user, w.item, w.target, user_lead=w.ulead)


def _read(fm):
    return A.flatten(*fm.get_params(), [fm.get_embedding_params(k) for k in range(len(fm.dims))])


def _same_bits(a, b):
    return all(np.array_equal(np.asarray(x, f32).view(u32), np.asarray(y, f32).view(u32)) for x, y in zip(a, b))


def _opt(adam):
    return capi.OPT_ADAM if adam else capi.OPT_SGD


def _twins(d, dims, w, bs, adam, epochs=3, extra=0):
    """handle A on the materialised set, handle B on the samples: every epoch's cost and every tensor after the last"""
    model = _model(d, dims, 11 + d)
    lr, wd = A.rates(adam, d)
    a, b = _handle(d, dims, model), _handle(d, dims, model)
    _load_padded(a, w, extra)
    _load_samples(b, w)
    for e in range(epochs):
        ca, cb = a.epoch(bs, _opt(adam), lr, wd), b.epoch(bs, _opt(adam), lr, wd)
        assert np.isfinite(ca) and _same_bits([ca], [cb]), (e, ca, cb)
    pa, pb = _read(a), _read(b)
    assert not _same_bits(pa[:3], A.flatten(*model)[:3])  # it trained
    for name, x, y in zip(A.tensor_names(len(dims)), pa, pb):
        assert _same_bits([x], [y]), (name, int(np.sum(np.asarray(x).view(u32) != np.asarray(y).view(u32))))
    return a, b


# ---- 1. twin handles -------------------------------------------------------------------------------------------------------
_SHAPES = sorted({(d, dims) for d in (5, 8, 16, 17, 32, 64, 65, 128) for dims in ((), (65,))}
                 | {(d, dims) for d in (16, 128) for dims in ((1,), (63,), (64,), (65,), (130, 64))})


def test_the_world_holds_its_cases():
    w = _world((65,))
    idx, val, _, embs = w.materialise()
    assert len(w.users[0][0]) == 0 and len(w.items[3][0]) == 0 and set(w.ulead) == {0, 1} and set(w.ilead) == {0, 1}
    assert (w.users[5][1] == 0).any() and (w.items[4][1] == 0).any() and not embs[0][12].any() and w.item[12] == 9
    assert S.BOTH in w.users[7][0] and S.BOTH in w.items[6][0] and (w.user[3], w.item[3]) == (7, 6)
    for r0 in (0, 64):  # 64 positions of one feature in a batch: more than one pass of the accumulation loop at every width
        assert int(((idx[r0:r0 + 64] == S.SHARED) & (val[r0:r0 + 64] != 0)).sum()) == 64 > R.U_ACC * 64 // 8
    assert len(np.unique(w.item[:64])) < 64 and not val[140].any() and w.n % S.BS == 22


@pytest.mark.parametrize("adam", [False, True], ids=["sgd", "adam"])
@pytest.mark.parametrize("d,dims", _SHAPES, ids=lambda v: str(v).replace(" ", ""))
def test_twin_handles_three_epochs(d, dims, adam):
    _twins(d, dims, _world(dims), S.BS, adam)


@pytest.mark.parametrize("adam", [False, True], ids=["sgd", "adam"])
@pytest.mark.parametrize("bs,n", [(1, 3), (256, S.N), (64, 5)], ids=["bs1-n3", "bs256", "n5"])
def test_twin_handles_batch_edges(bs, n, adam):
    """batch 1 with n = 3; a batch larger than the set; fewer rows than the 8 gradient segments"""
    w = _world((65,))
    _twins(16, (65,), w if n == S.N else w.head(n), bs, adam)


def test_twin_handles_any_padded_width():
    """the materialised rows may be padded wider than the longest row"""
    _twins(16, (65,), _world((65,)), S.BS, True, extra=3)


# ---- 2. independent of the device's padded route ------------------------------------------------------------------------------
@pytest.mark.parametrize("adam", [False, True], ids=["sgd", "adam"])
@pytest.mark.parametrize("dims", [(), (65,)], ids=str)
@pytest.mark.parametrize("d", [8, 65])
def test_one_step_against_float64(d, dims, adam):
    w = _world(dims)
    idx, val, tgt, embs = w.materialise()
    B, W, V, fields = model = _model(d, dims, 23 + d)
    lr, wd = A.rates(adam)
    fm = _handle(d, dims, model)
    _load_samples(fm, w)
    cost = fm.epoch(w.n, _opt(adam), lr, wd)  # one batch: one step
    if not dims:
        rep = R.one_step_report(B, W, V, idx, val, tgt, fm.get_params(), cost, adam, lr, wd)
        print("one step d=%d %s: %s" % (d, "adam" if adam else "sgd", rep))
        assert rep["cost"] <= 1 and rep["B"] <= 1 and rep["W"] <= 1 and rep["V"] <= 1
        for name in ("W_unt", "V_unt"):
            mism, ulp, n_body, n_tail = rep[name]
            assert n_body > 0 and mism == 0 and ulp <= 1
        if not adam:
            assert rep["gW"] <= 1 and rep["gV"] <= 1
        else:
            for name in ("W_ill", "V_ill"):
                n_ill, n_touched, ratio = rep[name]
                assert n_ill <= A.ILL_SHARE * n_touched and ratio <= 1
        return
    rep = A.one_step_report(B, W, V, fields, idx, val, embs, tgt, _read(fm), cost, adam, lr, wd)
    print("one step d=%d %s %s: worst error over bar %.3g; %s" % (d, dims, "adam" if adam else "sgd", A.worst(rep), rep))
    assert not rep["still"], rep["still"]
    for k, v in rep.items():
        if k.endswith("_zero"):
            assert v[0] == 0 and v[1] <= (1 if k in ("W_zero", "V_zero") else 0), (k, v)
        elif k.endswith("_ill"):
            assert v[2] <= 1, (k, v)
        elif k == "ill":
            assert v[0] <= A.ILL_SHARE * v[1], v
        elif k != "still":
            assert v <= 1, (k, v)


# ---- 3. evaluation -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", ["mixed", "no-positive", "no-negative"])
@pytest.mark.parametrize("dims", [(), (65,)], ids=str)
def test_evaluate_samples_equals_padded_split(dims, split):
    w = _world(dims).head(S.N)
    if split != "mixed":
        w.target = np.full(w.n, -1.0 if split == "no-positive" else 1.0, f32)
    idx, val, tgt, embs = w.materialise()
    model = _model(16, dims, 5)
    a, b = _handle(16, dims, model), _handle(16, dims, model)
    a.set_test(idx, val, tgt, embs)
    _set_items(b, w)
    b.set_test_samples(*w.user_csr(), w.user, w.item, w.target, user_lead=w.ulead)
    for bs in (1, 7, 64, 512):
        ca, sa, la = a.evaluate(bs, logits=True)
        cb, sb, lb = b.evaluate(bs, logits=True)
        assert ca == cb and ca["n_pos"] == int((tgt > 0).sum()) and ca["n_pos"] + ca["n_neg"] == w.n, (bs, ca, cb)
        assert _same_bits([sa], [sb]) and _same_bits([la], [lb]), bs
        assert a.evaluate_stats()["slices"] == b.evaluate_stats()["slices"]
    b.set_test_samples(*w.user_csr(), w.user[:0], w.item[:0], w.target[:0], user_lead=w.ulead)  # n = 0 drops the split
    with pytest.raises(capi.GorseHipError):
        b.evaluate(64)


# ---- 4. lifetime and errors ------------------------------------------------------------------------------------------------
def _raises(code, fn, *a, **kw):
    with pytest.raises(capi.GorseHipError) as e:
        fn(*a, **kw)
    assert e.value.code == code, (e.value.code, str(e.value))
    return str(e.value)


def _step(fm, adam=True, bs=S.BS):
    return fm.epoch(bs, _opt(adam), *A.rates(adam, 16))


def test_catalogue_changes_drop_both_sets():
    dims = (65,)
    w = _world(dims)
    fm = _handle(16, dims, _model(16, dims, 3))
    test = lambda: fm.set_test_samples(*w.user_csr(), w.user, w.item, w.target, user_lead=w.ulead)  # noqa: E731
    for change in (lambda: _set_items(fm, w),                                      # replacing the catalogue
                   lambda: fm.set_items(np.zeros(1, np.int64), [], [], embs=()),   # dropping it
                   lambda: fm.set_embedding_dims(dims)):                           # the field set
        _load_samples(fm, w)
        test()
        _step(fm)
        fm.evaluate(64)
        change()
        assert "dropped" in _raises(capi.ERR_INVALID, _step, fm)
        assert "dropped" in _raises(capi.ERR_INVALID, fm.evaluate, 64)
    # with no catalogue both calls are refused; then everything works again
    _raises(capi.ERR_INVALID, _load_samples, fm, w, items=False)
    _raises(capi.ERR_INVALID, test)
    _set(fm, _model(16, dims, 3))
    _load_samples(fm, w)
    test()
    assert np.isfinite(_step(fm)) and fm.evaluate(64)[0]["n_pos"] == int((w.target > 0).sum())


def test_each_training_form_replaces_the_other():
    dims = (65,)
    w = _world(dims)
    model = _model(16, dims, 4)
    a, b = _handle(16, dims, model), _handle(16, dims, model)
    _load_padded(a, w)
    _load_samples(b, w)
    assert "sample form" in _raises(capi.ERR_INVALID, b.set_train_embeddings, 0, w.materialise()[3][0])
    costs = []
    for stage in range(3):  # b: samples, padded, samples again; a: padded throughout
        if stage == 1:
            _load_padded(b, w)
        if stage == 2:
            _load_samples(b, w, items=False)
        ca, cb = _step(a), _step(b)
        costs.append(ca)
        assert _same_bits([ca], [cb]) and _same_bits(_read(a), _read(b)), stage
    assert len(set(costs)) == 3
    # a padded set on a handle that trained from samples needs its embeddings again
    _load_samples(b, w, items=False)
    idx, val, tgt, _ = w.materialise()
    b.set_train(idx, val, tgt)
    _raises(capi.ERR_INVALID, _step, b)


def test_a_refused_set_leaves_the_previous_one():
    dims = (65,)
    w = _world(dims)
    model = _model(16, dims, 6)
    a, b = _handle(16, dims, model), _handle(16, dims, model)
    _load_padded(a, w)
    _load_samples(b, w)
    uptr, uidx, uval = w.user_csr()
    b.set_test_samples(uptr, uidx, uval, w.user, w.item, w.target, user_lead=w.ulead)
    before = b.evaluate(64, logits=True)

    def bad(which):
        user, item, idx, ptr, lead, tgt = w.user.copy(), w.item.copy(), uidx.copy(), uptr.copy(), w.ulead.copy(), w.target
        code = capi.ERR_RANGE
        if which == "user":
            user[77] = S.N_USERS
        elif which == "user<0":
            user[0] = -1
        elif which == "item":
            item[149] = S.N_ITEMS
        elif which == "feature":
            idx[-1] = S.NF
        elif which == "indptr":
            ptr[5], code = ptr[6] + 1, capi.ERR_INVALID
        elif which == "lead":
            lead[0], code = 1, capi.ERR_INVALID  # user 0 has no entries
        return code, (ptr, idx, uval, user, item, tgt), dict(user_lead=lead)

    for which in ("user", "user<0", "item", "feature", "indptr", "lead"):
        code, args, kw = bad(which)
        _raises(code, b.set_train_samples, *args, **kw)
        _raises(code, b.set_test_samples, *args, **kw)
    _raises(capi.ERR_INVALID, b.set_train_samples, uptr, uidx, uval, w.user[:0], w.item[:0], w.target[:0], user_lead=w.ulead)
    ca, cb = _step(a), _step(b)
    assert _same_bits([ca], [cb]) and _same_bits(_read(a), _read(b))
    _set(b, model)
    after = b.evaluate(64, logits=True)
    assert before[0] == after[0] and _same_bits(before[1:], after[1:])


def test_rank_and_evaluate_between_epochs_change_nothing():
    dims = (65,)
    w = _world(dims)
    model = _model(16, dims, 8)
    a, b = _handle(16, dims, model), _handle(16, dims, model)
    for fm in (a, b):
        _load_samples(fm, w)
    b.set_test_samples(*w.user_csr(), w.user, w.item, w.target, user_lead=w.ulead)
    assert _same_bits([_step(a)], [_step(b)])
    uptr, uidx, uval = w.user_csr()
    cptr = np.arange(S.N_USERS + 1, dtype=np.int64) * 5
    cand = (np.arange(S.N_USERS * 5) % S.N_ITEMS).astype(np.int32)
    scores, order = b.rank_users(uptr, uidx, uval, cptr, cand, 64, user_lead=w.ulead)
    assert np.isfinite(scores).all()
    b.evaluate(7)
    assert _same_bits([_step(a)], [_step(b)]) and _same_bits(_read(a), _read(b))


# ---- 5. host mirror ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host_eval", [False, True], ids=["resident", "host-evaluate"])
@pytest.mark.parametrize("dims", [(), (65,)], ids=str)
def test_fit_samples_equals_fit_on_materialised_sets(dims, host_eval):
    from gorse_amd import ctr
    w = S.LabelWorld(dims)
    train = ctr.SampleDataset(w.n_features, *w.sides(), embs=w.embs, samples=w.train)
    test = ctr.SampleDataset(w.n_features, *w.sides(), embs=w.embs, samples=w.test)
    kw = dict(nFactors=16, nEpochs=5, batchSize=64, lr=0.01, reg=0.001, optimizer=ctr.Adam, seed=7)
    a, b = ctr.FM(**kw), ctr.FM(**kw)
    for m in (a, b):
        m.SetHostEvaluate(host_eval)
    sa = a.Fit(train.Materialise(), test.Materialise(), Verbose=2)
    sb = b.FitSamples(train, test, Verbose=2)
    la, lb = a.log(), b.log()
    assert [e for e, _, _ in la] == [0, 2, 4, 5] and la[-1][1] > 0 and 0 < la[-1][2] < 1
    assert [e for e, _, _ in la] == [e for e, _, _ in lb]
    assert _same_bits([[c for _, c, _ in la]], [[c for _, c, _ in lb]]) and _same_bits([[x for _, _, x in la]], [[x for _, _, x in lb]])
    assert _same_bits([[sa.Precision, sa.Recall, sa.Accuracy, sa.AUC]], [[sb.Precision, sb.Recall, sb.Accuracy, sb.AUC]])
    assert _same_bits(a.params(), b.params())
    for k in range(len(dims)):
        assert _same_bits(a.field_params(k), b.field_params(k)), k
    # the catalogue stayed resident: RankUsers needs no SetItems, and a fresh SetItems changes nothing
    uid, urows, iid, irows = w.sides()
    rng = np.random.default_rng(1)
    cands = [list(rng.integers(0, w.n_items, int(rng.integers(0, 9)))) for _ in range(w.n_users)]
    kept = b.RankUsers(uid, urows, cands)
    b.SetItems(iid, irows, w.embs)
    fresh = b.RankUsers(uid, urows, cands)
    a.SetItems(iid, irows, w.embs)
    other = a.RankUsers(uid, urows, cands)
    for x, y, z in zip(kept, fresh, other):
        assert [c for c, _ in x] == [c for c, _ in y] == [c for c, _ in z]
        assert _same_bits([[s for _, s in x]], [[s for _, s in y]]) and _same_bits([[s for _, s in x]], [[s for _, s in z]])
    assert sum(len(x) for x in kept) == sum(len(c) for c in cands) > 0
