"""gorse_fm_set_test / gorse_fm_evaluate on the MI355X.  The yardsticks are the EXISTING routes: the host library's
ctr.Precision / Recall / Accuracy / AUC for the metric stage, predict / predict_embeddings on the positive rows alone and on the
negative rows alone for the logits, and Evaluate(test) / a Fit with SetHostEvaluate(True) for the whole.  Every comparison is of
bits.  fm_eval_ref restates the counts in numpy; test_fm_evaluate_cpu.py pins that restatement to the host metrics."""
import numpy as np
import pytest

import fm_attention_ref as A
import fm_eval_ref as E
from gorse_amd import capi, ctr

pytestmark = pytest.mark.gpu
f32, u32 = np.float32, np.uint32
_i64p, _f32p = capi._i64p, capi._f32p


@pytest.fixture(autouse=True)
def _default_hooks():
    capi.lib().gorse_hip_test_set_fm_evaluate(0, 0)
    yield
    capi.lib().gorse_hip_test_set_fm_evaluate(0, 0)


@pytest.fixture(scope="module")
def plain():
    fm = capi.FM(16, 8)
    yield fm
    fm.close()


def _auc(fm, pos, neg):
    pos, neg = np.ascontiguousarray(pos, f32), np.ascontiguousarray(neg, f32)
    c, s = np.zeros(7, np.int64), np.zeros(1, f32)
    capi.check(capi.lib().gorse_hip_test_fm_auc(fm.h, capi._p(pos, _f32p), pos.size, capi._p(neg, _f32p), neg.size,
                                                capi._p(c, _i64p), capi._p(s, _f32p)))
    return [int(x) for x in c], s[0]


def _check_metrics(fm, pos, neg, tag):
    c, s = _auc(fm, pos, neg)
    want_c, want_s = E.counts(pos, neg)
    assert c == want_c, (tag, c, want_c)
    assert E.same_bits(s, want_s), (tag, s, want_s)
    assert E.same_bits(E.score(c, s), E.host_score(pos, neg)), (tag, E.score(c, s), E.host_score(pos, neg))
    return c, s


# ---- 1. the metric stage alone -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(E.CONTENTS))
def test_metric_stage(plain, kind):
    """every pair of sizes around the wave, the workgroup and the tile (three tiles at 3 * 256 + 7), one side empty included:
    counts, pairs_less against searchsorted, auc_sum and the four Score fields in every bit"""
    capi.lib().gorse_hip_test_set_fm_evaluate(0, 256)
    for n_pos in E.SIZES:
        for n_neg in E.SIZES:
            pos, neg = E.sides(kind, n_pos, n_neg)
            _check_metrics(plain, pos, neg, (kind, n_pos, n_neg))


def test_metric_stage_where_the_chain_rounds(plain):
    """8192 x 8192 at the library's own tile: the exact total passes 2^25 and the float32 chain leaves it"""
    pos, neg = E.wide()
    c, s = _check_metrics(plain, pos, neg, "wide")
    assert c[6] > 1 << 25
    host_chain = f32(ctr.AUC(pos, neg)) * f32(8192 * 8192)  # exact: the divisor is a power of two
    assert float(host_chain) != float(c[6])
    assert E.same_bits(f32(s) / f32(8192 * 8192), f32(ctr.AUC(pos, neg)))


def test_metric_stage_with_nans(plain):
    capi.lib().gorse_hip_test_set_fm_evaluate(0, 256)
    pos, neg = E.with_nans()
    c, s = _auc(plain, pos, neg)
    want_c, _ = E.counts(pos, neg)
    assert c == want_c and c[5] == 5
    keep_p, keep_n = pos[~np.isnan(pos)], neg[~np.isnan(neg)]
    assert c[6] == int(np.searchsorted(np.sort(keep_n), keep_p, side="left").sum())
    assert E.same_bits(f32(s) / f32(keep_p.size * keep_n.size), f32(ctr.AUC(keep_p, keep_n)))


# ---- 2. scoring from the resident split ------------------------------------------------------------------------------------
def _handle(d, dims, B, W, V, fields):
    fm = capi.FM(A.NF, d, embedding_dims=dims)
    fm.set_params(B, W, V)
    for k, fld in enumerate(fields):
        fm.set_embedding_params(k, *fld)
    return fm


def _split(d, dims, n, seed, targets=None):
    """a model and n test rows: rows 4, 11, ... carry a zero embedding (fm_attention_ref.rows), row 2 has no entries, and
    a few targets are exactly 0 (negatives)"""
    B, W, V, fields = A.model(d, dims or (1,), seed)
    fields = fields[:len(dims)]
    idx, val, tgt, embs = A.rows(n, dims, seed + 1)
    if n > 2:
        val[2] = 0
    if targets is not None:
        tgt = np.full(n, targets, f32)
    elif n > 9:
        tgt[[3, 9]] = 0
    return (B, W, V, fields), (idx, val, tgt, embs)


def _predict(fm, dims, idx, val, embs, bs):
    if idx.shape[0] == 0:
        return np.zeros(0, f32)
    return fm.predict_embeddings(idx, val, embs, bs) if dims else fm.predict(idx, val)


def _expect(fm, dims, rows, bs):
    """predict / predict_embeddings on the positives alone and on the negatives alone, scattered back to dataset order"""
    idx, val, tgt, embs = rows
    out = np.zeros(len(tgt), f32)
    for side in (tgt > 0, ~(tgt > 0)):
        out[side] = _predict(fm, dims, idx[side], val[side], [e[side] for e in embs], bs)
    return out


def _check_scoring(d, dims, n, bs_list, seed, targets=None, round_factor=None):
    model, rows = _split(d, dims, n, seed, targets)
    fm = _handle(d, dims, *model)
    fm.set_test(rows[0], rows[1], rows[2], rows[3])
    tgt = rows[2]
    if targets is None:  # the positives' last slice is partial, so slicing on through the boundary would show
        assert int((tgt > 0).sum()) % bs_list[0] != 0
    for bs in bs_list:
        capi.lib().gorse_hip_test_set_fm_evaluate(round_factor * bs if round_factor else 0, 256)
        c, s, logits = fm.evaluate(bs, logits=True)
        want = _expect(fm, dims, rows, bs)
        assert E.same_bits(logits, want), (d, dims, n, bs, np.flatnonzero(logits.view(u32) != want.view(u32))[:8])
        want_c, want_s = E.counts(want[tgt > 0], want[~(tgt > 0)])
        assert [c[k] for k in capi.EVAL_COUNTS] == want_c and E.same_bits(s, want_s), (d, dims, n, bs, c, want_c)
        st = fm.evaluate_stats()
        n_pos = int((tgt > 0).sum())
        assert st["rows"] == n and st["slices"] == -(-n_pos // bs) + -(-(n - n_pos) // bs)
        if round_factor and n > round_factor * bs:
            assert st["rounds"] > 1
    fm.close()
    return model, rows


@pytest.mark.parametrize("d", [8, 16, 32, 64, 128])
def test_scoring_every_lane_width(d):
    _check_scoring(d, (65,), 45, (7, 64), 10 + d, round_factor=2)


@pytest.mark.parametrize("dims", [(63,), (64,), (65,), (65, 9), ()], ids=str)
def test_scoring_every_column_edge(dims):
    """D around the wave, two fields of different D, and the plain machine (predict's bits); batch sizes 7, 64 and one larger
    than n; rounds of two slices, then the library's own"""
    _check_scoring(16, dims, 45, (7, 64, 100), 20 + sum(dims), round_factor=2)
    _check_scoring(16, dims, 45, (7, 100), 20 + sum(dims))


@pytest.mark.parametrize("targets", [1.0, -1.0, 0.0])
def test_scoring_one_side_only(targets):
    """all rows positive, all negative, and every target exactly 0 (negatives)"""
    model, rows = _check_scoring(16, (65,), 23, (7, 64), 31, targets=targets, round_factor=2)
    assert ((rows[2] > 0).sum() == 23) == (targets > 0)


def test_slicing_restarts_at_the_first_negative():
    """n_pos % batch_size != 0: slicing that ran on through the boundary would change the negatives' logits (shown on the numpy
    restatement), and the resident route does not do that (shown on the device in test_scoring_*)"""
    d, dims, bs = 16, (65,), 7
    (B, W, V, fields), (idx, val, tgt, embs) = _split(d, dims, 45, 20 + 65)
    pos, neg = tgt > 0, ~(tgt > 0)
    n_pos = int(pos.sum())
    assert n_pos % bs != 0 and (45 - n_pos) % bs != 0
    order = np.concatenate([np.flatnonzero(pos), np.flatnonzero(neg)])
    through = A.predict(B, W, V, fields, idx[order], val[order], [e[order] for e in embs], bs)[0][n_pos:]
    afresh = A.predict(B, W, V, fields, idx[neg], val[neg], [e[neg] for e in embs], bs)[0]
    assert not np.array_equal(through.astype(f32), afresh.astype(f32))
    assert np.max(np.abs(through - afresh)) > 1e-4


# ---- 3. lifetime and errors ------------------------------------------------------------------------------------------------
def test_lifetime_and_errors():
    d, dims, bs = 16, (65,), 7
    model, rows = _split(d, dims, 45, 41)
    idx, val, tgt, embs = rows
    fm = _handle(d, dims, *model)
    with pytest.raises(capi.GorseHipError) as e:  # nothing resident yet
        fm.evaluate(bs)
    assert e.value.code == capi.ERR_INVALID
    fm.set_test(idx, val, tgt, embs)
    with pytest.raises(capi.GorseHipError) as e:
        fm.evaluate(0)
    assert e.value.code == capi.ERR_INVALID
    base = fm.evaluate(bs, logits=True)
    assert E.same_bits(base[2], _expect(fm, dims, rows, bs))
    # a cancel flag set before the call
    with pytest.raises(capi.GorseHipError) as e:
        fm.evaluate(bs, cancel=np.ones(1, np.int32))
    assert e.value.code == capi.ERR_CANCELLED
    # an index out of range: the previous split keeps answering
    bad = idx.copy()
    bad[5, 0] = A.NF
    with pytest.raises(capi.GorseHipError) as e:
        fm.set_test(bad, val, tgt, embs)
    assert e.value.code == capi.ERR_RANGE
    again = fm.evaluate(bs, logits=True)
    assert again[0] == base[0] and E.same_bits(again[1], base[1]) and E.same_bits(again[2], base[2])
    # set_params, an epoch and rank_users leave the split alone: it is scored with the parameters of the moment
    fm.set_params(*model[:3])
    fm.set_train(idx, val, np.where(tgt > 0, 1, -1).astype(f32))
    fm.set_train_embeddings(0, embs[0])
    fm.epoch(13, capi.OPT_ADAM, 0.01, 0.0)
    fm.set_items(np.arange(4, dtype=np.int64), np.array([1, 2, 3], np.int32), np.ones(3, f32), embs=[embs[0][:3]])
    fm.rank_users(np.array([0, 1], np.int64), np.array([5], np.int32), np.ones(1, f32), np.array([0, 3], np.int64),
                  np.array([0, 1, 2], np.int32), bs)
    moved = fm.evaluate(bs, logits=True)
    assert E.same_bits(moved[2], _expect(fm, dims, rows, bs)) and not E.same_bits(moved[2], base[2])
    # n = 0 drops it, and so does set_embedding_dims
    fm.set_test(idx[:0], val[:0], tgt[:0], [embs[0][:0]])
    with pytest.raises(capi.GorseHipError) as e:
        fm.evaluate(bs)
    assert e.value.code == capi.ERR_INVALID
    fm.set_test(idx, val, tgt, embs)
    fm.evaluate(bs)
    fm.set_embedding_dims(dims)
    with pytest.raises(capi.GorseHipError) as e:
        fm.evaluate(bs)
    assert e.value.code == capi.ERR_INVALID
    fm.close()


def test_evaluating_between_epochs_changes_nothing():
    """two handles trained alike, one of them evaluated between the epochs: the parameters agree in every bit"""
    d, dims, bs = 16, (65,), 13
    model, rows = _split(d, dims, 45, 43)
    idx, val, tgt, embs = rows
    got = []
    for evaluated in (False, True):
        fm = _handle(d, dims, *model)
        fm.set_train(idx, val, np.where(tgt > 0, 1, -1).astype(f32))
        fm.set_train_embeddings(0, embs[0])
        if evaluated:
            fm.set_test(idx, val, tgt, embs)
        for _ in range(3):
            fm.epoch(bs, capi.OPT_ADAM, 0.01, 0.01)
            if evaluated:
                fm.evaluate(7)
        B, W, V = fm.get_params()
        got.append([np.array([B]), W, V] + list(fm.get_embedding_params(0)))
        fm.close()
    for a, b in zip(*got):
        assert E.same_bits(a, b)


# ---- 4. Fit ------------------------------------------------------------------------------------------------------------------
def _dataset(idx, val, tgt, embs, nf):
    lens = (val != 0).sum(1)
    indptr = np.concatenate([[0], np.cumsum(lens)])
    ii = np.concatenate([idx[i][val[i] != 0] for i in range(len(lens))])
    vv = np.concatenate([val[i][val[i] != 0] for i in range(len(lens))])
    ds = ctr.Dataset(nf, (indptr, ii, vv, tgt))
    if embs:
        ds.set_embeddings(embs)
    return ds


def test_fit_scores_keep_their_bits():
    """the same Fit (Adam, three epochs, Verbose 1, one field, a partial last batch) evaluated through the host route and from
    the resident split: the same log, the same Score, the same parameters; EvaluateResident afterwards equals Evaluate(test)"""
    d, dims = 16, (65,)
    tr = A.rows(150, dims, 51)
    te = A.rows(90, dims, 52)
    train, test = _dataset(*tr, A.NF), _dataset(*te, A.NF)
    runs = []
    for host_route in (True, False):
        m = ctr.FM(nFactors=d, nEpochs=3, batchSize=32, lr=0.01, reg=1e-4, optimizer=ctr.Adam, seed=1)
        m.SetHostEvaluate(host_route)
        s = m.Fit(train, test, Verbose=1)
        runs.append((m, s, m.log(), m.params(), m.field_params(0)))
    (m0, s0, lg0, p0, f0), (m1, s1, lg1, p1, f1) = runs
    assert [e for e, _, _ in lg1] == [0, 1, 2, 3]
    assert [e for e, _, _ in lg0] == [e for e, _, _ in lg1]
    assert E.same_bits([c for _, c, _ in lg0], [c for _, c, _ in lg1])
    assert E.same_bits([a for _, _, a in lg0], [a for _, _, a in lg1])
    assert s0 == s1
    for a, b in zip(list(p0) + list(f0), list(p1) + list(f1)):
        assert E.same_bits(a, b)
    assert m1.EvaluateResident() == m1.Evaluate(test)
    # a set made resident by hand, on the model the host route trained
    m0.SetTest(test)
    assert m0.EvaluateResident() == m0.Evaluate(test) == s0
