"""The FM ranker's item-embedding attention branch on the MI355X per element, at the shape edges of its kernels (att_score /
att_exp / att_enc / att_loss / att_bwd_gx / att_bwd_ds / att_grad and fm_dense_opt): one step at every edge, several steps
with a partial last batch, one handle through buffer rebuilds, a second training set and a second Fit, and scoring at the same
edges.  The reference is always fm_attention_ref.py: float64 gradients (grads_ex), the optimizer restated in fp32
(fm_ref.opt_step32), carried from step to step by StepTrainer.  Every test prints its worst error over bar before it asserts.

Inputs (fm_attention_ref.model / rows / case): H ~ Normal(0, 0.3) (4.5 / sqrt(d) at D = 4096), biases ~ Normal(0, 0.1), bf16
embeddings ~ Normal(0, 1) with rows 4, 11, 18, ... all zero, both signs of pre.  One quantity at a time moves around
(d, dims, n) = (20, (65,), 13): d over the factor chunks of 16 and both paths of load_w16, D over the 64-column tiles of
att_grad_kernel with the bias column at lane 63 / alone in a tile / alone in tile 65, n over empty and ragged row segments and
idle waves, n dividing D, not dividing D and above D.

Tolerances (fm_attention_ref.one_step_report / params_report form the ratios; test_fm_attention_cpu.py checks each claim on the CPU,
on these inputs):

  one step, parameters       1e-5 (|ref| + lr), the bar of test_gpu_fm_attention.py::test_one_step_parity, on every element whose
                             float64 gradient is not exactly zero.  The fp32 numpy restatement of the gradients sits at 0.0764
                             (SGD) / 0.360 (Adam; 0.385 on the ill-conditioned elements' bar) of it at worst: A.HEADROOM,
                             which the CPU test measures again.  Every field tensor must have moved (with wd > 0 one whose
                             gradient is all zero, H / Wa / ba at D = 1, moves by weight decay alone and is held to the
                             zero-gradient rule below).
  one step, cost             1e-5 relative, as there (restatement: 0.00505).
  one step, zero gradient    elements whose float64 gradient is exactly zero -- rows of W and V the batch does not touch, a
                             factor whose relu no row opens (half of them at n = 1), everything before the softmax at D = 1 (it
                             is 1 whatever s is) -- equal the zero-gradient opt_step32 bit for bit, FMA body and unfused tail
                             (the rule of test_zero_embeddings_leave_a_zero_gradient) in all five tensors of every field; the
                             plain W and V (fm_opt_kernel's step) within one ulp in the tail, as in
                             test_gpu_fm_train_shapes.py.  No margin: exact.
  one step, carried gradient SGD only: (p0 - p1) / lr - wd p0 against the float64 gradient within
                             1e-5 scale + 2^-23 (|p1| / lr + |g| + wd |p0|), the plain machine's form; scale is grads_ex's
                             per-element sum of the magnitudes an fp32 evaluation rounds, upstream quantities (denc, da, ds,
                             dpre) entering by their own magnitude sums.  The constant 1e-5 is the project's: the restatement
                             sits at 0.499 of the bar at worst over all 28 cases (the rounding term, as in the plain machine),
                             D = 4096 included, so it was not set from a measurement.
                             What the bars exclude (one SGD step, weakest case, in bars): row softmax 1.1e4; a row lost from
                             dH / dWa / dWe 561; dbe zero 7.6e3, dba zero 74; the relu gate ignored 635; a column lost 3.5e3;
                             a later field's enc missing from dV 6.9e4; a field reading the previous field's gx 1.4e4.
  one step, Adam             the first step is p - lr b1 / (|b1| + e), b1 = grad + wd p: where b1 all but cancels, elements
                             get the plain machine's widened bar (flat + lr gbar e / (|b1| + e)^2) and are counted.  Which
                             elements these are depends on the reference alone: at most 3.09 % of a case's elements
                             ((128, (4096,), 9)); the cap A.ILL_SHARE = 6.2 % is twice that.
  several steps              |got - ref| <= K (|ref| + lr), K = 2.24e-6 (SGD), 2.72e-5 (Adam) = 4 x the largest divergence of
                             the fp32-step reference from its all-float64 twin over the multi-step and life-cycle schedules
                             here: 5.59e-7 / 6.79e-6 (both at d = 100), recorded as 5.6e-7 / 6.8e-6.  Adam adds
                             StepTrainer.slack, capped at fm_ref.SLACK_CAP bars.  A wrapped modulus taken from the full batch
                             size shows in the partial batch, as the worst tensor's bars out: 3.2e4 (SGD, d = 20), 2.1e4
                             (SGD, d = 100), 8.4e3 (Adam, d = 20), 1.2e4 (Adam, d = 100).  At d = 100 the rates are a tenth of
                             the one-step rates: at the full ones the wrapped softmax lets that model's logits run away (scale
                             49 to 1.5e3 in twelve steps).  With these rates every logit's scale stays within 1.73 x its value
                             at the first step over every schedule (d = 20 SGD: 11.6 to 20.1; d = 100: 1.54 x at most; life
                             cycle 1.40 x); the CPU test asserts 2 x (A.SCALE_GROWTH).
  epoch cost                 1e-4 relative, the existing bar.
  scoring                    1e-5 of a row's scale, the bar of test_scoring_parity.

Between steps the parameters are read from a second handle that runs every batch as a one-batch epoch over its slice
(set_train + set_train_embeddings + epoch(rows)); the production call runs on a first handle and must match it bit for bit at
each epoch's end.

Measured on the MI355X (profiles/r10_fm_attention_shapes_pytest.log, 64 passed), worst error over bar: one step, parameters 0.058
(SGD, We at D = 4096), 0.11 (Adam, We at d = 128, D = 4096; its ill-conditioned elements 0.14 of theirs), carried gradient
0.499 (dH at d = 128, D = 4096: the rounding term, the restatement's own figure), cost 0.010, zero-gradient elements 0 bits /
0 ulp; three epochs SGD 0.12 (d = 100), Adam 0.053, the two handles equal in every bit; life cycle 0.045 (SGD) / 0.065 (Adam);
epoch cost 0.0018; scoring 0.0057."""
import numpy as np
import pytest

import fm_attention_ref as A
import fm_ref as R
from gorse_amd import capi

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
K_MULTI = A.K_MULTI
ILL_SHARE = A.ILL_SHARE  # twice the largest share of ill-conditioned elements the reference alone produces (3.09 %)
_CASES = {}


def _case(c):
    if c not in _CASES:
        _CASES[c] = A.case(*c)
    return _CASES[c]


def _opt(adam):
    return capi.OPT_ADAM if adam else capi.OPT_SGD


def _handle(d, dims, B, W, V, fields):
    fm = capi.FM(A.NF, d, embedding_dims=dims)
    _set(fm, B, W, V, fields)
    return fm


def _set(fm, B, W, V, fields):
    fm.set_params(B, W, V)
    for k, fld in enumerate(fields):
        fm.set_embedding_params(k, *fld)


def _load(fm, idx, val, tgt, embs):
    fm.set_train(idx, val, tgt)
    for k, e in enumerate(embs):
        fm.set_train_embeddings(k, e)


def _read(fm, n_fields):
    return A.flatten(*fm.get_params(), [fm.get_embedding_params(k) for k in range(n_fields)])


def _id(c):
    return "d%d-D%s-n%d" % (c[0], "_".join(map(str, c[1])), c[2])


@pytest.mark.parametrize("adam", [False, True], ids=["sgd", "adam"])
@pytest.mark.parametrize("c", A.ONE_STEP, ids=_id)
def test_one_step_at_every_edge(c, adam):
    d, dims, n = c
    B, W, V, fields, idx, val, tgt, embs = _case(c)
    lr, wd = A.rates(adam)
    fm = _handle(d, dims, B, W, V, fields)
    _load(fm, idx, val, tgt, embs)
    cost = fm.epoch(n, _opt(adam), lr, wd)
    rep = A.one_step_report(B, W, V, fields, idx, val, embs, tgt, _read(fm, len(dims)), cost, adam, lr, wd)
    print("one step %s %s: worst error over bar %.3g; %s" % (_id(c), "adam" if adam else "sgd", A.worst(rep),
                                                              {k: (float("%.3g" % v) if isinstance(v, float) else v) for k, v in rep.items()}))
    assert not rep["still"], rep["still"]  # every tensor of the branch moved
    assert rep["W_zero"][2] > 0 and rep["W_zero"][3] > 0 and ((A.NF * d) % 16 == 0 or rep["V_zero"][3] > 0)  # untouched rows, tails too
    for k, v in rep.items():
        if k.endswith("_zero"):
            assert v[0] == 0 and v[1] <= (1 if k in ("W_zero", "V_zero") else 0), (k, v)
        elif k.endswith("_ill"):
            assert v[2] <= 1, (k, v)
        elif k == "ill":
            assert v[0] <= ILL_SHARE * v[1], v
        elif k != "still":
            assert v <= 1, (k, v)
    if not adam:
        assert "gV" in rep and "gWe[%d]" % (len(dims) - 1) in rep and "gbe[0]" in rep
    if n == 1 or max(dims) == 1:
        assert "ba[0]_zero" in rep  # a relu no row opens / the constant softmax: exact zeros in the branch's own tensors


def _same_bits(a, b):
    return all(np.array_equal(np.asarray(x, f32).view(np.uint32), np.asarray(y, f32).view(np.uint32)) for x, y in zip(a, b))


def _worst(r):
    return max(r.values())


@pytest.mark.parametrize("adam", [False, True], ids=["sgd", "adam"])
@pytest.mark.parametrize("d,dims", A.MULTI)
def test_three_epochs_per_element(d, dims, adam):
    n, bs = A.MULTI_N, A.MULTI_BS  # batches of 13, 13, 13, 6: r0 > 0, and the softmax's modulus changes inside the epoch
    idx, val, tgt, embs = A.rows(n, dims, 7 + d)
    B, W, V, fields = A.model(d, dims, 5 + d)
    lr, wd = A.rates(adam, d)
    K = K_MULTI[adam]
    prod, step = _handle(d, dims, B, W, V, fields), _handle(d, dims, B, W, V, fields)
    _load(prod, idx, val, tgt, embs)
    ref = A.StepTrainer(B, W, V, fields)
    worst = {"step": 0.0, "epoch": 0.0, "cost": 0.0}
    for e in range(3):
        c_dev = prod.epoch(bs, _opt(adam), lr, wd)
        c_ref = f32(0)
        for i in range(0, n, bs):
            sl = slice(i, min(i + bs, n))
            es = [x[sl] for x in embs]
            _load(step, idx[sl], val[sl], tgt[sl], es)
            step.epoch(sl.stop - sl.start, _opt(adam), lr, wd)
            got = _read(step, len(dims))
            c_ref = f32(c_ref + f32(ref.step(idx[sl], val[sl], es, tgt[sl], adam, lr, wd)))
            r = A.params_report(got, ref.p, lr, K, ref.slack if adam else None)
            worst["step"] = max(worst["step"], _worst(r))
            assert _worst(r) <= 1, (e, i, r)
        last = got
        got = _read(prod, len(dims))
        r = A.params_report(got, ref.p, lr, K, ref.slack if adam else None)
        worst["epoch"] = max(worst["epoch"], _worst(r))
        worst["cost"] = max(worst["cost"], abs(c_dev - c_ref) / (1e-4 * abs(c_ref)))
        assert _worst(r) <= 1, (e, r)
        assert abs(c_dev - c_ref) <= 1e-4 * abs(c_ref), (c_dev, c_ref)
        assert _same_bits(got, last), "the production epoch and the batch-by-batch handle took different steps"
    print("three epochs d=%d dims=%s %s: worst error over bar %s" % (d, dims, "adam" if adam else "sgd", worst))


@pytest.mark.parametrize("adam", [False, True], ids=["sgd", "adam"])
def test_handle_life_cycle(adam):
    d, dims = A.LIFE
    S, S2 = A.rows(45, dims, 71), A.rows(40, dims, 72)
    lr, wd = A.rates(adam, d)
    K = K_MULTI[adam]
    B, W, V, fields = A.model(d, dims, 5 + d)
    fm = _handle(d, dims, B, W, V, fields)
    _load(fm, *S)
    ref = A.StepTrainer(B, W, V, fields)
    worst = []
    for name, (idx, val, tgt, embs), bs, new_set, new_fit in A.life_stages(S, S2):
        if new_set:
            _load(fm, idx, val, tgt, embs)  # the first set's embeddings are dropped with it
        if new_fit:
            B, W, V, fields = A.model(d, dims, 6 + d)
            _set(fm, B, W, V, fields)  # Adam's t restarts and every moment is zeroed: a fresh reference
            ref = A.StepTrainer(B, W, V, fields)
        c_dev = fm.epoch(bs, _opt(adam), lr, wd)
        c_ref = ref.epoch(idx, val, embs, tgt, bs, adam, lr, wd)
        r = A.params_report(_read(fm, len(dims)), ref.p, lr, K, ref.slack if adam else None)
        worst.append((name, float("%.3g" % _worst(r)), float("%.3g" % (abs(c_dev - c_ref) / (1e-4 * abs(c_ref))))))
        print("life cycle %s %s: %s" % ("adam" if adam else "sgd", name, {k: float("%.3g" % v) for k, v in r.items()}))
        assert _worst(r) <= 1, (name, r)
        assert abs(c_dev - c_ref) <= 1e-4 * abs(c_ref), (name, c_dev, c_ref)
    print("life cycle %s: (stage, parameters over bar, cost over bar) %s" % ("adam" if adam else "sgd", worst))


@pytest.mark.parametrize("d,dims,batch_sizes", [(128, (4096,), (1, 3, 67)), (20, (5, 129, 64), (1, 3, 67))])
def test_scoring_at_the_same_edges(d, dims, batch_sizes):
    """d = 128 with D = 4096, and three fields whose largest D is not field 0 (scoring works every field in field 0's
    buffers), at batch lengths 1, 3 and 67 (67 rows: n = 1 is the row softmax, 3 leaves a partial batch of 1)"""
    n = 67
    B, W, V, fields = A.model(d, dims, 900 + d)
    idx, val, _, embs = A.rows(n, dims, 901 + d)
    fm = _handle(d, dims, B, W, V, fields)
    for bs in batch_sizes:
        want, scale = A.predict(B, W, V, fields, idx, val, embs, bs)
        w32, _ = A.predict(B, W, V, fields, idx, val, embs, bs, dtype=f32)
        assert np.all(np.abs(w32 - want) <= 0.5 * 1e-5 * scale), ("the restatement's own fp32 error", bs)
        got = fm.predict_embeddings(idx, val, embs, bs)
        err = np.max(np.abs(got - want) / scale)
        print("scoring d %d dims %s bs %d: worst error over bar %.3g" % (d, dims, bs, err / 1e-5))
        assert np.all(np.abs(got - want) <= 1e-5 * scale), (bs, err)
    plain = R.forward64(B, W, V, idx, val)[0]
    assert np.max(np.abs(want - plain) / scale) > 100 * 1e-5  # the branch is in the result at all
