"""FM training on the MI355X per element: one step at every instantiation of fm_forward_kernel / fm_accum_kernel, several
steps with features that come and go, and one handle through plan rebuilds, a second training set and a second set_params.
The reference is always fm_ref.py: float64 gradients (grads64), the optimizer restated in fp32 (opt_step32), carried from
step to step by StepTrainer.  Every test prints its worst error over bar before it asserts.

Tolerances (fm_ref.one_step_report / params_report form the ratios; test_fm_cpu.py checks each claim below on the CPU):

  one step, untouched rows   bit-equal to the zero-gradient opt_step32 in the fused body, <= 1 ulp in the unfused tail (the
                             tail's mul + add may or may not be contracted by the device compiler).  No margin: exact.
  one step, touched, B       1e-5 (|ref| + lr), the bar of test_gpu_fm.py::test_one_step_parity.
  one step, cost             1e-5 relative, as there.
  one step, carried gradient SGD only: (p0 - p1) / lr - wd p0 against the float64 gradient, within
                             1e-5 grad_scale64 + 2^-23 (|p1| / lr + |g| + wd |p0|).  grad_scale64 is the sum of the magnitudes
                             an fp32 evaluation rounds (what forward64's scale is to a logit): the worst case of a sequential
                             fp32 sum of L = 272 such terms is L 2^-24 = 1.6e-5 of it, the expected error sqrt(L) 2^-24 = 1e-6;
                             the second term is the fp32 rounding of p1 and of grad + wd p seen through 1 / lr, twice (the
                             tail rounds twice).  The fp32 reference itself sits at 0.35-0.48 of this bar (the rounding term).
                             What the bars exclude: with any ONE position of the longest list (feature 7, in all 272 rows)
                             dropped or doubled, the parameters are >= 10 bars of the touched bar out and so is the carried
                             gradient (every 16th row and the rows of the smallest and largest loss gradient); one lane's share of one
                             position of that list, dropped or doubled, fails both at each of the five instantiations.
                             Adam's first step is p - lr b1 / (|b1| + e), b1 = grad + wd p, e = 3.2e-7: it keeps the sign
                             of b1 and little of its size.  With the model and wd = 0.01 of the SGD cases the sign follows
                             the gradient on most touched elements: a touched row given a zero gradient, the negated gradient
                             or another slot's gradient fails at each instantiation (test_fm_cpu.py); a gradient merely
                             mis-scaled shows under Adam from the second step on, in the multi-step tests.  Where b1 all but
                             cancels, the step turns a gradient error dg into lr dg e / (|b1| + e)^2, one fp32 ulp into
                             several bars.  Touched elements for which that amount, at dg = the carried-gradient bar above
                             (without its 1 / lr term), exceeds 1e-5 (|ref| + lr) are counted and held to the sum of the two
                             instead of the flat bar: 0.60 % (d = 1) to 1.04 % (d = 8, nf = 212) of the touched elements
                             of V, at most one of W; the test asserts the share stays below 2 %, and every other touched
                             element is held to the flat bar.
  several steps              |got - ref| <= K (|ref| + lr), K = 1.7e-6 (SGD), 1.5e-5 (Adam) = 4 x the largest divergence of
                             the fp32-step reference from an all-float64 run of the same schedules on the CPU over every case
                             here: 4.22e-7 (SGD, d = 64, after 12 steps), 3.70e-6 (Adam, d = 100, after 4 steps), recorded as 4.3e-7 / 3.8e-6; the life-cycle
                             schedule measures 3.0e-7 / 1.6e-6.  The float64 run takes the fp32 lr_t (a host scalar the library
                             forms in the same fp32 steps; in float64 too, the cancellation in 1 - beta2^t alone moves it by
                             3e-5).  The factor 4 absorbs the device's fixed-tree summation order against numpy's.
                             Adam adds StepTrainer.slack per element: what gradients that each sit within the one-step
                             gradient bar (1e-5 grad_scale64) may have moved the parameter by, summed over the steps:
                             lr_t (1 - beta1) 1e-5 grad_scale64 / (sqrt(v) + eps) per step, counted up to 16 K (|ref| + lr)
                             (fm_ref.SLACK_CAP).  Adam divides by sqrt(v): where grad + wd p has been near zero so far a
                             rounding error decides the step, and an fp32 numpy restatement of the gradient already stands at
                             1.14 K without the slack (d = 64, step 8).  Its size, as slack / (K (|ref| + lr)) over the
                             touched elements of V after the three epochs, d = 8 / 64 / 100: median 1.23 / 1.14 / 1.09, 99th
                             percentile 30 / 41 / 32, above 10 on 4.0 / 4.5 / 4.1 %, above the cap of 16 on 1.9 / 2.5 / 2.2 %
                             (uncapped it would peak at 284 / 8.8e3 / 1.4e3).  So Adam's bar is about 2.1 K = 8 x the measured
                             divergence at the median and at most 17 K anywhere; a lost position is still >= 10 bars out
                             (test_fm_cpu.py).
  several steps, untouched   SGD: rows a step does not touch equal the zero-gradient opt_step32 of their previous DEVICE value,
                             bit for bit (body) / <= 1 ulp (tail).  Adam: the same for rows no step has touched yet, whose
                             moments the reference reproduces exactly from weight decay alone; rows touched earlier carry
                             moments the test cannot read and fall under K (a stale gradient is five orders above it).
  life cycle                 every stage under K (+ slack) as above, read once per epoch (the production call cannot be read
                             between its steps).  Rows nothing has touched since set_params: bit-equal to the reference's
                             zero-gradient steps in the fused body; in the tail at most one ulp per step taken since
                             set_params (the per-step bound above; several steps pass between reads, and a step carries a
                             one-ulp difference on as one ulp: it scales p by 1 - lr wd).  Rows touched in one stage and not
                             in the next fall under K alone here; their bit-level check is the three-epoch test's.
  epoch cost                 1e-4 relative, the bar of test_gpu_fm.py::test_training_parity.

Between steps the parameters are read from a second handle that runs every batch as a one-batch epoch over its slice
(set_train + epoch(rows of the slice)): the kernels see the same rows, slots, tags and step numbers as in the production
call, only row0 / slot0 are zero.  The production call (one epoch() per epoch over the whole set, batches at row0 / slot0 > 0)
runs on a first handle, is held to the same reference, and must match the second handle bit for bit.

Measured on the MI355X (profiles/r09_fm_train_shapes_pytest.log), worst error over bar: one step, touched parameters 0.004 (SGD),
0.021 (Adam; its ill-conditioned elements 0.009 of theirs), carried gradient 0.44 (the same rounding term as the reference's
own), cost 0.010, untouched rows 0 bits / 0 ulp; several steps SGD 0.062, Adam 0.46 (d = 64); life cycle 0.047, tails 0 ulp;
epoch cost 0.0016."""
import numpy as np
import pytest

import fm_ref as R
from gorse_amd import capi

pytestmark = pytest.mark.gpu
f32 = np.float32
K_MULTI = R.K_MULTI
ILL_SHARE = 0.02  # twice the largest share of ill-conditioned touched elements of the Adam one-step cases (1.04 %)


def _model(nf, d, seed, sd=0.1):
    rng = np.random.default_rng(seed)
    return f32(0.1), rng.normal(0, sd, nf).astype(f32), rng.normal(0, sd, (nf, d)).astype(f32)


def _opt(adam):
    return capi.OPT_ADAM if adam else capi.OPT_SGD


def _rates(adam, one_step=False):
    if adam:
        return 0.01, 0.01
    return (0.25 if one_step else 0.1), 0.01


# d -> instantiation: 1, 8: <8, 1>; 16: <16, 1>; 17, 32: <32, 1>; 33, 64: <64, 1>; 65, 100, 128: <64, 2>.  nf = 211 leaves a tail
# (nf d % 16 != 0) wherever d allows one; (8, 212) has none; d % 4 != 0 puts touched and untouched rows into one float4.
ONE_STEP = [(1, 211), (8, 211), (8, 212), (16, 211), (17, 211), (32, 211), (33, 211), (64, 211), (65, 211), (100, 211), (128, 211)]


@pytest.mark.parametrize("adam", [False, True])
@pytest.mark.parametrize("d,nf", ONE_STEP)
def test_one_step_every_instantiation(d, nf, adam):
    n = 272  # more than one trip of the dB / loss block's loop, and > 2 U NG - 1 = 63 for every d
    idx, val, tgt, lists = R.shape_batch(d, nf, n, seed=d)
    T = R.trip(d)
    assert [len(R.rows_of(idx, val, f)) for f in (7, 1, 2, 4)] == [n, T, T + 1, 2 * T - 1]
    B, W, V = _model(nf, d, d + 50)
    lr, wd = _rates(adam, one_step=True)
    fm = capi.FM(nf, d)
    fm.set_params(B, W, V)
    fm.set_train(idx, val, tgt)
    cost = fm.epoch(n, _opt(adam), lr, wd)
    rep = R.one_step_report(B, W, V, idx, val, tgt, fm.get_params(), cost, adam, lr, wd)
    print("one step d=%d nf=%d %s: %s" % (d, nf, "adam" if adam else "sgd", rep))
    assert rep["cost"] <= 1 and rep["B"] <= 1 and rep["W"] <= 1 and rep["V"] <= 1
    for name in ("W_unt", "V_unt"):
        mism, ulp, n_body, n_tail = rep[name]
        assert n_body > 0 and (n_tail > 0 or (nf * (d if name[0] == "V" else 1)) % 16 == 0)
        assert mism == 0 and ulp <= 1
    if (nf * d) % 16:
        assert rep["V_unt"][3] > 0
    if d % 4:
        assert rep["straddle"] > 0
    if not adam:
        assert rep["gW"] <= 1 and rep["gV"] <= 1
    else:
        for name in ("W_ill", "V_ill"):
            n_ill, n_touched, ratio = rep[name]
            assert n_ill <= ILL_SHARE * n_touched + 1 and ratio <= 1


def _step_by_slice(fm, idx, val, tgt, sl, adam, lr, wd):
    fm.set_train(idx[sl], val[sl], tgt[sl])
    return fm.epoch(sl.stop - sl.start, _opt(adam), lr, wd)


def _same_bits(a, b):
    return all(np.array_equal(np.asarray(x, f32).view(np.uint32), np.asarray(y, f32).view(np.uint32)) for x, y in zip(a, b))


@pytest.mark.parametrize("adam", [False, True])
@pytest.mark.parametrize("d", [8, 64, 100])
def test_three_epochs_per_element(d, adam):
    nf, n, bs = 163, 230, 64  # batches of 64, 64, 64, 38
    idx, val, tgt = R.drift_set(n, nf, bs, seed=d)
    slots = R.batch_slots(idx, val, bs)
    assert len({s[140] for s in slots}) > 1 and all(10 not in s for s in slots[1:]) and all(20 not in s for s in slots[:-1])
    B, W, V = _model(nf, d, d + 7)
    lr, wd = _rates(adam)
    K = K_MULTI[adam]
    prod, step = capi.FM(nf, d), capi.FM(nf, d)
    for h in (prod, step):
        h.set_params(B, W, V)
    prod.set_train(idx, val, tgt)
    ref = R.StepTrainer(B, W, V)
    prev = step.get_params()
    worst = {"step": 0.0, "epoch": 0.0, "ulp": 0, "cost": 0.0}
    for e in range(3):
        c_dev = prod.epoch(bs, _opt(adam), lr, wd)
        c_ref = f32(0)
        for i in range(0, n, bs):
            sl = slice(i, min(i + bs, n))
            zero = [ref.zero_step(k, prev[k], adam, lr, wd) for k in (1, 2)]  # before the reference's moments move
            _step_by_slice(step, idx, val, tgt, sl, adam, lr, wd)
            got = step.get_params()
            c_ref = f32(c_ref + f32(ref.step(idx[sl], val[sl], tgt[sl], adam, lr, wd)))
            clean = ~(ref.ever if adam else ref.touched)
            assert clean[:nf - nf % 16].any() and clean[nf - nf % 16:].any()
            for k, un in ((1, clean), (2, np.repeat(clean, d))):
                mism, ulp, _, _ = R.untouched_report(got[k], zero[k - 1], un)
                assert mism == 0 and ulp <= 1, (e, i, k, mism, ulp)
                worst["ulp"] = max(worst["ulp"], ulp)
            r = R.params_report(got, ref.params, lr, K, ref.slack if adam else None)
            worst["step"] = max(worst["step"], r)
            assert r <= 1, (e, i, r)
            prev = got
        got = prod.get_params()
        r = R.params_report(got, ref.params, lr, K, ref.slack if adam else None)
        worst["epoch"] = max(worst["epoch"], r)
        worst["cost"] = max(worst["cost"], abs(c_dev - c_ref) / (1e-4 * abs(c_ref)))
        assert r <= 1, (e, r)
        assert abs(c_dev - c_ref) <= 1e-4 * abs(c_ref), (c_dev, c_ref)
        assert _same_bits(got, prev), "the production epoch and the batch-by-batch handle took different steps"
    print("three epochs d=%d %s: worst error over bar %s" % (d, "adam" if adam else "sgd", worst))


@pytest.mark.parametrize("adam", [False, True])
def test_handle_life_cycle(adam):
    nf, d = 163, 20
    A = R.drift_set(230, nf, 64, seed=91)
    i2, v2, t2 = R.drift_set(150, nf, 64, seed=92)
    i2 = np.where(v2 != 0, (i2 * 3 + 5) % 157, 0).astype(np.int32)  # other features than A's, 1..9 among them
    assert (R.touched_rows(i2, v2, nf) & ~R.touched_rows(A[0], A[1], nf)).sum() > 5
    lr, wd = _rates(adam)
    K = K_MULTI[adam]
    B, W, V = _model(nf, d, 3)
    fm = capi.FM(nf, d)
    fm.set_params(B, W, V)
    fm.set_train(*A)
    ref = R.StepTrainer(B, W, V)
    worst, steps = [], [0]

    def stage(name, data, bs):
        steps[0] += -(-len(data[2]) // bs)
        c_dev = fm.epoch(bs, _opt(adam), lr, wd)
        c_ref = ref.epoch(*data, bs, adam, lr, wd)
        got = fm.get_params()
        r = R.params_report(got, ref.params, lr, K, ref.slack if adam else None)
        worst.append((name, round(r, 3), round(abs(c_dev - c_ref) / (1e-4 * abs(c_ref)), 3)))
        assert r <= 1, worst
        assert abs(c_dev - c_ref) <= 1e-4 * abs(c_ref), worst
        # rows nothing has touched yet: the reference's zero-gradient steps, bit for bit in the fused body
        clean = ~ref.ever
        assert clean.any()
        for k, un in ((1, clean), (2, np.repeat(clean, d))):
            mism, ulp, n_body, n_tail = R.untouched_report(got[k], ref.params[k], un)
            assert n_body > 0 and n_tail > 0
            assert mism == 0 and ulp <= steps[0], (name, k, mism, ulp, steps[0])
            worst[-1] += (ulp,)

    stage("bs 64", A, 64)
    stage("bs 50", A, 50)   # a smaller batch: the plan is rebuilt, the step clock runs on
    stage("bs 64 again", A, 64)
    fm.set_train(i2, v2, t2)
    stage("second set", (i2, v2, t2), 64)
    B, W, V = _model(nf, d, 4)
    fm.set_params(B, W, V)  # a new Fit: Adam's t restarts at 1, the tags' clock does not
    ref = R.StepTrainer(B, W, V)
    steps[0] = 0
    stage("set_params again", (i2, v2, t2), 64)
    print("life cycle %s: (stage, parameters over bar, cost over bar, tail ulp of W, of V) %s" % ("adam" if adam else "sgd", worst))
