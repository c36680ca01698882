"""numpy restatement of the factorization machine (model/ctr/fm.go without the embedding branch) used by the FM tests:
the forward pass, the loss and its gradient in float64, and the reference's optimizer steps in fp32 with the FMA-body /
unfused-tail rule of common/floats/src/floats_avx512.c."""
import numpy as np

f32, f64 = np.float32, np.float64
BETA1, BETA2, EPS = f32(0.9), f32(0.999), f32(1e-8)


def pad(rows, width=None):
    """[(indices, values)] -> n x width index / value matrices padded with index 0, value 0 (convertToTensors)"""
    width = width or max(1, max(len(r[0]) for r in rows))
    idx = np.zeros((len(rows), width), np.int32)
    val = np.zeros((len(rows), width), np.float32)
    for i, (a, b) in enumerate(rows):
        idx[i, :len(a)] = a
        val[i, :len(b)] = b
    return idx, val


def forward64(B, W, V, idx, val):
    """logits, vx (n x d) and each row's scale |B| + sum|w x| + 0.5 sum (vx^2 + sum v^2 x^2), all float64"""
    Vg = np.asarray(V, f64)[idx]
    x = np.asarray(val, f64)[..., None]
    vx = (Vg * x).sum(1)
    sq = (Vg * Vg * x * x).sum(1)
    wx = np.asarray(W, f64)[idx] * np.asarray(val, f64)
    logit = wx.sum(1) + 0.5 * (vx * vx - sq).sum(1) + f64(B)
    scale = abs(f64(B)) + np.abs(wx).sum(1) + 0.5 * (vx * vx + sq).sum(1)
    return logit, vx, scale


def loss64(B, W, V, idx, val, t):
    p = forward64(B, W, V, idx, val)[0]
    y = (np.asarray(t, f64) + 1) / 2
    return (np.maximum(p, 0) - p * y + np.log1p(np.exp(-np.abs(p)))).mean()


def _contrib64(B, W, V, idx, val, t):
    """every position's share of the gradient: g (n), g x (n x width), g (x vx - v x^2) (n x width x d), the mean loss"""
    p, vx, _ = forward64(B, W, V, idx, val)
    y = (np.asarray(t, f64) + 1) / 2
    g = (1 / (1 + np.exp(-p)) - y) / len(p)
    x = np.asarray(val, f64)
    c = g[:, None, None] * (x[..., None] * vx[:, None, :] - np.asarray(V, f64)[idx] * (x * x)[..., None])
    loss = (np.maximum(p, 0) - p * y + np.log1p(np.exp(-np.abs(p)))).mean()
    return g, g[:, None] * x, c, loss


def grads64(B, W, V, idx, val, t, wW=None, wV=None):
    """(dB, dW, dV, mean loss) of BCEWithLogits averaged over the rows, float64.  wW (n x width) and wV (n x width x d, or
    anything that broadcasts to it) scale single positions' shares of dW / dV on their way into the sums -- the forward pass
    stays as it is: what a kernel that drops, doubles or mis-scales a position of a feature's list would produce."""
    g, cw, c, loss = _contrib64(B, W, V, idx, val, t)
    if wW is not None:
        cw = cw * wW
    if wV is not None:
        c = c * wV
    dW = np.zeros(len(W))
    np.add.at(dW, idx, cw)
    dV = np.zeros(np.shape(V))
    np.add.at(dV, idx, c)
    return g.sum(), dW, dV, loss


def grad_scale64(B, W, V, idx, val, t):
    """(aW, aV): per element the sum of the magnitudes that an fp32 evaluation of dW / dV rounds -- sum_b |g_b x| and
    sum_b |g_b| (|x| sum_j |v_jf x_j| + |v_f| x^2), float64; what forward64's `scale` is to the logit"""
    g, cw, _, _ = _contrib64(B, W, V, idx, val, t)
    x = np.abs(np.asarray(val, f64))
    Va = np.abs(np.asarray(V, f64))[idx]
    avx = (Va * x[..., None]).sum(1)
    c = np.abs(g)[:, None, None] * (x[..., None] * avx[:, None, :] + Va * (x * x)[..., None])
    aW = np.zeros(len(W))
    np.add.at(aW, idx, np.abs(cw))
    aV = np.zeros(np.shape(V))
    np.add.at(aV, idx, c)
    return aW, aV


def fma32(a, b, c):
    """fp32 fused multiply-add, correctly rounded: the exact product in float64, an error-free sum, and the one case where
    rounding the float64 sum to fp32 can differ from rounding the exact sum (a float64 sum exactly halfway between two fp32)"""
    a, b, c = (np.asarray(v, f32).astype(f64) for v in (a, b, c))
    ab = a * b
    s = ab + c
    bb = s - ab
    e = (ab - (s - bb)) + (c - bb)
    r = s.astype(f32)
    r64 = r.astype(f64)
    other = np.where(s > r64, np.nextafter(r, f32(np.inf)), np.nextafter(r, f32(-np.inf)))
    mid = (r64 + other.astype(f64)) / 2
    fix = (s == mid) & (e != 0) & (np.sign(e) == np.sign(other.astype(f64) - r64))
    return np.where(fix, other, r).astype(f32)


def pow32(x, y):
    """math32.Pow for a positive integer y, in fp32 (square-and-multiply on the Frexp mantissa)"""
    x1, xe = np.frexp(f32(x))
    x1, xe = f32(x1), int(xe)
    a1, ae, i = f32(1), 0, int(y)
    while i:
        if i & 1:
            a1 = f32(a1 * x1)
            ae += xe
        x1 = f32(x1 * x1)
        xe <<= 1
        if x1 < 0.5:
            x1 = f32(x1 + x1)
            xe -= 1
        i >>= 1
    return f32(np.ldexp(a1, ae))


def adam_lr(alpha, t):
    fix1 = f32(1) - pow32(BETA1, t)
    fix2 = f32(1) - pow32(BETA2, t)
    return f32(f32(f32(alpha) * np.sqrt(fix2)) / fix1)


def opt_step32(p, g, m, v, wd, lr, adam):
    """one nn.SGD / nn.Adam step of one flat tensor in fp32 (optimizers.go:70-84, 118-156); lr is Adam's lr_t"""
    p, g, m, v = (np.asarray(a, f32).reshape(-1) for a in (p, g, m, v))
    L = p.size
    body = np.arange(L) < L - L % 16
    wd, lr = f32(wd), f32(lr)

    def mca(a, c, dst):  # floats.MulConstAdd(To): dst + a * c, fused in the 16-lane body
        return np.where(body, fma32(a, np.full(L, c, f32), dst), (dst + a * c).astype(f32))

    b1 = mca(p, wd, g)
    if not adam:
        return mca(b1, -lr, p), m, v
    b2 = (b1 - m).astype(f32)
    m = mca(b2, f32(1) - BETA1, m)
    b2 = (b1 * b1 - v).astype(f32)
    v = mca(b2, f32(1) - BETA2, v)
    q = (m / (np.sqrt(v) + EPS)).astype(f32)
    return mca(q, -lr, p), m, v


class Trainer:
    """AFM.Fit's epoch loop restated: fp32 parameters and moments, float64 gradients rounded to fp32, fp32 steps"""

    def __init__(self, B, W, V):
        self.p = [np.array([B], f32), np.asarray(W, f32).reshape(-1).copy(), np.asarray(V, f32).copy()]
        self.m = [np.zeros_like(x).reshape(-1) for x in self.p]
        self.v = [np.zeros_like(x).reshape(-1) for x in self.p]
        self.t = 0

    @property
    def params(self):
        return self.p[0][0], self.p[1], self.p[2]

    def epoch(self, idx, val, tgt, bs, adam, lr, wd):
        cost = f32(0)
        for i in range(0, len(tgt), bs):
            sl = slice(i, min(i + bs, len(tgt)))
            dB, dW, dV, loss = grads64(self.p[0][0], self.p[1], self.p[2], idx[sl], val[sl], tgt[sl])
            cost = f32(cost + f32(loss))
            if adam:
                self.t += 1
            lr_t = adam_lr(lr, self.t) if adam else f32(lr)
            for k, gk in enumerate((np.array([dB]), dW, dV)):
                shape = self.p[k].shape
                p, self.m[k], self.v[k] = opt_step32(self.p[k], np.asarray(gk, f32), self.m[k], self.v[k], wd, lr_t, adam)
                self.p[k] = p.reshape(shape)
        return cost


def auc(pos, neg):
    """model/ctr/evaluator.go AUC in float64 bookkeeping (the tests compare it with a tolerance)"""
    pos, neg = np.sort(pos), np.sort(neg)
    return float(np.searchsorted(neg, pos, side="left").sum()) / (len(pos) * len(neg))


def synth_ctr(n, nf, d, seed, wmin=3, wmax=12):
    """rows of distinct features with widths in [wmin, wmax], values mostly 1 (a few numeric), +-1 targets drawn from a
    planted FM with logistic noise; returns (idx, val, tgt) padded to wmax"""
    rng = np.random.default_rng(seed)
    Wt = rng.normal(0, 0.5, nf)
    Vt = rng.normal(0, 0.3, (nf, d))
    rows = []
    for _ in range(n):
        k = rng.integers(wmin, wmax + 1)
        a = rng.choice(nf, k, replace=False).astype(np.int32)
        b = np.where(rng.random(k) < 0.2, rng.normal(1, 0.5, k), 1.0).astype(np.float32)
        rows.append((a, b))
    idx, val = pad(rows, wmax)
    logit = forward64(0.0, Wt, Vt, idx, val)[0]
    tgt = np.where(rng.random(n) < 1 / (1 + np.exp(-logit)), 1.0, -1.0).astype(np.float32)
    return idx, val, tgt


# ---- training at every kernel shape: generators, a step-by-step trainer, the per-element comparison ------------------------

# largest divergence of the fp32-step reference (StepTrainer) from its all-float64 run, as |a - b| / (|b| + lr), over the
# schedules of test_gpu_fm_train_shapes.py (test_fm_cpu.py measures it again), and the multi-step bar: 4 x that
DIVERGENCE = {False: 4.3e-7, True: 3.8e-6}  # SGD, Adam: 4.22e-7 and 3.70e-6 measured, rounded up
K_MULTI = {adam: 4 * v for adam, v in DIVERGENCE.items()}
U_ACC = 4  # positions per lane group and trip of fm_accum_kernel's loop


def lanes_for(d):
    """lanes per sample of fm_forward_kernel / fm_accum_kernel (two factors per lane above 64)"""
    g = 8
    while g < d and g < 64:
        g *= 2
    return g


def trip(d):
    """positions of a feature's list that one trip of the accumulate loop takes: U x NG, NG = 64 / lanes"""
    return U_ACC * (64 // lanes_for(d))


def rows_of(idx, val, f):
    """rows in which feature f holds a nonzero value (what the batch plan lists for it)"""
    return np.flatnonzero(((idx == f) & (val != 0)).sum(1))


def touched_rows(idx, val, nf):
    t = np.zeros(nf, bool)
    t[np.unique(idx[val != 0])] = True
    return t


def shape_batch(d, nf, n, seed):
    """One batch for a one-step check at d factors.  With T = trip(d): feature 7 in every row, features 1 / 2 / 4 in exactly
    T / T + 1 / 2 T - 1 rows, feature 0 as a real feature in every sixth row, eight features in one row each (three of them
    sharing row 5, one of them nf - 2: inside the tail of W and V), one to four random others per row (a row with a single
    feature has no share in dV at all); features with id % 5 == 3 and feature nf - 1 are never used; every row ends in
    padding, and the features of a row are shuffled.
    Returns (idx, val, tgt, lists): lists maps the features with a promised count to that count.  Raises where the batch is too
    small for the promise."""
    T = trip(d)
    if n < 2 * T - 1 or n < 12 or nf < 60 or (nf - 2) % 5 == 3:
        raise ValueError("shape_batch: n = %d rows / nf = %d features cannot hold lists of %d positions" % (n, nf, 2 * T - 1))
    rng = np.random.default_rng(seed)
    lists = {7: n, 1: T, 2: T + 1, 4: 2 * T - 1, 0: len(range(0, n, 6))}
    single = [nf - 2] + [f for f in range(nf - 3, 0, -1) if f % 5 != 3][:7]
    single_row = dict(zip(single, [5, 5, 5, 0, 1, 2, 9, 11]))
    lists.update({f: 1 for f in single})
    member = {f: set() for f in lists}
    member[7] = set(range(n))
    member[0] = set(range(0, n, 6))
    for f in (1, 2, 4):
        member[f] = set(rng.choice(n, lists[f], replace=False).tolist())
    for f, r in single_row.items():
        member[f] = {r}
    pool = np.array([f for f in range(nf - 1) if f % 5 != 3 and f not in lists])
    rows = []
    for r in range(n):
        a = [f for f in lists if r in member[f]]
        a += rng.choice(pool, int(rng.integers(1, 5)), replace=False).tolist()
        a = np.array(a, np.int32)[rng.permutation(len(a))]
        b = np.where(rng.random(len(a)) < 0.3, rng.normal(1, 0.5, len(a)), 1.0)
        b = np.where(np.abs(b) < 0.1, 1.0, b).astype(np.float32)
        rows.append((a, b))
    idx, val = pad(rows, max(len(a) for a, _ in rows) + 2)
    tgt = np.where(rng.random(n) < 0.5, 1.0, -1.0).astype(np.float32)
    for f, c in lists.items():
        if len(rows_of(idx, val, f)) != c:
            raise ValueError("shape_batch: feature %d is in %d rows, promised %d" % (f, len(rows_of(idx, val, f)), c))
    return idx, val, tgt, lists


def drift_set(n, nf, bs, seed):
    """A small training set for several epochs of ceil(n / bs) batches (the last one partial).  Features 10..19 only in batch 0,
    20..29 only in the last batch, 100 / 120 / 140 in every batch (140 in every row) -- their slot, the rank among the features
    the batch touches, changes from batch to batch because each batch draws its other features from its own part of the ids;
    feature 0 is a real feature; ids from nf - 6 on are never used.  Returns (idx, val, tgt)."""
    nb = -(-n // bs)
    if nb < 3 or n % bs == 0 or nf < 160:
        raise ValueError("drift_set: wants >= 3 batches, a partial last batch and nf >= 160")
    rng = np.random.default_rng(seed)
    rows = []
    for r in range(n):
        k = r // bs
        lo = 30 + (k * 17) % 60  # each batch's own window of the common ids
        a = [140] + rng.choice(np.arange(lo, lo + 40 + 9 * k), int(rng.integers(1, 5)), replace=False).tolist()
        a = [f for f in a if f not in (100, 120)]
        if r % bs < 3 or rng.random() < 0.1:
            a += [100, 120]
        if k == 0:
            a.append(10 + r % 10)
        if k == nb - 1:
            a.append(20 + r % 10)
        if r % 7 == 0:
            a.append(0)
        if rng.random() < 0.3:
            a.append(int(rng.integers(141, nf - 6)))
        a = np.array(sorted(set(a)), np.int32)[rng.permutation(len(set(a)))]
        b = np.where(rng.random(len(a)) < 0.3, rng.normal(1, 0.5, len(a)), 1.0)
        rows.append((a, np.where(np.abs(b) < 0.1, 1.0, b).astype(np.float32)))
    idx, val = pad(rows, max(len(a) for a, _ in rows) + 1)
    tgt = np.where(rng.random(n) < 0.5, 1.0, -1.0).astype(np.float32)
    return idx, val, tgt


def batch_slots(idx, val, bs):
    """per batch {feature: slot}: the feature's rank among the features the batch touches, ascending (the batch plan's order)"""
    out = []
    for i in range(0, len(idx), bs):
        u = np.unique(idx[i:i + bs][val[i:i + bs] != 0])
        out.append({int(f): s for s, f in enumerate(u)})
    return out


def opt_step64(p, g, m, v, wd, lr, adam):
    """opt_step32's step in float64 throughout (the same constants, no fp32 rounding anywhere)"""
    p, g, m, v = (np.asarray(a, f64).reshape(-1) for a in (p, g, m, v))
    b1 = g + p * f64(f32(wd))
    if not adam:
        return p - lr * b1, m, v
    m = m + (b1 - m) * f64(f32(1) - BETA1)
    v = v + (b1 * b1 - v) * f64(f32(1) - BETA2)
    return p - lr * (m / (np.sqrt(v) + f64(EPS))), m, v


class StepTrainer:
    """Trainer one step at a time: step() takes one batch, so a caller can look at the parameters (and at which rows the
    batch touched) between steps; t is nn.Adam's step count so far.  dtype float32 is Trainer's arithmetic (float64 gradients
    rounded to fp32, opt_step32); dtype float64 runs the same schedule without any fp32 rounding (opt_step64), the measure of
    what fp32 steps alone move a parameter by."""

    def __init__(self, B, W, V, t=0, dtype=f32):
        self.dt = dtype
        self.p = [np.array([B], dtype), np.asarray(W, dtype).reshape(-1).copy(), np.asarray(V, dtype).copy()]
        self.m = [np.zeros(x.size, dtype) for x in self.p]
        self.v = [np.zeros(x.size, dtype) for x in self.p]
        self.t = t
        self.touched = np.zeros(len(self.p[1]), bool)       # rows the last step touched
        self.ever = np.zeros(len(self.p[1]), bool)          # rows any step touched
        # Adam only, per element of (B, W, V): what gradients that each sit within their bar of 1e-5 grad_scale64 may have moved
        # the parameter by so far -- per step lr_t (1 - beta1) 1e-5 grad_scale64 / (sqrt(v) + eps), the step's derivative to its
        # gradient with v held (at the first step, lr 1e-5 grad_scale64 / (|b1| + 3.2e-7), above the exact derivative).  Adam
        # divides by sqrt(v): where grad + wd p has been all but zero so far, a rounding error of the gradient decides the step.
        self.slack = [np.zeros(x.size) for x in self.p]

    @property
    def params(self):
        return self.p[0][0], self.p[1], self.p[2]

    def lr_t(self, adam, lr, t):
        # the float64 run takes the fp32 lr_t too: a host-side scalar (the library forms it with the same fp32 steps); in float64
        # it differs by up to 3e-5 relative (the cancellation in 1 - beta2^t), which is no property of the per-element steps
        return self.dt(adam_lr(lr, t) if adam else f32(lr))

    def zero_step(self, k, p_prev, adam, lr, wd):
        """tensor k (0 B, 1 W, 2 V) after the NEXT step if its gradient were zero, from p_prev and this trainer's moments"""
        step = opt_step32 if self.dt == f32 else opt_step64
        z = np.zeros(self.p[k].size, self.dt)
        return step(p_prev, z, self.m[k], self.v[k], wd, self.lr_t(adam, lr, self.t + 1 if adam else self.t), adam)[0]

    def step(self, idx, val, tgt, adam, lr, wd, wW=None, wV=None):
        old = (self.p[0][0], self.p[1], self.p[2])
        dB, dW, dV, loss = grads64(*old, idx, val, tgt, wW, wV)
        if adam:
            self.t += 1
        lr_t = self.lr_t(adam, lr, self.t)
        step = opt_step32 if self.dt == f32 else opt_step64
        for k, gk in enumerate((np.array([dB]), dW, dV)):
            shape = self.p[k].shape
            p, self.m[k], self.v[k] = step(self.p[k], np.asarray(gk, self.dt), self.m[k], self.v[k], wd, lr_t, adam)
            self.p[k] = p.reshape(shape)
        if adam:
            aW, aV = grad_scale64(*old, idx, val, tgt)
            aB = np.abs(_contrib64(*old, idx, val, tgt)[0]).sum()
            for k, a in enumerate((np.array([aB]), aW, aV.reshape(-1))):
                self.slack[k] += f64(lr_t) * f64(f32(1) - BETA1) * 1e-5 * a / (np.sqrt(self.v[k].astype(f64)) + f64(EPS))
        self.touched = touched_rows(idx, val, len(self.p[1]))
        self.ever |= self.touched
        return loss

    def epoch(self, idx, val, tgt, bs, adam, lr, wd):
        cost = f32(0)
        for i in range(0, len(tgt), bs):
            cost = f32(cost + f32(self.step(idx[i:i + bs], val[i:i + bs], tgt[i:i + bs], adam, lr, wd)))
        return cost


def ulp_diff(a, b):
    a, b = (np.asarray(x, f32).reshape(-1).view(np.int32).astype(np.int64) for x in (a, b))
    return np.abs(a - b)


def untouched_report(got, want, un):
    """(bit mismatches among the untouched elements of the fused body, worst ulp distance among those of the unfused tail,
    untouched elements in the body, in the tail) of one flat tensor"""
    got, want = np.asarray(got, f32).reshape(-1), np.asarray(want, f32).reshape(-1)
    L = got.size
    body = np.arange(L) < L - L % 16
    ub, ut = un & body, un & ~body
    mism = int((got[ub].view(np.uint32) != want[ub].view(np.uint32)).sum())
    return mism, int(ulp_diff(got[ut], want[ut]).max()) if ut.any() else 0, int(ub.sum()), int(ut.sum())


def straddles(un, group=4):
    """aligned groups of `group` elements that hold untouched and touched elements at once"""
    L = un.size - un.size % group
    g = un[:L].reshape(-1, group)
    return int((g.any(1) & ~g.all(1)).sum())


def one_step_report(B, W, V, idx, val, tgt, got, cost, adam, lr, wd, wW=None, wV=None):
    """Everything test_gpu_fm_train_shapes.py asserts of one step from (B, W, V) on one batch, as figures; got = (B, W, V) after
    the step, cost = the epoch's cost.  Ratios are error / bar (<= 1 passes):
      cost      |cost - loss| / (1e-5 loss)
      B, W, V   touched elements (B always): |got - ref| / (1e-5 (|ref| + lr)), ref = opt_step32 of the float64 gradient
      W_ill, V_ill   Adam only: (elements, touched elements, worst ratio) of the touched elements that no gradient within its
                bar can hold to that bar.  Adam's first step is p - lr b1 / (|b1| + e), b1 = grad + wd p, e = eps / sqrt(1 -
                beta2) = 3.2e-7: it turns a gradient error dg into lr dg e / (|b1| + e)^2.  An element is counted here when
                that amount for dg = the gradient bar (1e-5 grad_scale64 + 2^-23 (|g| + wd |p0|), as under gW / gV) exceeds
                1e-5 (|ref| + lr) -- b1 all but cancels, and its sign is a rounding error's -- and is held to the sum of the
                two instead; W, V then cover every other touched element.
      W_unt, V_unt   untouched_report() against the zero-gradient step
      gW, gV    SGD only: the gradient the step carried, (p0 - got) / lr - wd p0, against the float64 gradient, over the
                bar 1e-5 grad_scale64 + 2^-23 (|got| / lr + |g| + wd |p0|) (the second term: got and b1 are rounded to fp32)
      straddle  float4 groups of V with touched and untouched elements
    wW / wV perturb the reference's sums (grads64)."""
    nf, d = np.shape(V)
    dB, dW, dV, loss = grads64(B, W, V, idx, val, tgt, wW, wV)
    aW, aV = grad_scale64(B, W, V, idx, val, tgt)
    lr_t = adam_lr(lr, 1) if adam else f32(lr)
    touched = touched_rows(idx, val, nf)
    rep = {"cost": abs(cost - loss) / (1e-5 * loss)}
    gB = got[0]
    refB = opt_step32(np.array([B]), np.array([dB], f32), np.zeros(1, f32), np.zeros(1, f32), wd, lr_t, adam)[0][0]
    rep["B"] = abs(f64(gB) - f64(refB)) / (1e-5 * (abs(f64(refB)) + lr))
    for name, p0, g64, a64, gp, row_of in (("W", W, dW, aW, got[1], np.arange(nf)),
                                           ("V", V, dV, aV, got[2], np.arange(nf * d) // d)):
        p0, g64, a64, gp = (np.asarray(x).reshape(-1) for x in (p0, g64, a64, gp))
        zero = np.zeros(p0.size, f32)
        ref_un = opt_step32(p0, zero, zero, zero, wd, lr_t, adam)[0]
        ref_t = opt_step32(p0, g64.astype(f32), zero, zero, wd, lr_t, adam)[0]
        un = ~touched[row_of]
        rep[name + "_unt"] = untouched_report(gp, ref_un, un)
        t = ~un
        err = np.abs(gp.astype(f64) - ref_t)
        flat = 1e-5 * (np.abs(ref_t.astype(f64)) + lr)
        lr64, wd64, p64, q64 = f64(f32(lr)), f64(f32(wd)), p0.astype(f64), gp.astype(f64)
        if adam:
            e = f64(EPS) / np.sqrt(f64(f32(1) - BETA2))
            gbar = 1e-5 * a64 + 2.0 ** -23 * (np.abs(g64) + wd64 * np.abs(p64))
            prop = lr64 * gbar * e / (np.abs(g64 + wd64 * p64) + e) ** 2
            ill = t & (prop > flat)
            rep[name + "_ill"] = (int(ill.sum()), int(t.sum()), float(np.max(err[ill] / (flat + prop)[ill])) if ill.any() else 0.0)
            t = t & ~ill
        rep[name] = float(np.max(err[t] / flat[t]))
        if not adam:
            carried = (p64 - q64) / lr64 - wd64 * p64
            bar = 1e-5 * a64 + 2.0 ** -23 * (np.abs(q64) / lr64 + np.abs(g64) + wd64 * np.abs(p64))
            rep["g" + name] = float(np.max(np.abs(carried[t] - g64[t]) / bar[t]))
        if name == "V":
            rep["straddle"] = straddles(un)
    return rep


SLACK_CAP = 16  # StepTrainer.slack counts up to this many multiples of k (|ref| + lr)


def params_report(got, ref, lr, k, slack=None):
    """worst |got - ref| / (k (|ref| + lr) + min(slack, SLACK_CAP k (|ref| + lr))) over B, W, V: the multi-step comparison"""
    worst = 0.0
    for i, (g, r) in enumerate(zip(got, ref)):
        g, r = np.asarray(g, f64).reshape(-1), np.asarray(r, f64).reshape(-1)
        bar = k * (np.abs(r) + lr)
        if slack is not None:
            bar = bar + np.minimum(slack[i], SLACK_CAP * bar)
        worst = max(worst, float(np.max(np.abs(g - r) / bar)))
    return worst
