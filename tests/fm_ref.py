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


def grads64(B, W, V, idx, val, t):
    """(dB, dW, dV, mean loss) of BCEWithLogits averaged over the rows, float64"""
    p, vx, _ = forward64(B, W, V, idx, val)
    y = (np.asarray(t, f64) + 1) / 2
    g = (1 / (1 + np.exp(-p)) - y) / len(p)
    x = np.asarray(val, f64)
    dW = np.zeros(len(W))
    np.add.at(dW, idx, g[:, None] * x)
    c = g[:, None, None] * (x[..., None] * vx[:, None, :] - np.asarray(V, f64)[idx] * (x * x)[..., None])
    dV = np.zeros(np.shape(V))
    np.add.at(dV, idx, c)
    loss = (np.maximum(p, 0) - p * y + np.log1p(np.exp(-np.abs(p)))).mean()
    return g.sum(), dW, dV, loss


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
