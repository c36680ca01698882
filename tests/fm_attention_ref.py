"""numpy restatement of ctr.AFM's item-embedding branch (model/ctr/fm.go:127-132; nn.Attention and nn.Linear,
common/nn/layers.go:36-60, 160-190) on top of fm_ref.py, used by the attention tests.

The reference's Softmax (common/nn/op.go:760-777) applies the row maxima and row sums through Tensor.sub / Tensor.div /
Tensor.mul (tensor.go:328-379), which index their (n x 1) operand by flat index % n: element (r, c) of an n x D matrix uses
entry (r D + c) % n.  softmax_fwd / softmax_bwd restate exactly that, vectorised; softmax_*_literal transcribe the loops one
by one (float32) so that the vectorised form can be pinned to them; row_softmax is the mathematically usual one, kept only
to show that the two differ."""
import numpy as np

import fm_ref as R

f32, f64 = np.float32, np.float64


# ---- bf16 ---------------------------------------------------------------------------------------------------------
def to_bf16(x):
    """float -> bf16 bit patterns (uint16), round to nearest even"""
    b = np.ascontiguousarray(x, f32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) >> 16
    return b.astype(np.uint16)


def from_bf16(bits, dtype=f64):
    return (np.ascontiguousarray(bits, np.uint16).astype(np.uint32) << 16).view(f32).astype(dtype)


# ---- the reference's Softmax ------------------------------------------------------------------------------------------
def wrap_index(n, D):
    return (np.arange(n * D) % n).reshape(n, D)


def _seqsum(a):
    """row sums added left to right in a's own precision (Tensor.sum, tensor.go:697-734)"""
    return np.cumsum(a, axis=1)[:, -1]


def _exp(y):
    """Tensor.exp (tensor.go:414-419): float32(math.Exp(float64(x)))"""
    return np.exp(y.astype(f64)).astype(y.dtype)


def softmax_fwd(s):
    n, D = s.shape
    w = wrap_index(n, D)
    e = _exp(s - s.max(1)[w])
    return e / _seqsum(e)[w]


def softmax_bwd(a, da):
    n, D = a.shape
    gx = a * da
    return gx - a * _seqsum(gx)[wrap_index(n, D)]


def row_softmax(s):
    e = np.exp(s - s.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def _reduce_literal(data, n, D, op):
    out = np.zeros(n, f32)
    for i in range(n):
        v = data[i * D]
        for k in range(1, D):
            v = op(v, data[i * D + k])
        out[i] = v
    return out


def softmax_fwd_literal(s):
    """op.go:760-767 with tensor.go's sub / exp / div / max / sum written out loop by loop, float32"""
    n, D = s.shape
    x = np.asarray(s, f32).reshape(-1)
    y = x.copy()
    mx = _reduce_literal(x, n, D, max)  # x.max(axis, keepDim): shape (n, 1), wSize = n
    for i in range(y.size):
        y[i] = f32(y[i] - mx[i % n])
    for i in range(y.size):
        y[i] = f32(np.exp(f64(y[i])))
    sm = _reduce_literal(y, n, D, lambda p, q: f32(p + q))
    for i in range(y.size):
        y[i] = f32(y[i] / sm[i % n])
    return y.reshape(n, D)


def softmax_bwd_literal(a, da):
    """op.go:769-777: gx = y * dy; sumdx = gx.sum(axis, keepDim); y.mul(sumdx); gx.sub(y)"""
    n, D = a.shape
    y = np.asarray(a, f32).reshape(-1).copy()
    dy = np.asarray(da, f32).reshape(-1)
    gx = y.copy()
    for i in range(gx.size):
        gx[i] = f32(gx[i] * dy[i])
    sumdx = _reduce_literal(gx, n, D, lambda p, q: f32(p + q))
    for i in range(y.size):
        y[i] = f32(y[i] * sumdx[i % n])
    for i in range(gx.size):
        gx[i] = f32(gx[i] - y[i])
    return gx.reshape(n, D)


# ---- the branch ---------------------------------------------------------------------------------------------------------
NAMES = ("H", "Wa", "ba", "We", "be")  # Parameters() order of one field (fm.go:136-146, layers.go:173-178)


def init_field(rng, D, d, h_sd=0.01):
    """AFM.Init's draws: H ~ Normal(0, 0.01), Wa, We ~ Uniform(+-1/sqrt(D)), biases 0 -> (H, Wa, ba, We, be) float32"""
    b = 1 / np.sqrt(D)
    return (rng.normal(0, h_sd, (d, D)).astype(f32), rng.uniform(-b, b, (D, d)).astype(f32), np.zeros(d, f32),
            rng.uniform(-b, b, (D, d)).astype(f32), np.zeros(d, f32))


def branch_fwd(field, x, softmax=softmax_fwd):
    """x: n x D in the working precision -> dict of every intermediate"""
    H, Wa, ba, We, be = (np.asarray(t, x.dtype) for t in field)
    pre = x @ Wa + ba
    h = np.maximum(pre, 0)
    s = h @ H
    a = softmax(s)
    z = a * x
    enc = z @ We + be
    return dict(x=x, pre=pre, h=h, s=s, a=a, z=z, enc=enc)


def forward(B, W, V, fields, idx, val, embs, dtype=f64, softmax=softmax_fwd):
    """logits of ONE batch (the softmax makes the batch part of the result), each row's scale, and the caches.
    The factorization machine's own part is always float64; dtype is the branch's working precision."""
    logit, vx, scale = R.forward64(B, W, V, idx, val)
    caches = []
    for field, bits in zip(fields, embs):
        c = branch_fwd(field, from_bf16(bits, dtype), softmax)
        logit = logit + (vx.astype(dtype) * c["enc"]).sum(1).astype(f64)
        We, be = np.abs(np.asarray(field[3], f64)), np.abs(np.asarray(field[4], f64))
        scale = scale + (np.abs(vx) * (np.abs(c["z"].astype(f64)) @ We + be)).sum(1)
        caches.append(c)
    return logit, vx, scale, caches


def predict(B, W, V, fields, idx, val, embs, batch_size, dtype=f64, softmax=softmax_fwd):
    """BatchInternalPredict (fm.go:156-178): slices of batch_size rows -> (logits, scales)"""
    out, sc = [], []
    for i in range(0, len(idx), batch_size):
        sl = slice(i, min(i + batch_size, len(idx)))
        lg, _, s, _ = forward(B, W, V, fields, idx[sl], val[sl], [e[sl] for e in embs], dtype, softmax)
        out.append(lg)
        sc.append(s)
    return np.concatenate(out), np.concatenate(sc)


def loss(B, W, V, fields, idx, val, embs, t):
    p = forward(B, W, V, fields, idx, val, embs)[0]
    y = (np.asarray(t, f64) + 1) / 2
    return (np.maximum(p, 0) - p * y + np.log1p(np.exp(-np.abs(p)))).mean()


def grads(B, W, V, fields, idx, val, embs, t, dtype=f64):
    """(dB, dW, dV, [(dH, dWa, dba, dWe, dbe) per field], mean loss) of BCEWithLogits averaged over the batch"""
    p, vx, _, caches = forward(B, W, V, fields, idx, val, embs, dtype)
    y = (np.asarray(t, f64) + 1) / 2
    g = (1 / (1 + np.exp(-p)) - y) / len(p)
    gd, vxd = g.astype(dtype), vx.astype(dtype)
    fgrads, esum = [], np.zeros_like(vx)
    for field, c in zip(fields, caches):
        H, Wa, ba, We, be = (np.asarray(a, dtype) for a in field)
        esum += c["enc"].astype(f64)
        denc = gd[:, None] * vxd
        dWe, dbe = c["z"].T @ denc, denc.sum(0)
        da = (denc @ We.T) * c["x"]
        ds = softmax_bwd(c["a"], da)
        dH = c["h"].T @ ds
        dpre = (c["pre"] > 0) * (ds @ H.T)
        fgrads.append((dH, c["x"].T @ dpre, dpre.sum(0), dWe, dbe))
    x = np.asarray(val, f64)
    dW = np.zeros(len(W))
    np.add.at(dW, idx, g[:, None] * x)
    # d logit / d vx = vx + sum of the fields' enc
    cc = g[:, None, None] * (x[..., None] * (vx + esum)[:, None, :] - np.asarray(V, f64)[idx] * (x * x)[..., None])
    dV = np.zeros(np.shape(V))
    np.add.at(dV, idx, cc)
    lossv = (np.maximum(p, 0) - p * y + np.log1p(np.exp(-np.abs(p)))).mean()
    return g.sum(), dW, dV, fgrads, lossv


class Trainer:
    """AFM.Fit's epoch loop with embedding fields: fp32 parameters and moments, float64 gradients rounded to fp32, the
    reference's fp32 steps (fm_ref.opt_step32), every tensor on its own, in Parameters() order"""

    def __init__(self, B, W, V, fields):
        self.p = [np.array([B], f32), np.asarray(V, f32).copy(), np.asarray(W, f32).reshape(-1).copy()]
        for fld in fields:
            self.p += [np.asarray(a, f32).copy() for a in fld]
        self.m = [np.zeros(x.size, f32) for x in self.p]
        self.v = [np.zeros(x.size, f32) for x in self.p]
        self.t = 0

    @property
    def params(self):
        return self.p[0][0], self.p[2], self.p[1]

    @property
    def fields(self):
        return [tuple(self.p[3 + 5 * k:8 + 5 * k]) for k in range((len(self.p) - 3) // 5)]

    def step(self, idx, val, embs, tgt, adam, lr, wd):
        B, W, V = self.params
        dB, dW, dV, fg, lossv = grads(B, W, V, self.fields, idx, val, embs, tgt)
        if adam:
            self.t += 1
        lr_t = R.adam_lr(lr, self.t) if adam else f32(lr)
        gl = [np.array([dB]), dV, dW] + [a for fld in fg for a in fld]
        for k, gk in enumerate(gl):
            shape = self.p[k].shape
            p, self.m[k], self.v[k] = R.opt_step32(self.p[k], np.asarray(gk, f32), self.m[k], self.v[k], wd, lr_t, adam)
            self.p[k] = p.reshape(shape)
        return lossv

    def epoch(self, idx, val, embs, tgt, bs, adam, lr, wd):
        cost = f32(0)
        for i in range(0, len(tgt), bs):
            sl = slice(i, min(i + bs, len(tgt)))
            cost = f32(cost + f32(self.step(idx[sl], val[sl], [e[sl] for e in embs], tgt[sl], adam, lr, wd)))
        return cost
