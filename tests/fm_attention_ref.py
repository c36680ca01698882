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
    """(dB, dW, dV, [(dH, dWa, dba, dWe, dbe) per field], mean loss) of BCEWithLogits averaged over the batch: grads_ex's"""
    G = grads_ex(B, W, V, fields, idx, val, embs, t, dtype)
    return G["dB"], G["dW"], G["dV"], G["fg"], G["loss"]


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


# ---- the per-element yardstick: gradients with their scales, planted faults, a step trainer, reports ------------------------
# Planted faults (CPU tests only), fault = (kind, arg):
#   ("row_softmax", None)     the usual row softmax, forward and backward, instead of the wrapped one
#   ("full_modulus", N)       maxima, sums and sumdx indexed by (r D + c) % N (the full batch size) instead of % the batch's own
#                             row count; an index past the batch's rows wraps once more (a kernel would read a stale entry)
#   ("lost_row", r)           row r left out of dH, dWa and dWe (the bias sums keep it)
#   ("no_bias", "ba" | "be")  that bias gradient is zero
#   ("no_relu", None)         dpre = dh, the gate ignored
#   ("lost_col", c)           column c left out of dH, dWa and dWe in every field that has it
#   ("esum_first", None)      only field 0's enc enters dV's vx + esum
#   ("shared_gx", k)          field k forms dH and dpre from the buffer field k - 1 left its ds in (read with field k's stride)
def _wrap(n, D, N=None):
    return ((np.arange(n * D) % (N or n)) % n).reshape(n, D)


def _softmax_pair(fault):
    kind, arg = fault or (None, None)
    if kind == "row_softmax":
        return row_softmax, lambda a, da: a * da - a * (a * da).sum(1, keepdims=True)
    if kind == "full_modulus":
        def fwd(s):
            w = _wrap(*s.shape, arg)
            e = _exp(s - s.max(1)[w])
            return e / _seqsum(e)[w]

        def bwd(a, da):
            gx = a * da
            return gx - a * _seqsum(gx)[_wrap(*a.shape, arg)]
        return fwd, bwd
    return softmax_fwd, softmax_bwd


def grads_ex(B, W, V, fields, idx, val, embs, t, dtype=f64, fault=None):
    """grads() with a planted fault and with every gradient's scale: dict of dB, dW, dV, fg (per field dH, dWa, dba, dWe, dbe),
    loss, and aB, aW, aV, fs in the same shapes: per element the sum of the magnitudes an fp32 evaluation of that gradient
    rounds (fm_ref.grad_scale64's meaning).  Upstream quantities enter by their own magnitude sums: denc by |g| sum_j |v x|,
    dz = denc We^T by A_denc |We|^T, da by A_dz |x|, gx by |a| A_da, ds by A_gx + |a| (row sums of A_gx)[wrapped], dpre by the
    gated A_ds |H|^T.  The scales are float64 and never carry a fault."""
    kind, arg = fault or (None, None)
    sfwd, sbwd = _softmax_pair(fault)
    p, vx, _, caches = forward(B, W, V, fields, idx, val, embs, dtype, sfwd)
    n = len(p)
    y = (np.asarray(t, f64) + 1) / 2
    g = (1 / (1 + np.exp(-p)) - y) / n
    gd, vxd = g.astype(dtype), vx.astype(dtype)
    x = np.asarray(val, f64)
    Va = np.abs(np.asarray(V, f64))[idx]
    avx = (Va * np.abs(x)[..., None]).sum(1)
    A_denc = np.abs(g)[:, None] * avx
    keep = np.ones((n, 1), dtype)
    if kind == "lost_row":
        keep[arg] = 0
    fg, fs, esum, A_esum, prev_ds = [], [], np.zeros_like(vx), np.zeros_like(vx), None
    for k, (field, c) in enumerate(zip(fields, caches)):
        H, Wa, ba, We, be = (np.asarray(a, dtype) for a in field)
        D = H.shape[1]
        if not (kind == "esum_first" and k > 0):
            esum += c["enc"].astype(f64)
        denc = gd[:, None] * vxd
        dWe, dbe = (c["z"] * keep).T @ denc, denc.sum(0)
        da = (denc @ We.T) * c["x"]
        ds = own = sbwd(c["a"], da)
        if kind == "shared_gx" and k == arg:
            flat = np.zeros(n * D, dtype)
            m = min(n * D, prev_ds.size)
            flat[:m] = prev_ds.reshape(-1)[:m]
            ds = flat.reshape(n, D)
        prev_ds = own
        dH = (c["h"] * keep).T @ ds
        dh = ds @ H.T
        dpre = dh if kind == "no_relu" else (c["pre"] > 0) * dh
        dWa, dba = (c["x"] * keep).T @ dpre, dpre.sum(0)
        if kind == "no_bias":
            dba, dbe = (np.zeros_like(dba), dbe) if arg == "ba" else (dba, np.zeros_like(dbe))
        if kind == "lost_col" and arg < D:
            dH[:, arg], dWa[arg], dWe[arg] = 0, 0, 0
        fg.append((dH, dWa, dba, dWe, dbe))
        xa, aa, ha, za = (np.abs(c[q].astype(f64)) for q in ("x", "a", "h", "z"))
        Ha, Wea, bea = (np.abs(np.asarray(q, f64)) for q in (field[0], field[3], field[4]))
        A_gx = aa * ((A_denc @ Wea.T) * xa)
        A_ds = A_gx + aa * A_gx.sum(1)[_wrap(n, D)]
        A_dpre = (c["pre"] > 0) * (A_ds @ Ha.T)
        fs.append((ha.T @ A_ds, xa.T @ A_dpre, A_dpre.sum(0), za.T @ A_denc, A_denc.sum(0)))
        A_esum += za @ Wea + bea
    dW, aW = np.zeros(len(W)), np.zeros(len(W))
    np.add.at(dW, idx, g[:, None] * x)
    np.add.at(aW, idx, np.abs(g[:, None] * x))
    cc = g[:, None, None] * (x[..., None] * (vx + esum)[:, None, :] - np.asarray(V, f64)[idx] * (x * x)[..., None])
    ca = np.abs(g)[:, None, None] * (np.abs(x)[..., None] * (avx + A_esum)[:, None, :] + Va * (x * x)[..., None])
    dV, aV = np.zeros(np.shape(V)), np.zeros(np.shape(V))
    np.add.at(dV, idx, cc)
    np.add.at(aV, idx, ca)
    lossv = (np.maximum(p, 0) - p * y + np.log1p(np.exp(-np.abs(p)))).mean()
    return dict(dB=g.sum(), dW=dW, dV=dV, fg=fg, loss=lossv, aB=np.abs(g).sum(), aW=aW, aV=aV, fs=fs)


def tensor_names(n_fields):
    return ["B", "W", "V"] + ["%s[%d]" % (nm, k) for k in range(n_fields) for nm in NAMES]


def flatten(B, W, V, fields):
    """[B, W, V, H[0], Wa[0], ...]: the order of tensor_names()"""
    return [np.array([B]).reshape(-1), np.asarray(W), np.asarray(V)] + [np.asarray(a) for fld in fields for a in fld]


def _glist(G):
    return flatten(G["dB"], G["dW"], G["dV"], G["fg"]), flatten(G["aB"], G["aW"], G["aV"], G["fs"])


class StepTrainer:
    """fm_ref.StepTrainer with embedding fields: one batch per step(), fp32 parameters and moments of B, W, V and every field
    tensor, float64 gradients rounded to fp32, fm_ref.opt_step32 on each tensor on its own.  dtype float64 is the all-float64
    twin (opt_step64, the fp32 lr_t), used only to measure this reference's own divergence.  slack: fm_ref.StepTrainer.slack's
    rule per element of every tensor, with grads_ex's scales."""

    def __init__(self, B, W, V, fields, t=0, dtype=f32):
        self.dt = dtype
        self.p = [np.asarray(a, dtype).copy() for a in flatten(B, W, V, fields)]
        self.m = [np.zeros(a.size, dtype) for a in self.p]
        self.v = [np.zeros(a.size, dtype) for a in self.p]
        self.slack = [np.zeros(a.size) for a in self.p]
        self.t = t
        self.max_scale = 0.0  # the largest logit scale any step has seen

    @property
    def params(self):
        return self.p[0][0], self.p[1], self.p[2]

    @property
    def fields(self):
        return [tuple(self.p[3 + 5 * k:8 + 5 * k]) for k in range((len(self.p) - 3) // 5)]

    def lr_t(self, adam, lr, t):
        return self.dt(R.adam_lr(lr, t) if adam else f32(lr))

    def step(self, idx, val, embs, tgt, adam, lr, wd, fault=None):
        B, W, V = self.params
        G = grads_ex(B, W, V, self.fields, idx, val, embs, tgt, fault=fault)
        self.max_scale = max(self.max_scale, float(np.max(forward(B, W, V, self.fields, idx, val, embs)[2])))
        gl, al = _glist(G)
        if adam:
            self.t += 1
        lr_t = self.lr_t(adam, lr, self.t)
        step = R.opt_step32 if self.dt == f32 else R.opt_step64
        for k, gk in enumerate(gl):
            shape = self.p[k].shape
            p, self.m[k], self.v[k] = step(self.p[k], np.asarray(gk, self.dt), self.m[k], self.v[k], wd, lr_t, adam)
            self.p[k] = p.reshape(shape)
            if adam:
                self.slack[k] += f64(lr_t) * f64(f32(1) - R.BETA1) * GRAD_K * al[k].reshape(-1) / (
                    np.sqrt(self.v[k].astype(f64)) + f64(R.EPS))
        return G["loss"]

    def epoch(self, idx, val, embs, tgt, bs, adam, lr, wd, fault=None):
        """fault: a planted fault; ("full_modulus", None) takes bs for the modulus"""
        cost = f32(0)
        if fault and fault[0] == "full_modulus":
            fault = ("full_modulus", bs)
        for i in range(0, len(tgt), bs):
            sl = slice(i, min(i + bs, len(tgt)))
            cost = f32(cost + f32(self.step(idx[sl], val[sl], [e[sl] for e in embs], tgt[sl], adam, lr, wd, fault)))
        return cost


GRAD_K = 1e-5  # the carried-gradient bar's share of the gradient scale (the plain machine's; test_fm_attention_cpu.py measures it)


def one_step_report(B, W, V, fields, idx, val, embs, tgt, got, cost, adam, lr, wd):
    """fm_ref.one_step_report for a model with embedding fields.  got = flatten() of the parameters after the step.  Ratios are
    error / bar (<= 1 passes), per tensor name of tensor_names():
      cost          |cost - loss| / (1e-5 loss)
      <name>        elements with a nonzero float64 gradient: |got - ref| / (1e-5 (|ref| + lr)), ref = opt_step32 of that gradient
      <name>_ill    Adam only: (elements, elements with a gradient, worst ratio) of those that no gradient within its bar can
                    hold to the flat bar (fm_ref.one_step_report's rule, with grads_ex's scales)
      ill           Adam only: (such elements, elements with a gradient) over all tensors; a property of the reference alone
      <name>_zero   elements whose float64 gradient is exactly zero (untouched rows of W and V, a relu no row opens, an embedding
                    column that is zero in every row): fm_ref.untouched_report against the zero-gradient opt_step32
      g<name>       SGD only: (p0 - got) / lr - wd p0 against the float64 gradient over
                    GRAD_K scale + 2^-23 (|got| / lr + |g| + wd |p0|)
      still         names of the field tensors (H, Wa, ba, We, be of every field) that did not move at all.  With wd > 0 a tensor
                    whose gradient is all zero (H, Wa, ba at D = 1) moves too, by weight decay alone: what its elements then
                    have to equal is <name>_zero's business; elements with a gradient are held to ref, which differs from p0"""
    G = grads_ex(B, W, V, fields, idx, val, embs, tgt)
    gl, al = _glist(G)
    p0s = flatten(B, W, V, fields)
    names = tensor_names(len(fields))
    lr_t = R.adam_lr(lr, 1) if adam else f32(lr)
    rep = {"cost": abs(cost - G["loss"]) / (1e-5 * G["loss"]), "still": []}
    lr64, wd64 = f64(f32(lr)), f64(f32(wd))
    for name, p0, g64, a64, gp in zip(names, p0s, gl, al, got):
        p0, g64, a64, gp = np.asarray(p0, f32).reshape(-1), g64.reshape(-1), a64.reshape(-1), np.asarray(gp, f32).reshape(-1)
        zero = np.zeros(p0.size, f32)
        ref = R.opt_step32(p0, g64.astype(f32), zero, zero, wd, lr_t, adam)[0]
        un = g64 == 0
        if un.any():
            rep[name + "_zero"] = R.untouched_report(gp, R.opt_step32(p0, zero, zero, zero, wd, lr_t, adam)[0], un)
        if name not in ("B", "W", "V") and np.array_equal(gp, p0):
            rep["still"].append(name)
        t = ~un
        if not t.any():
            continue
        err = np.abs(gp.astype(f64) - ref)
        flat = 1e-5 * (np.abs(ref.astype(f64)) + lr)
        p64, q64 = p0.astype(f64), gp.astype(f64)
        if adam:
            e = f64(R.EPS) / np.sqrt(f64(f32(1) - R.BETA2))
            gbar = GRAD_K * a64 + 2.0 ** -23 * (np.abs(g64) + wd64 * np.abs(p64))
            prop = lr64 * gbar * e / (np.abs(g64 + wd64 * p64) + e) ** 2
            ill = t & (prop > flat)
            rep[name + "_ill"] = (int(ill.sum()), int(t.sum()), float(np.max(err[ill] / (flat + prop)[ill])) if ill.any() else 0.0)
            rep["ill"] = (rep.get("ill", (0, 0))[0] + int(ill.sum()), rep.get("ill", (0, 0))[1] + int(t.sum()))
            t = t & ~ill
        rep[name] = float(np.max(err[t] / flat[t])) if t.any() else 0.0
        if not adam:
            carried = (p64 - q64) / lr64 - wd64 * p64
            bar = GRAD_K * a64 + 2.0 ** -23 * (np.abs(q64) / lr64 + np.abs(g64) + wd64 * np.abs(p64))
            rep["g" + name] = float(np.max(np.abs(carried[t] - g64[t]) / bar[t]))
    return rep


def worst(rep):
    """the largest ratio of a one_step_report (cost, parameters, ill-conditioned elements, carried gradients); infinite where
    an element with a zero gradient breaks its exact rule (a bit in the fused body or in the tail; W and V, whose step is
    fm_opt_kernel's, may differ by one ulp in the tail as in test_gpu_fm_train_shapes.py)"""
    out = 0.0
    for k, v in rep.items():
        if k.endswith("_zero") and (v[0] > 0 or v[1] > (1 if k in ("W_zero", "V_zero") else 0)):
            return np.inf
        if k in ("still", "ill") or k.endswith("_zero"):
            continue
        out = max(out, v[2] if k.endswith("_ill") else v)
    return out


def ref_step(B, W, V, fields, idx, val, embs, tgt, adam, lr, wd, dtype=f64, fault=None):
    """(flatten() of the parameters after one step, the loss) with the gradients evaluated in dtype / with a planted fault:
    what one_step_report is given in a device's place by the CPU tests"""
    G = grads_ex(B, W, V, fields, idx, val, embs, tgt, dtype, fault)
    lr_t = R.adam_lr(lr, 1) if adam else f32(lr)
    out = []
    for p0, g in zip(flatten(B, W, V, fields), _glist(G)[0]):
        z = np.zeros(p0.size, f32)
        out.append(R.opt_step32(p0, np.asarray(g, f32), z, z, wd, lr_t, adam)[0].reshape(p0.shape))
    return out, G["loss"]


def params_report(got, ref, lr, k, slack=None):
    """fm_ref.params_report over flatten()'s tensors -> {name: worst |got - ref| / (k (|ref| + lr) + capped slack)}"""
    names = tensor_names((len(ref) - 3) // 5)
    out = {}
    for i, (name, g, r) in enumerate(zip(names, got, ref)):
        out[name] = R.params_report([g], [r], lr, k, None if slack is None else [slack[i]])
    return out


def divergence(a, b, lr):
    """largest |a - b| / (|b| + lr) over two lists of tensors"""
    return max(float(np.max(np.abs(np.asarray(x, f64) - np.asarray(y, f64)) / (np.abs(np.asarray(y, f64)) + lr))) for x, y in zip(a, b))


# ---- the inputs of test_gpu_fm_attention_shapes.py (test_fm_attention_cpu.py checks the bars on the same) ---------------------
NF = 203  # W's tail holds 11 elements; features 150.. are never used


def model(d, dims, seed):
    """B, W, V and fields with H ~ Normal(0, 0.3) and nonzero biases (AFM.Init's sd of 0.01 would make the softmax all but
    uniform and hide an indexing fault).  At D = 4096 H's sd is 4.5 / sqrt(d) (1.0 at d = 20, 0.4 at d = 128): with a flatter
    softmax dWa lies so far below its scale there that Adam's first step is ill-conditioned on over 5 % of the elements."""
    rng = np.random.default_rng(seed)
    h_sd = max(0.3, 4.5 / np.sqrt(d)) if max(dims) >= 4096 else 0.3
    B, W, V = f32(rng.normal(0, 0.5)), rng.normal(0, 0.2, NF).astype(f32), rng.normal(0, 0.2, (NF, d)).astype(f32)
    fields = []
    for D in dims:
        H, Wa, _, We, _ = init_field(rng, D, d, h_sd)
        fields.append((H, Wa, rng.normal(0, 0.1, d).astype(f32), We, rng.normal(0, 0.1, d).astype(f32)))
    return B, W, V, fields


def rows(n, dims, seed):
    """n training rows of one to six features below 150, +-1 targets, bf16 embeddings ~ Normal(0, 1); rows 4, 11, 18, ... carry
    all-zero embeddings (a sample without one, fm.go:555-561)"""
    rng = np.random.default_rng(seed)
    rr = []
    for _ in range(n):
        k = int(rng.integers(1, 7))
        rr.append((rng.choice(150, k, replace=False).astype(np.int32), rng.normal(1, 0.5, k).astype(f32)))
    idx, val = R.pad(rr, 6)
    tgt = np.where(rng.random(n) < 0.5, 1, -1).astype(f32)
    embs = []
    for D in dims:
        e = rng.normal(0, 1, (n, D)).astype(f32)
        e[4::7] = 0
        embs.append(to_bf16(e))
    return idx, val, tgt, embs


def case(d, dims, n):
    """(B, W, V, fields, idx, val, tgt, embs) of one one-step case"""
    seed = 1000 * d + 10 * n + sum(dims) % 997
    return model(d, dims, seed) + rows(n, dims, seed + 1)


BASE = (20, (65,), 13)
EIGHT = (61, 50, 33, 17, 16, 9, 3, 1)  # eight fields, each of another small D, the largest first
ONE_STEP = ([(d, BASE[1], BASE[2]) for d in (1, 3, 4, 15, 16, 17, 20, 64, 65, 100, 128)]
            + [(BASE[0], (D,), BASE[2]) for D in (1, 63, 64, 127, 128, 129, 4096)]
            + [(BASE[0], BASE[1], n) for n in (1, 3, 7, 8, 9, 64, 67)]
            + [(128, (4096,), 9), (20, (129, 5, 64), 13), (20, EIGHT, 13)])
MULTI = [(20, (65, 9)), (100, (128,))]  # 45 rows in batches of 13, 13, 13, 6, three epochs
MULTI_N, MULTI_BS = 45, 13
LIFE = (20, (65, 9))                    # 45 rows at batch sizes 13, 9, 32; a second set of 40 rows; a new Fit


def rates(adam, d=0):
    """(lr, wd): the one-step rates of test_gpu_fm_attention.py; over several steps at d >= 64 a tenth of them, since the
    wrapped softmax (it subtracts another row's maximum) lets the d = 100 model's logits run away at the full rate"""
    lr = 0.01 if adam else 0.05
    return (lr / 10 if d >= 64 else lr), 0.01


def life_stages(A, A2):
    """(stage, data, batch size, new set?, new Fit?) of the handle life cycle"""
    return [("bs 13", A, 13, False, False), ("bs 9", A, 9, False, False), ("bs 32", A, 32, False, False),
            ("second set", A2, 32, True, False), ("new Fit", A2, 32, False, True)]


# measured by test_fm_attention_cpu.py (which measures them again and fails if they are exceeded)
# largest divergence of the fp32-step StepTrainer from its all-float64 twin, |a - b| / (|b| + lr), over the multi-step and
# life-cycle schedules: 5.59e-7 (SGD, d = 100, epoch 3, last batch) and 6.79e-6 (Adam, d = 100, epoch 3), rounded up
DIVERGENCE = {False: 5.6e-7, True: 6.8e-6}
K_MULTI = {adam: R.K_MULTI[adam] / R.DIVERGENCE[adam] * v for adam, v in DIVERGENCE.items()}  # 4 x, fm_ref.K_MULTI's factor
# the fp32 restatement of the gradients over the one-step bars, worst case over the 28 cases as (kind, adam): measured 0.00505
# (cost, either optimizer), 0.0764 (SGD parameters), 0.499 (carried gradient: the bar's rounding term, as in the plain machine),
# 0.360 (Adam parameters), 0.385 (Adam's ill-conditioned elements over their widened bar), rounded up.  All at most half a
# bar, so GRAD_K stays the plain machine's 1e-5.
HEADROOM = {("cost", False): 0.0051, ("cost", True): 0.0051, ("param", False): 0.077, ("carried", False): 0.5,
            ("param", True): 0.37, ("ill", True): 0.39}
# cap on the share of a case's elements that Adam's first step leaves ill-conditioned: twice the largest share the reference
# produces, 3.09 % at (d, dims, n) = (128, (4096,), 9)
ILL_SHARE = 0.062
# every logit's scale over a multi-step or life-cycle schedule stays within this factor of its value at the first step
# (measured: 1.73 at most, the d = 20 SGD schedule; 1.54 at d = 100, 1.40 over the life cycle)
SCALE_GROWTH = 2.0
