"""numpy restatement of what gorse_fm_evaluate returns (model/ctr/evaluator.go:85-153 on the two sides' logits), shared by
test_fm_evaluate_cpu.py (which pins it to ctr.AUC and the other host metrics without a device) and test_gpu_fm_evaluate.py."""
import numpy as np

f32, u32 = np.float32, np.uint32
SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257, 3 * 256 + 7)
CAP = 1 << 24  # a float32 counter incremented by one stops here: 2^24 + 1 rounds back to 2^24


def below(pos, neg):
    """per non-NaN positive in ascending order: the non-NaN negatives strictly below it (as floats: -0 == +0)"""
    pos, neg = np.asarray(pos, f32), np.asarray(neg, f32)
    p, n = np.sort(pos[~np.isnan(pos)]), np.sort(neg[~np.isnan(neg)])
    return np.searchsorted(n, p, side="left").astype(np.int64)


def chain(cnt):
    """sum += float32(count), one after the other (cumsum adds strictly left to right in the array's own precision)"""
    return np.cumsum(np.asarray(cnt).astype(f32), dtype=f32)[-1] if len(cnt) else f32(0)


def counts(pos, neg):
    """gorse_fm_evaluate's seven counts, in its order, and auc_sum"""
    pos, neg = np.asarray(pos, f32), np.asarray(neg, f32)
    cnt = below(pos, neg)
    c = [len(pos), len(neg), int((pos > 0).sum()), int((neg > 0).sum()), int((neg < 0).sum()),
         int(np.isnan(pos).sum() + np.isnan(neg).sum()), int(cnt.sum())]
    return c, chain(cnt)


def score(c, auc_sum):
    """(Precision, Recall, Accuracy, AUC) formed from the counts as evaluator.go forms them from the logits, float32 throughout"""
    n_pos, n_neg = c[0], c[1]
    tp, fp, fn = f32(min(c[2], CAP)), f32(min(c[3], CAP)), f32(min(n_pos - c[2], CAP))
    correct = f32(min(c[2] + c[4], CAP))
    precision = f32(0) if tp + fp == 0 else f32(tp / f32(tp + fp))
    recall = f32(0) if tp + fn == 0 else f32(tp / f32(tp + fn))
    accuracy = f32(0) if n_pos + n_neg == 0 else f32(correct / f32(n_pos + n_neg))
    auc = f32(0) if n_pos * n_neg == 0 else f32(f32(auc_sum) / f32(n_pos * n_neg))
    return precision, recall, accuracy, auc


def host_score(pos, neg):
    """the same four through the host library's metrics (ctr.Precision / Recall / Accuracy / AUC: the yardstick)"""
    from gorse_amd import ctr
    return tuple(f32(m(pos, neg)) for m in (ctr.Precision, ctr.Recall, ctr.Accuracy, ctr.AUC))


def same_bits(a, b):
    return np.array_equal(np.asarray(a, f32).view(u32), np.asarray(b, f32).view(u32))


# ---- the logits of the metric tests ---------------------------------------------------------------------------------------
def _pick(values):
    pool = np.array(values, f32)
    return lambda rng, n: pool[rng.integers(0, pool.size, n)]


CONTENTS = {
    "normal": lambda rng, n: rng.normal(0, 1, n).astype(f32),
    "quarters": lambda rng, n: (np.round(rng.normal(0, 1, n) * 4) / 4).astype(f32),  # many ties between the sides
    "equal": lambda rng, n: np.full(n, 0.5, f32),
    "signed_zeros": _pick([0.0, -0.0, 0.0, -0.0, 1.0, -1.0]),
    "infinities": _pick([np.inf, -np.inf, 0.5, -0.5, 0.0]),
    "subnormals": _pick([1e-45, -1e-45, 1e-40, -1e-40, 0.0, -0.0, 1.1754944e-38, -1.1754944e-38]),
    "negative": lambda rng, n: (-np.abs(rng.normal(0, 1, n)) - 0.1).astype(f32),
    "zero": lambda rng, n: np.zeros(n, f32),  # counts for neither Precision's > 0 nor Accuracy's < 0
}


def sides(kind, n_pos, n_neg):
    rng = np.random.default_rng(1000 * n_pos + n_neg + 7 * len(kind))
    return CONTENTS[kind](rng, n_pos), CONTENTS[kind](rng, n_neg)


def wide():
    """8192 x 8192 normal logits, the positives shifted by 0.5: the exact total passes 2^25, so the chain rounds"""
    rng = np.random.default_rng(0)
    return (rng.normal(0.5, 1, 8192)).astype(f32), rng.normal(0, 1, 8192).astype(f32)


def with_nans():
    rng = np.random.default_rng(3)
    pos, neg = rng.normal(0.3, 1, 300).astype(f32), rng.normal(0, 1, 270).astype(f32)
    pos[[0, 17, 299]] = np.nan
    neg[[5, 64]] = np.array([0xffc00001, 0x7fc00000], u32).view(f32)  # either sign
    return pos, neg
