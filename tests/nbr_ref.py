"""recommendItemToItem / recommendUserToUser (logics/recommend.go:244-348) restated in plain Python as gorse_nbr_recommend defines
them (include/gorse_hip.h): a dict of Python floats added in stored order, the weight transform of item_to_item.go:64-87 /
user_to_user.go:63-80, and the call's total order -- larger sum first, equal sums by ascending item, a NaN sum after every number."""
import math

import numpy as np

RAW, RECIP = 0, 1
HOP1, HOP2 = 0, 1


class Table:
    """a neighbour table: rows = lists of indices, weights = lists of raw float32 similarities per row, or None"""

    def __init__(self, rows, weights=None, transform=RAW, scale=1.0):
        self.rows = [np.asarray(r, np.int32) for r in rows]
        self.weights = None if weights is None else [np.asarray(w, np.float32) for w in weights]
        self.transform, self.scale = transform, float(scale)
        assert self.weights is None or [len(w) for w in self.weights] == [len(r) for r in self.rows]

    def csr(self):
        ptr = np.zeros(len(self.rows) + 1, np.int64)
        ptr[1:] = np.cumsum([len(r) for r in self.rows])
        cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs and ptr[-1] else np.zeros(0, dt)  # noqa: E731
        return ptr, cat(self.rows, np.int32), None if self.weights is None else cat(self.weights, np.float32)

    def set_on(self, handle, which):
        ptr, idx, w = self.csr()
        handle.set_table(which, ptr, idx, w, self.transform, self.scale)

    def entries(self, r):
        """(index, weight as a Python float) of row r in stored order"""
        if self.weights is None:
            return [(int(j), 1.0) for j in self.rows[r]]
        return [(int(j), weight(x, self.transform, self.scale)) for j, x in zip(self.rows[r], self.weights[r])]


def weight(raw, transform, scale):
    w = float(np.float32(raw)) * scale
    if transform == RECIP:
        d = 1.0 - w
        w = math.copysign(math.inf, d) if d == 0.0 else 1.0 / d  # IEEE division where Python raises
    return w


def sums(hop1, hop2, row, reverse=False):
    """item -> sum for a walk from hop-1 row `row`, in insertion order (reverse: the same lists, last list first)"""
    s = {}
    lists = hop1.entries(row)
    for src, w1 in (reversed(lists) if reverse else lists):
        for j, w2 in hop2.entries(src):
            s[j] = s.get(j, 0.0) + w1 * w2
    return s


def order_key(item, s):
    """sorted by (isnan, -sum, item); a NaN's -sum compares with nothing, so NaN sums rank among themselves by item alone"""
    nan = math.isnan(s)
    return (nan, 0.0 if nan else -s, item)


def recommend_one(hop1, hop2, row, k, seen=()):
    if row < 0:
        return []
    seen = set(int(x) for x in seen)
    cand = [(j, s) for j, s in sums(hop1, hop2, row).items() if j not in seen]
    return sorted(cand, key=lambda e: order_key(*e))[:k]


def recommend(hop1, hop2, rows, k, seen_rows=None):
    """what gorse_nbr_recommend returns: (items n x k padded with -1, sums n x k padded with 0, counts)"""
    n = len(rows)
    items, sc, cnt = np.full((n, k), -1, np.int32), np.zeros((n, k), np.float64), np.zeros(n, np.int32)
    for t, r in enumerate(rows):
        got = recommend_one(hop1, hop2, int(r), k, () if seen_rows is None else seen_rows[t])
        cnt[t] = len(got)
        for i, (j, s) in enumerate(got):
            items[t, i], sc[t, i] = j, s
    return items, sc, cnt


def seen_csr(seen_rows):
    ptr = np.zeros(len(seen_rows) + 1, np.int64)
    ptr[1:] = np.cumsum([len(r) for r in seen_rows])
    flat = np.concatenate([np.asarray(r, np.int32) for r in seen_rows]).astype(np.int32) if ptr[-1] else np.zeros(0, np.int32)
    return ptr, flat


def assert_same(got, want, what=""):
    """items, counts, padding and the bits of every sum"""
    gi, gs, gc = got
    wi, ws, wc = want
    assert np.array_equal(gc, wc), (what, "counts", gc.tolist(), wc.tolist())
    bad = np.nonzero((gi != wi).any(axis=1))[0]
    assert bad.size == 0, (what, "items of query", int(bad[0]), gi[bad[0]].tolist(), wi[bad[0]].tolist())
    gb, wb = np.ascontiguousarray(gs).view(np.uint64), np.ascontiguousarray(ws).view(np.uint64)
    bad = np.nonzero((gb != wb).any(axis=1))[0]
    assert bad.size == 0, (what, "sums of query", int(bad[0]), gs[bad[0]].tolist(), ws[bad[0]].tolist())


def order_sensitive_inputs(seed=7, n_queries=32, n_lists=24, list_len=65, n_items=257):
    """RECIP over raw weights -20 U(0,1): sums whose bits depend on the order of the lists.  Query t walks hop-1 row t, whose entries
    are hop-2 rows t * n_lists .. (t + 1) * n_lists - 1, each `list_len` distinct items of n_items."""
    rng = np.random.default_rng(seed)
    rows2, w2 = [], []
    for _ in range(n_queries * n_lists):
        rows2.append(rng.choice(n_items, list_len, replace=False).astype(np.int32))
        w2.append((-20.0 * rng.random(list_len)).astype(np.float32))
    hop1 = Table([np.arange(t * n_lists, (t + 1) * n_lists) for t in range(n_queries)])
    return hop1, Table(rows2, w2, RECIP, 1.0), n_items
