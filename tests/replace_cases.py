"""The passes tests/test_gpu_cand_replace.py runs, as plain data built without a device, so that tests/test_cand_replace_cpu.py can
show with the restatement alone that every case reaches what it is named for.

The ranker is a factorization machine whose score of item i is W[i] whoever asks (no factors, one feature per item), so a case
chooses every score.  Query 0 of every ranked case is the ANCHOR: under each pair of decays used here it has an appended item, a
history item that was a candidate already, and a tie that only the decay makes."""
import numpy as np

import replace_ref as RR

P, RD = RR.POSITIVE, RR.READ
SORT_LDS = 4096   # the longest history row sorted in LDS, and the longest list sorted on the device
DECAYS = {"reference": (0.8, 0.7), "one": (1.0, 1.0), "above_one": (1.5, 2.0), "tiny": (1e-300, 1e-300)}

# items 0 .. 7 belong to the anchor.  10 * 0.8 == 8; 10 * 1 == 10; 10 * 1.5 == 15; -2e-38 * 1e-300 == -0 against the +0 of item 5
ANCHOR_W = [10.0, 8.0, 10.0, 15.0, -2e-38, 0.0, 9.0, 12.0]
ANCHOR_LIST = [(i, float(i)) for i in (0, 1, 2, 3, 4, 5, 7)]
ANCHOR_HISTORY = [(0, P), (4, P), (6, RD), (7, RD), (0, RD)]
# what the other items score: values that tie under the decays above (5 * 0.8 == 4, 10 * 1.5 == 15, 5 * 1.5 == 7.5, 2.5 * 2 == 5), both
# infinities, a NaN, and 1e-10, whose product with 1e-300 is a subnormal double
POOL = np.array([10.0, 8.0, 5.0, 4.0, 15.0, 7.5, 2.5, 2.0, 0.0, -1.0, -0.8, 1e-10, -2e-38, 3e38, np.inf, -np.inf, np.nan, 6.25, 5.0, 7.0],
                np.float32)


class Case:
    def __init__(self, name, n_items, seed=0, ranked=True):
        self.name, self.n_items, self.ranked = name, n_items, ranked
        self.rng = np.random.default_rng(seed)
        self.base, self.lists, self.history = [], [], []
        self.keep = self.finish_keep = None
        self.k = 8
        self.sort_cap = 0
        self.W = None
        if ranked:
            self.W = self.rng.choice(POOL, n_items).astype(np.float32)
            self.W[:8] = ANCHOR_W
            self.query([], ANCHOR_LIST, ANCHOR_HISTORY)

    def query(self, base, lst, history):
        """lst = [(item, recommender's score)], history = [(item, kind)]"""
        self.base.append([int(i) for i in base])
        self.lists.append([(int(i), float(s)) for i, s in lst])
        self.history.append([(int(i), int(k)) for i, k in history])
        self.k = max(self.k, len(lst))

    def scored(self, items):
        return [(int(i), float(s)) for i, s in zip(items, self.rng.normal(0, 1, len(items)))]

    def kinds(self, items):
        return [(int(i), int(k)) for i, k in zip(items, self.rng.choice([P, P, RD], len(items)))]

    @property
    def nq(self):
        return len(self.lists)


def raw_row(c, n, lo):
    """a history row of exactly n entries of items >= lo: n - n // 8 distinct ones, the rest repeats, under the other kind and under
    the same one, shuffled"""
    if n == 0:
        return []
    distinct = lo + c.rng.choice(c.n_items - lo, n - n // 8, replace=False)
    row = c.kinds(distinct)
    row += [(i, P + RD - k) for i, k in row[: n // 16]] + row[n // 16: n // 8]
    return [row[j] for j in c.rng.permutation(len(row))]


def history_rows():
    """raw history rows at the edges of the wave's chunk of 64 and of the LDS sort; a row of one item under both kinds; a row keep
    drops whole"""
    c = Case("history_rows", 6000, seed=1)
    c.lengths = [0, 1, 63, 64, 65, SORT_LDS - 1, SORT_LDS, SORT_LDS + 1]
    for n in c.lengths:
        row = raw_row(c, n, 8)
        inside = [i for i, _ in row[:5]]  # candidates that are in the history, and some that are not
        c.query([], c.scored(list(dict.fromkeys(inside + (8 + c.rng.choice(5000, 6, replace=False)).tolist()))), row)
    c.one_item = c.nq
    c.query([], c.scored([20, 21]), [(33, RD), (33, P)] * 50)
    c.dropped = c.nq
    gone = (8 + c.rng.choice(5000, 70, replace=False)).tolist()
    c.query([], c.scored([30, 31, gone[0]]), c.kinds(gone + gone[:9]))
    c.keep = np.ones(c.n_items, np.uint8)
    c.keep[gone] = 0
    c.keep[8 + c.rng.choice(5000, 500, replace=False)] = 0
    c.keep[:8] = 1
    c.keep[33] = 1
    return c


def top_items():
    """items next to 2^31 - 1: the history word item * 2 + read uses all 32 bits.  No catalogue is that large: rows only."""
    n = 2**31 - 1
    c = Case("top_items", n, ranked=False)
    top = n - 1
    c.query([top], [(top - 1, 1.0), (5, 2.0), (top - 2, 3.0)], [(top, RD), (top, P), (top - 1, RD), (0, P), (top - 3, P), (top - 3, RD)])
    c.query([], [(top, 1.0)], [(top, RD)])
    c.query([], [], [(top - 1, P), (top, RD), (1, RD)])
    return c


def candidates():
    """what the candidates can be against the history"""
    c = Case("candidates", 300, seed=2)
    hist = c.kinds(8 + c.rng.choice(200, 40, replace=False))
    items = [i for i, _ in hist]
    c.empty = c.nq
    c.query([], [], hist)                                                  # no candidates at all: everything is appended
    c.whole = c.nq
    c.query([], c.scored(items + [250, 251]), hist)                        # the whole history among the candidates: nothing is appended
    c.repeat = c.nq
    c.query([], c.scored([items[0], 260, items[0], items[1]]), hist[:5])   # a candidate twice, and in the history
    c.excluded = c.nq
    c.query(items, c.scored(items[:10] + [270, 271]), hist)                # the base row holds the history: no recommender offers it
    c.query([250, 251], c.scored(items[:10] + [270, 271]), hist)           # ... and a base row that does not
    c.finish_keep = np.ones(300, np.uint8)
    c.finish_keep[[251, 271]] = 0
    return c


def queries(nq):
    """nq queries with tiny rows: 2047 / 2048 around one scan tile, 4097 past two tiles and past the launches' grid caps (4096 queries
    in flight), where the kernels' loops stride"""
    c = Case("queries_%d" % nq, 97, seed=nq)
    for _ in range(nq - 1):
        lst = c.scored(c.rng.integers(8, 97, int(c.rng.integers(0, 6))))
        c.query(c.rng.integers(0, 97, int(c.rng.integers(0, 3))), lst, c.kinds(c.rng.integers(8, 97, int(c.rng.integers(0, 6)))))
    c.keep = (np.arange(97) % 7 != 3).astype(np.uint8)
    c.keep[:8] = 1
    return c


def sort_lengths(lengths=(1, 2, 63, 64, 65, SORT_LDS, SORT_LDS + 1), sort_cap=0, name="sort_lengths"):
    """lists of exactly these lengths after the append, of candidates outside the history, candidates inside it and appended items"""
    c = Case(name, 6000, seed=3)
    c.lengths = list(lengths)
    c.sort_cap = sort_cap
    for n in lengths:
        items = 8 + c.rng.choice(5900, n, replace=False)
        a = min(n // 3, 100)
        c.query([], c.scored(items[: 2 * a]), c.kinds(items[a:]))
    return c


def specials():
    """a NaN score, the infinities, zero and a score whose product is a subnormal double, each once decayed and once not"""
    c = Case("specials", 40, seed=4)
    w = [np.nan, np.nan, np.inf, np.inf, -np.inf, -np.inf, 0.0, 0.0, 1e-10, 1e-10, -2e-38, -2e-38, 10.0, 8.0, 3e38, 3e38]
    c.W[8:8 + len(w)] = w
    items = list(range(8, 8 + len(w)))
    c.special = c.nq
    c.query([], c.scored(items), [(i, P if i % 4 == 0 else RD) for i in items[::2]] + [(30, P), (31, RD)])
    c.query([], [], [(i, P) for i in items])
    return c


RANKED = {
    "history_rows": history_rows,
    "candidates": candidates,
    "queries_1": lambda: queries(1),
    "queries_2047": lambda: queries(2047),
    "queries_2048": lambda: queries(2048),
    "queries_4097": lambda: queries(4097),
    "sort_lengths": sort_lengths,
    "sort_cap_hook": lambda: sort_lengths((15, 16, 17, 40), sort_cap=16, name="sort_cap_hook"),
    "specials": specials,
}
# the decays every ranked case runs under; the order-sensitive ones under all four
CASE_DECAYS = [(name, "reference") for name in RANKED] + [(name, d) for name in ("sort_lengths", "specials", "candidates")
                                                          for d in ("one", "above_one", "tiny")]


def restate(c):
    """the case on the restatement: (cand_ref.Chain, replace_ref.Replaced)"""
    import cand_ref as R
    chain = R.Chain(c.nq, c.base)
    chain.add(c.lists, c.k)
    return chain, RR.Replaced(chain, c.history, c.finish_keep, c.keep)


def ranker_scores(c, rep):
    """what the ranker gives every candidate of the grown rows: W[item]"""
    return c.W[rep.finished()[1]]
