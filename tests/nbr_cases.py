"""Inputs of the neighbourhood recommender's selection and walk tests (tests/test_gpu_nbr_select.py, tests/test_gpu_nbr_walk.py), kept
apart from the GPU modules so that tests/test_nbr_cases_cpu.py can show, with tests/nbr_ref.py alone, that every builder gives the
property its GPU test relies on.

A case is a pair of tables, the queries and the k's of its calls.  Every case runs in three forms of csrc/nbr_recommend.hip's kernel:
    wave    as built: a bound of at most 511 puts the query on a 512-slot LDS table walked by one wave (64 threads)
    lds256  each seen row padded with 600 items no table names: the bound lies in 512 .. 4095, a 4096-slot LDS table and 256 threads
    global  the test hook leaves 2 LDS slots, each seen row is padded with 2 such items: every query walks a table in global scratch
The padding names items that are never reached, so one expectation serves the three forms.  stop_depth() is a plain model of the
kernel's radix select that tells which byte of the 96-bit key a query's selection stops at; it never produces an expected result."""
import functools
import struct

import numpy as np

import nbr_ref as R

WAVE_SLOTS, MID_SLOTS, MAX_SLOTS = 512, 4096, 13056  # kWaveSlots, kMidSlots, kMaxLdsSlots of csrc/nbr_plan.hpp
FORMS = ("wave", "lds256", "global")
PAD = {"wave": 0, "lds256": 600, "global": 2}
HOOK = {"wave": 0, "lds256": 0, "global": 1}  # capi.set_nbr's lds_slots
MAX_ITEMS = 2 ** 31 - 1
M64 = (1 << 64) - 1


# ---- the select's order as integers

def sum_key(s):
    """larger sum = larger key; -0 as +0; every NaN below every number"""
    if s != s:
        return 0
    bits = 0 if s == 0.0 else struct.unpack("<Q", struct.pack("<d", s))[0]
    return (~bits & M64) if bits >> 63 else bits | 1 << 63


def key96(item, s):
    return sum_key(s) << 32 | (~item & 0xffffffff)


def stop_depth(cands, k):
    """the byte (11 = the sums' top byte .. 4 = their low byte, 3 .. 0 = the item's bytes) at which a most-significant-byte-first
    select over the (item, sum) candidates has separated exactly k keys; None when there are at most k candidates"""
    keys = [key96(j, s) for j, s in cands]
    assert len(set(keys)) == len(keys)
    if len(keys) <= k:
        return None
    need = k
    for d in range(11, -1, -1):
        byte = [(x >> 8 * d) & 255 for x in keys]
        above, b = 0, 255
        while above + byte.count(b) < need:
            above += byte.count(b)
            b -= 1
        need -= above
        keys = [x for x, y in zip(keys, byte) if y == b]
        if len(keys) == need:
            return d
    raise AssertionError("distinct keys are separated at byte 0 at the latest")


# ---- cases and their three forms

class Case:
    def __init__(self, name, hop1, hop2, n_items, rows, ks, seen=None, **notes):
        self.name, self.hop1, self.hop2, self.n_items, self.rows, self.ks = name, hop1, hop2, int(n_items), list(rows), tuple(ks)
        self.seen = None if seen is None else [[int(x) for x in s] for s in seen]
        self.notes = notes
        assert self.seen is None or len(self.seen) == len(self.rows)

    def seen_of(self, t):
        return [] if self.seen is None else self.seen[t]

    def candidates(self, t):
        """(item, sum) of query t in no particular order"""
        if self.rows[t] < 0:
            return []
        seen = set(self.seen_of(t))
        return [(j, s) for j, s in R.sums(self.hop1, self.hop2, self.rows[t]).items() if j not in seen]

    def depths(self):
        """{(query, k): stop depth} of every call in which the select runs"""
        out = {}
        for t in range(len(self.rows)):
            cand = self.candidates(t)
            for k in self.ks:
                d = stop_depth(cand, k)
                if d is not None:
                    out[t, k] = d
        return out


def pad_items(case, n):
    """n items that no hop-2 row and no seen row of the case names, residues spread (step 3)"""
    used = set(int(j) for r in case.hop2.rows for j in r) | set(x for s in (case.seen or []) for x in s)
    out, x = [], 1000
    while len(out) < n:
        if x not in used:
            out.append(x)
        x += 3
    return out


def in_form(case, form):
    """(n_items, seen rows or None, the hook's lds_slots) of the case in one of FORMS"""
    pad = pad_items(case, PAD[form])
    if not pad:
        return case.n_items, case.seen, HOOK[form]
    seen = [case.seen_of(t) + pad if case.rows[t] >= 0 else case.seen_of(t) for t in range(len(case.rows))]
    return max(case.n_items, pad[-1] + 1), seen, HOOK[form]


def bounds(case, n_items, seen):
    """the header's bound per query: min(n_items, entries the walk meets) + the seen row's length; 0 for a negative row"""
    out = []
    for t, r in enumerate(case.rows):
        met = sum(len(case.hop2.rows[s]) for s in case.hop1.rows[r]) if r >= 0 else 0
        out.append(min(n_items, met) + (len(seen[t]) if seen is not None else 0) if r >= 0 else 0)
    return out


def table_class(bound, lds_slots=0):
    """make_plan's class of a query: a table needs bound + 1 slots"""
    cap = max(2, min(lds_slots, MAX_SLOTS)) if lds_slots > 0 else MAX_SLOTS
    for name, slots in (("wave", WAVE_SLOTS), ("mid", MID_SLOTS), ("max", MAX_SLOTS)):
        if bound + 1 <= min(slots, cap):
            return name if min(slots, cap) > WAVE_SLOTS else "wave"  # a table of up to 512 slots is walked by one wave
    return "global"


def classes(case, form):
    n_items, seen, hook = in_form(case, form)
    return [table_class(b, hook) for b in bounds(case, n_items, seen)]


@functools.lru_cache(maxsize=None)
def reference(name, k):
    """the expectation of one call, computed once and shared by the forms; callers leave it unchanged"""
    c = case(name)
    return R.recommend(c.hop1, c.hop2, c.rows, k, c.seen)


def f32(xs):
    return np.asarray(xs, np.float32)


# ---- 2a: every stop depth

DEPTH_ITEMS, DEPTH_K = 40, 7


def sum_byte_case(b):
    """sums 1 + (i + 1) * 2^(8b - 52): they differ in byte b of the double alone, the select stops at depth 4 + b"""
    items = np.arange(DEPTH_ITEMS)
    low = f32([(i + 1) * 2.0 ** (8 * b - 52) for i in items])
    assert all(float(x) == (i + 1) * 2.0 ** (8 * b - 52) for i, x in zip(items, low))
    hop2 = R.Table([items, items[::-1]], [np.ones(DEPTH_ITEMS, np.float32), low[::-1]])
    return Case("sum_byte_%d" % b, R.Table([[0, 1]]), hop2, 64, [0], [DEPTH_K], depth=4 + b)


def exponent_case():
    """sums 2^i: the 6th and the 7th share the top byte of the key and differ in the exponent's low bits"""
    items = np.arange(DEPTH_ITEMS)
    hop2 = R.Table([items], [f32([2.0 ** i for i in items])])
    return Case("sum_exponent", R.Table([[0]]), hop2, 64, [0], [6], depth=10)


def sign_case():
    """7 positive sums and 33 negative ones: the cut lies at the sign"""
    items = np.arange(DEPTH_ITEMS)
    hop2 = R.Table([items], [f32([(i + 1) if i % 6 == 0 else -(i + 1) for i in items])])
    return Case("sum_sign", R.Table([[0]]), hop2, 64, [0], [DEPTH_K], depth=11)


def item_byte_case(b):
    """equal sums, items (i + 1) << 8b: the select walks all eight sum bytes and stops at byte b of the item"""
    items = (np.arange(DEPTH_ITEMS, dtype=np.int64) + 1) << (8 * b)
    n_items = MAX_ITEMS if b == 3 else int(items.max()) + 1
    hop2 = R.Table([items[::-1]], [np.full(DEPTH_ITEMS, 0.75, np.float32)])
    return Case("item_byte_%d" % b, R.Table([[0]]), hop2, n_items, [0], [DEPTH_K], depth=b)


DEPTH_CASES = tuple("sum_byte_%d" % b for b in range(6)) + ("sum_exponent", "sum_sign") + tuple("item_byte_%d" % b for b in range(4))


# ---- 2b: plateaus

def plateau_case():
    """300 equal sums, more than the survivor buffer's 256; items 7 + 13 i in shuffled order span two item bytes"""
    rng = np.random.default_rng(31)
    items = rng.permutation(7 + 13 * np.arange(300))
    return Case("plateau_300", R.Table([[0]]), R.Table([items]), 4000, [0], [256, 1, 255])


def straddle_case():
    """10 sums of 2.0, a tie group of 30 at 1.0 on items 200 + 37 i (0x0c8 .. 0x4f9), 20 sums of 0.5; k = 25 and 26 cut the group
    inside one value of item byte 1 and between two"""
    rng = np.random.default_rng(32)
    tie = 200 + 37 * np.arange(30)
    items = np.concatenate([np.arange(10) * 3, tie, 2000 + np.arange(20) * 5])
    w = f32([2.0] * 10 + [1.0] * 30 + [0.5] * 20)
    p = rng.permutation(items.size)
    return Case("tie_straddle", R.Table([[0]]), R.Table([items[p]], [w[p]]), 2200, [0], [25, 26, 10, 40])


def unweighted_case():
    """neither table weighted, sources repeat in hop-1 rows and items in hop-2 rows: every sum is a small integer"""
    rng = np.random.default_rng(33)
    rows2 = [rng.integers(0, 90, int(n)) for n in rng.integers(10, 41, 30)]
    rows1 = [rng.integers(0, 30, int(n)) for n in (5, 8, 12, 20, 20, 3, 1, 16)]
    seen = [[], [4, 5, 6], [], list(range(0, 90, 7)), [], [], [], [1]]
    return Case("unweighted", R.Table(rows1), R.Table(rows2), 90, range(8), [10, 1, 64], seen)


# ---- 2c: non-finite sums from finite raw weights

NONFINITE_CLASSES = ("+inf", "positive", "zero", "negative", "-inf", "nan")


def sum_class(s):
    if s != s:
        return "nan"
    if s in (np.inf, -np.inf):
        return "+inf" if s > 0 else "-inf"
    return "zero" if s == 0.0 else "positive" if s > 0 else "negative"


def nonfinite_case():
    """hop 2 is RECIP: raw 1.0 is 1 / (1 - 1) = +inf.  Hop 1 is RAW: -1 makes it -inf, 0 makes it NaN, +1 then -1 on one list adds
    +inf and -inf to NaN; 0 times a finite weight is a zero sum (0.0 + -0.0 is +0.0).  Query 0 has all of them, query 1 hides a few
    of each class behind its seen row, query 2 has NaN sums only."""
    one = lambda n: np.ones(n, np.float32)  # noqa: E731
    rows2 = [[3, 40, 41, 9, 77], [5, 50, 2, 63], [1, 90, 33], [0, 95, 45],
             [10, 60, 21, 8, 70, 30, 11, 61, 22, 12, 71], [4, 80, 13, 55], [14, 81]]
    w2 = [one(5), one(4), one(3), one(3),
          f32([0.5, -1.0, 0.75, -3.0, 0.25, 0.5, 2.0, 3.0, 1.5, 5.0, 2.0]), f32([0.5, 2.0, -1.0, 3.0]), f32([2.0, 0.5])]
    rows1 = [[0, 1, 2, 3, 4, 5, 3, 6], [2, 3, 3]]
    w1 = [f32([1.0, -1.0, 0.0, 1.0, 1.0, 0.0, -1.0, -0.0]), f32([0.0, -1.0, 1.0])]
    seen = [[], [3, 50, 90, 0, 60, 4, 12, 99], []]
    counts = {"+inf": 5, "positive": 6, "zero": 6, "negative": 5, "-inf": 4, "nan": 6}
    # k = 3: among the +inf ties; 26: between the last number and the first NaN; 28: among the NaNs; 4: among query 2's six NaNs
    return Case("nonfinite", R.Table(rows1, w1), R.Table(rows2, w2, R.RECIP, 1.0), 100, [0, 0, 1], [3, 26, 28, 4, 40], seen,
                counts=counts)


# ---- 2d: candidate counts around k

COUNT_CASES = {1: (1, 2), 2: (1, 2, 3), 255: (254, 255, 256), 256: (255, 256), 257: (256,)}


def count_case(c):
    """c candidates with distinct sums behind 3 reached items that the seen row hides"""
    rng = np.random.default_rng(40 + c)
    items = rng.choice(900, c + 3, replace=False)
    w = rng.permutation(np.arange(1, c + 4)).astype(np.float32) / 8
    return Case("count_%d" % c, R.Table([[0]]), R.Table([items], [w]), 900, [0], COUNT_CASES[c], [items[[0, c // 2 + 1, c + 2]]], c=c)


# ---- 2e: item extremes

def extremes_case():
    """n_items = 2^31 - 1; item 2^31 - 2, whose blocked key ~item lies next to the free slot's INT32_MIN, as a candidate and as a
    seen item; weights of 0.5 and 1.0, so that it ties with item 0 and others; seen rows of unreached items congruent to the reached
    ones modulo 512 and 4096"""
    top = MAX_ITEMS - 1
    rows2 = [[top, 0, 5, top - 1, 511, 512, 1 << 30, (1 << 30) + 512, 1023, top - 512], [0, top, 7, 5 * 4096 + 5, top - 4096]]
    w2 = [f32([1.0, 1.0, 0.5, 1.0, 0.5, 1.0, 0.5, 1.0, 1.0, 0.5]), f32([0.5, 0.5, 1.0, 1.0, 0.5])]
    reached = sorted(set(rows2[0]) | set(rows2[1]))
    collide = [j + 4096 * m if j < (1 << 30) else j - 4096 * m for j in reached for m in (7, 8, 9)]
    assert not set(collide) & set(reached)
    rows = [0, 0, 1, 2, 1, 2]
    seen = [[], [top, 0], collide, [0], [top, top - 1, top], [top]]
    return Case("item_extremes", R.Table([[0], [0, 1], [1]]), R.Table(rows2, w2), MAX_ITEMS, rows, [1, 3, 256], seen, top=top)


# ---- 3a: staging boundaries of the hop-1 row

STAGE_LENGTHS = (255, 256, 257, 512, 513, 769)
STAGE_BOUNDARIES = (256, 512, 768)
BIG = 2.0 ** 40


def staging_case():
    """Hop-1 rows that end at and next to the 256-entry staging chunks.  Around boundary c a marker: list X_c with hop-1 weight +2^40
    at position c - 1, an ordinary list Y_c on mostly the same items at position c, X_c again with -2^40 a few positions later; a row
    that ends at position c has -2^40 at c - 2, Y_c at c - 1 and +2^40 at c.  Beside 2^40 x an addend of order 1 is rounded to 2^-13,
    so (s + X) + Y and (s + Y) + X differ, and the opposite weight brings the difference back into sight.  notes['planted'] lists
    (hop-1 row, c)."""
    rng = np.random.default_rng(21)
    n_items, n_plain = 160, 10
    rows2 = [rng.choice(n_items, int(n), replace=False) for n in rng.integers(40, 61, n_plain)]
    w2 = [rng.uniform(0.1, 1.9, len(r)).astype(np.float32) for r in rows2]
    marker = {}
    for c in STAGE_BOUNDARIES:
        x = rng.choice(n_items, 120, replace=False)
        y = np.concatenate([x[:100], rng.choice(np.setdiff1d(np.arange(n_items), x), 15, replace=False)])
        marker[c] = (len(rows2), len(rows2) + 1)
        rows2 += [x, rng.permutation(y)]
        w2 += [rng.uniform(0.5, 1.0, 120).astype(np.float32), rng.uniform(0.1, 1.9, 115).astype(np.float32)]
    rows1, w1, planted = [], [], []
    for n in STAGE_LENGTHS:
        src, w = rng.integers(0, n_plain, n), rng.uniform(0.5, 1.5, n).astype(np.float32)
        for c in STAGE_BOUNDARIES:
            x, y = marker[c]
            if n >= c + 2:
                later = min(c + 5, n - 1)
                src[[c - 1, c, later]], w[[c - 1, later]] = [x, y, x], [BIG, -BIG]
            elif n == c + 1:
                src[[c - 2, c - 1, c]], w[[c - 2, c]] = [x, y, x], [-BIG, BIG]
            else:
                continue
            planted.append((len(rows1), c))
        rows1.append(src)
        w1.append(w)
    return Case("staging", R.Table(rows1, w1), R.Table(rows2, w2), n_items, range(len(rows1)), [256, 10], planted=planted,
                marker=marker)


def exchanged(table, row, a, b):
    """the table with positions a and b of one row exchanged"""
    rows, weights = [r.copy() for r in table.rows], [w.copy() for w in table.weights]
    rows[row][[a, b]], weights[row][[a, b]] = rows[row][[b, a]], weights[row][[b, a]]
    return R.Table(rows, weights, table.transform, table.scale)


# ---- 3b: hop-2 list lengths at the thread-count edges

LIST_LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513)
FLANKS = (20, 33)


def lengths_case():
    """query i: the list of LIST_LENGTHS[i] alone; query 14 + i: the same list between two short ones that overlap it"""
    rng = np.random.default_rng(22)
    n_items = 1200
    rows2 = [rng.choice(n_items, n, replace=False) for n in LIST_LENGTHS + FLANKS]
    w2 = [rng.uniform(-2.0, 0.9, len(r)).astype(np.float32) for r in rows2]
    a, b = len(LIST_LENGTHS), len(LIST_LENGTHS) + 1
    rows1 = [[i] for i in range(len(LIST_LENGTHS))] + [[a, i, b] for i in range(len(LIST_LENGTHS))]
    return Case("list_lengths", R.Table(rows1), R.Table(rows2, w2, R.RECIP, 1.0), n_items, range(len(rows1)), [256, 10])


def lengths_wave(n, flanked):
    """whether the query of list length n is walked by one wave as built: the bound is the entries it meets"""
    return n + (sum(FLANKS) if flanked else 0) + 1 <= WAVE_SLOTS


# ---- 3c: awkward neighbours

NEIGHBOUR_ROWS = ("empty first", "empty between", "empty last", "empty at 255", "empty at 256", "empty at 255 and 256", "same source twice",
                  "same source at 255 and 256", "only empty lists", "257 empty lists", "one item 200 times", "200 times between two lists")


def neighbours_case():
    """hop 1 weighted (RECIP), hop 2 unweighted with repeats: lists 0 and 5 are empty, list 4 names item 7 two hundred times"""
    rng = np.random.default_rng(23)
    n_items = 300
    rep = rng.permutation(np.concatenate([np.full(200, 7), [3, 9, 250]]))
    rows2 = [[], rng.integers(0, n_items, 100), rng.integers(0, n_items, 90), rng.integers(0, n_items, 64), rep, []]
    long_row = lambda: rng.integers(1, 4, 300)  # noqa: E731
    at = lambda r, **put: [put.get("p%d" % i, int(s)) for i, s in enumerate(r)]  # noqa: E731
    rows1 = [[0, 1, 2], [1, 0, 2], [1, 2, 0], at(long_row(), p255=0), at(long_row(), p256=0), at(long_row(), p255=0, p256=5),
             [1, 2, 2, 1], at(long_row(), p255=2, p256=2), [0, 5, 0], [0, 5] * 128 + [0], [4], [1, 4, 2]]
    w1 = [rng.uniform(-2.0, 0.9, len(r)).astype(np.float32) for r in rows1]
    seen = [[] for _ in rows1]
    seen[1], seen[10] = [int(rows2[1][0]), 299], [9]
    assert len(rows1) == len(NEIGHBOUR_ROWS)
    return Case("neighbours", R.Table(rows1, w1, R.RECIP, 1.0), R.Table(rows2), n_items, range(len(rows1)), [256, 5], seen)


# ---- 3e: tables filled to bound + 1 == slots at the real class limits

FULL_REACHED = 300


def full_tables_case():
    """per class limit L of 512, 4096, 13056 two queries over one list of 300 items: seen rows of distinct items that are never
    reached, drawn at random (no long run of congruent ones), bring the bound to L - 1, the class's last fit, and to L"""
    rng = np.random.default_rng(24)
    n_items = 60000
    items = rng.choice(n_items, FULL_REACHED, replace=False)
    hop2 = R.Table([items], [rng.uniform(-2.0, 0.9, FULL_REACHED).astype(np.float32)], R.RECIP, 1.0)
    rest = rng.permutation(np.setdiff1d(np.arange(n_items), items))
    seen, at = [], 0
    for limit in (WAVE_SLOTS, MID_SLOTS, MAX_SLOTS):
        for bound in (limit - 1, limit):
            seen.append(rest[at:at + bound - FULL_REACHED])
            at += 100
    return Case("full_tables", R.Table([[0]]), hop2, n_items, [0] * 6, [256, 7], seen,
                bounds=[511, 512, 4095, 4096, 13055, 13056], classes=["wave", "mid", "mid", "max", "max", "global"])


BUILDERS = {"sum_exponent": exponent_case, "sum_sign": sign_case, "plateau_300": plateau_case, "tie_straddle": straddle_case,
            "unweighted": unweighted_case, "nonfinite": nonfinite_case, "item_extremes": extremes_case, "staging": staging_case,
            "list_lengths": lengths_case, "neighbours": neighbours_case, "full_tables": full_tables_case}
BUILDERS.update({"sum_byte_%d" % b: functools.partial(sum_byte_case, b) for b in range(6)})
BUILDERS.update({"item_byte_%d" % b: functools.partial(item_byte_case, b) for b in range(4)})
BUILDERS.update({"count_%d" % c: functools.partial(count_case, c) for c in COUNT_CASES})

SELECT_CASES = DEPTH_CASES + ("plateau_300", "tie_straddle", "unweighted", "nonfinite") + tuple("count_%d" % c for c in COUNT_CASES) + \
    ("item_extremes",)
WALK_CASES = ("staging", "list_lengths", "neighbours")  # full_tables brings its own classes and runs as built


@functools.lru_cache(maxsize=None)
def case(name):
    c = BUILDERS[name]()
    assert c.name == name
    return c


def run_case(name, form):
    """every call of the case in one form: the reference's rows, and the split the header's bound gives"""
    from gorse_amd import capi
    c = case(name)
    n_items, seen, hook = in_form(c, form)
    sp, si = R.seen_csr(seen) if seen is not None else (None, None)
    cls = classes(c, form)
    capi.set_nbr(hook, 0)
    h = capi.NbrRecommender(n_items)
    c.hop1.set_on(h, R.HOP1)
    c.hop2.set_on(h, R.HOP2)
    got = {}
    for k in c.ks:
        got[k] = h.recommend(c.rows, k, sp, si)
        R.assert_same(got[k], reference(name, k), (name, form, k))
        assert h.recommend_stats()[:2] == (len(cls) - cls.count("global"), cls.count("global")), (name, form, k)
    h.close()
    return got
