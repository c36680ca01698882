"""Replacement (worker/pipeline.go:573-643) restated in plain Python over lists, sets and float, on top of cand_ref.Chain's
finished rows: the history collected into `positive` and `distinct`, the existing distinct items that are no candidates yet
appended with score 0, the ranked scores of history items decayed by one double multiply, and the list sorted again.  Where the
reference leaves the order open (Go map order of the appended items, the unstable sort.Slice) the rule of include/gorse_hip.h
decides: appended items ascending; descending decayed score, equal doubles and NaNs in the ranker's order.  The ranker's float32
scores come from outside."""
import math

import numpy as np

import cand_ref as R

POSITIVE, READ, STAGE = 1, 2, 255


def collect(history, keep=None):
    """one user's feedback [(item, kind), ...] -> [(item, kind), ...]: distinct, ascending, positive wins, existing items only"""
    positive, distinct = set(), set()
    for item, kind in history:
        if kind == POSITIVE:
            positive.add(int(item))
            distinct.add(int(item))
        elif kind == READ:
            distinct.add(int(item))
    return [(i, POSITIVE if i in positive else READ) for i in sorted(distinct) if keep is None or keep[i]]


def ranker_order(scores):
    """fm_rank_order.hpp: descending score, equal floats by position, NaN last by position"""
    s = [float(x) for x in scores]
    return sorted(range(len(s)), key=lambda i: (1, 0.0) if math.isnan(s[i]) else (0, -s[i]))


class Replaced:
    """chain: a cand_ref.Chain; finish_keep: what finish() was given; history[t] = [(item, kind), ...]; keep: the existing items"""

    def __init__(self, chain, history, finish_keep=None, keep=None):
        ptr, items, scores, stages = chain.finished(finish_keep)
        self.n = chain.n
        self.rows = [collect(h, keep) for h in history]
        self.old = [list(zip(items[ptr[t]:ptr[t + 1]].tolist(), scores[ptr[t]:ptr[t + 1]].tolist(), stages[ptr[t]:ptr[t + 1]].tolist()))
                    for t in range(self.n)]
        self.cand = []
        for t in range(self.n):
            have = {c[0] for c in self.old[t]}
            self.cand.append(self.old[t] + [(i, 0, STAGE) for i, _ in self.rows[t] if i not in have])

    def finished(self):
        ptr, items = R.csr([[c[0] for c in r] for r in self.cand])
        _, sc = R.csr([[c[1] for c in r] for r in self.cand], np.uint64)
        _, st = R.csr([[c[2] for c in r] for r in self.cand], np.uint8)
        return ptr, items, sc, st

    def replacement(self):
        ptr, items = R.csr([[e[0] for e in r] for r in self.rows])
        _, kinds = R.csr([[e[1] for e in r] for r in self.rows], np.uint8)
        return ptr, items, kinds

    def stats(self):
        """(entries appended, positive entries, read entries of the replacement rows)"""
        flat = [e for r in self.rows for e in r]
        return (sum(len(c) - len(o) for c, o in zip(self.cand, self.old)), sum(1 for e in flat if e[1] == POSITIVE),
                sum(1 for e in flat if e[1] == READ))

    def kinds(self):
        """per candidate of the grown rows: 0, POSITIVE or READ"""
        return [[dict(self.rows[t]).get(c[0], 0) for c in self.cand[t]] for t in range(self.n)]

    def decayed(self, scores, positive_decay, read_decay):
        """scores: the ranker's float32 scores, flat over the grown rows -> (float64 decayed scores, int32 order), flat"""
        ptr = self.finished()[0]
        final, order = np.zeros(len(scores), np.float64), np.zeros(len(scores), np.int32)
        for t, kinds in enumerate(self.kinds()):
            p0 = int(ptr[t])
            s = scores[p0:p0 + len(kinds)]
            f = []
            for x, kind in zip(s, kinds):
                v = float(np.float32(x))
                if kind == POSITIVE:
                    v = v * float(positive_decay)
                elif kind == READ:
                    v = v * float(read_decay)
                f.append(v)
            final[p0:p0 + len(f)] = f
            by_ranker = ranker_order(s)
            order[p0:p0 + len(f)] = sorted(by_ranker, key=lambda i: (1, 0.0) if math.isnan(f[i]) else (0, -f[i]))
        return final, order


def assert_same(chain_handle, ref, what=""):
    """a device chain after add_replacement against the restatement, every bit"""
    ptr, items, scores, stages = chain_handle.get()
    eptr, eitems, escores, estages = ref.finished()
    assert np.array_equal(ptr, eptr), (what, "row pointer")
    assert np.array_equal(items, eitems), (what, "items")
    assert np.array_equal(scores.view(np.uint64), escores), (what, "score bits")
    assert np.array_equal(stages, estages), (what, "stage numbers")
    rptr, ritems, rkinds = chain_handle.replacement()
    wptr, witems, wkinds = ref.replacement()
    assert np.array_equal(rptr, wptr), (what, "replacement row pointer")
    assert np.array_equal(ritems, witems), (what, "replacement items")
    assert np.array_equal(rkinds, wkinds), (what, "replacement kinds")
    assert chain_handle.replacement_stats()[:3] == ref.stats(), (what, "counts")
    assert chain_handle.info()[2] == int(eptr[-1]), (what, "info")
