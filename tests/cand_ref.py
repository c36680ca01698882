"""The candidate chain's stage rule (include/gorse_hip.h, "the candidate chain") restated in plain Python over index lists:
RecommendSequential with limit = 0 (logics/recommend.go:135-156) for a block of queries.  A stage's lists come from outside: the
list stages pass theirs, and mf_lists / nbr_lists take them from the existing public host-to-host calls (MF.recommend under the BASE
rows, NbrRecommender.recommend under the concatenated current rows), never from the chain."""
import numpy as np


def csr(rows, dtype=np.int32):
    ptr = np.zeros(len(rows) + 1, np.int64)
    for t, r in enumerate(rows):
        ptr[t + 1] = ptr[t] + len(r)
    flat = np.array([x for r in rows for x in r], dtype) if ptr[-1] else np.zeros(0, dtype)
    return ptr, flat


def bits(x):
    """a double's bits"""
    return int(np.array([x], np.float64).view(np.uint64)[0])


class Chain:
    def __init__(self, n_queries, base_rows=None):
        self.n = n_queries
        self.base = [[int(i) for i in r] for r in base_rows] if base_rows is not None else [[] for _ in range(n_queries)]
        self.cur = [list(r) for r in self.base]  # concatenated, unsorted: what the host route keeps
        self.cand = [[] for _ in range(n_queries)]  # (item, score bits, stage)
        self.stage = 0

    def add(self, lists, k, keep=None):
        """lists[t] = [(item, score as float64), ...] in the stage's final order"""
        for t in range(self.n):
            excluded, kept = set(self.cur[t]), []
            for item, score in lists[t]:
                if len(kept) == k:
                    break
                if item in excluded or (keep is not None and not keep[item]):
                    continue
                kept.append((int(item), bits(score), self.stage))
            self.cand[t] += kept
            self.cur[t] += [c[0] for c in kept]
        self.stage += 1

    def add_shared(self, items, scores, k, keep=None):
        one = list(zip(items, scores))
        self.add([one] * self.n, k, keep)

    def exclusion(self):
        return csr([sorted(r) for r in self.cur])

    def seen(self):
        """the rows as the host route hands them to the next call"""
        return csr(self.cur)

    def finished(self, keep=None):
        rows = [[c for c in r if keep is None or keep[c[0]]] for r in self.cand]
        ptr, items = csr([[c[0] for c in r] for r in rows])
        _, sc = csr([[c[1] for c in r] for r in rows], np.uint64)
        _, st = csr([[c[2] for c in r] for r in rows], np.uint8)
        return ptr, items, sc, st


def rows_to_lists(items, scores, counts):
    return [[(int(items[t, r]), float(scores[t, r])) for r in range(int(counts[t]))] for t in range(items.shape[0])]


def mf_lists(mf, users, k, item_ok, chain):
    """MF.recommend under the chain's BASE rows (pipeline.go:200); the score is the float widened to double"""
    sp, si = csr(chain.base)
    n = chain.n if users is None else users
    return rows_to_lists(*mf.recommend(n, k, item_ok, sp, si))


def nbr_lists(nbr, rows, k, chain):
    """NbrRecommender.recommend under the concatenated current rows"""
    sp, si = chain.seen()
    n = chain.n if rows is None else rows
    return rows_to_lists(*nbr.recommend(n, k, sp, si))


def assert_same(chain_handle, ref, keep=None, what=""):
    """a finished device chain against the restatement, every bit"""
    ptr, items, scores, stages = chain_handle.get()
    eptr, eitems, escores, estages = ref.finished(keep)
    assert np.array_equal(ptr, eptr), (what, "row pointer")
    assert np.array_equal(items, eitems), (what, "items")
    assert np.array_equal(scores.view(np.uint64), escores), (what, "score bits")
    assert np.array_equal(stages, estages), (what, "stage numbers")


def assert_exclusion(chain_handle, ref, what=""):
    ptr, items = chain_handle.exclusion()
    eptr, eitems = ref.exclusion()
    assert np.array_equal(ptr, eptr), (what, "exclusion row pointer")
    assert np.array_equal(items, eitems), (what, "exclusion rows")
