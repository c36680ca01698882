"""The list rule of QueryItemToItem / QueryUserToUser (item_to_item.go:72-86, user_to_user.go:63-80) in plain Python, and the host
route to a neighbour table through public calls only: search to the host, the rule, a CSR for gorse_nbr_set_table.  This is what
gorse_nbr_set_table_from_topk / _from_sparse (include/gorse_hip.h) must equal bit for bit."""
import numpy as np


def apply_rule(idx, raw, cnt, source, n, positive_only):
    """walk the list in order: skip the entry whose index is the source, skip raw <= 0 when positive_only (a NaN is not <= 0 and is
    kept), stop after n kept entries -> (indices, raw weights)"""
    keep_i, keep_w = [], []
    for e in range(int(cnt)):
        j, w = int(idx[e]), np.float32(raw[e])
        if j == source:
            continue
        if positive_only and w <= 0:
            continue
        keep_i.append(j)
        keep_w.append(w)
        if len(keep_i) == n:
            break
    return keep_i, keep_w


def table_from_lists(sources, lists, n, positive_only):
    """sources: one stored row (or < 0: an empty row) per table row; lists: source -> (idx, raw, cnt).  -> (indptr, indices, weights)"""
    ptr, ix, w = [0], [], []
    for s in sources:
        if s >= 0:
            ki, kw = apply_rule(*lists[int(s)], int(s), n, positive_only)
            ix += ki
            w += kw
        ptr.append(len(ix))
    return np.array(ptr, np.int64), np.array(ix, np.int32), np.array(w, np.float32)


def dense_lists(index, X, sources, n):
    """the public search for the stored rows as query vectors, k = n + 1, prune0 = 0; raw = -dist"""
    valid = sorted(set(int(s) for s in sources if s >= 0))
    if not valid:
        return {}
    idx, dist, cnt = index.search_vector(X[valid], n + 1)
    return {s: (idx[t], -dist[t], cnt[t]) for t, s in enumerate(valid)}


def sparse_lists(index, ptr, idx, val, sources, n):
    """the public search for the stored rows as queries, exclude = None, k = n + 1; raw = the score"""
    valid = sorted(set(int(s) for s in sources if s >= 0))
    if not valid:
        return {}
    qp = np.zeros(len(valid) + 1, np.int64)
    qp[1:] = np.cumsum([ptr[s + 1] - ptr[s] for s in valid])
    qi = np.concatenate([idx[ptr[s]:ptr[s + 1]] for s in valid]).astype(np.uint32)
    qv = np.concatenate([val[ptr[s]:ptr[s + 1]] for s in valid]).astype(np.float32)
    ri, rs, rc = index.search(qp, qi, qv, n + 1)
    return {s: (ri[t], rs[t], rc[t]) for t, s in enumerate(valid)}
