"""What the tests of gorse_fm_rank_users restate in Python: the order of a ranked list, the composed row of a (user, candidate)
pair in BatchPredict's order (model/ctr/fm.go:183-206), and the CSR form of a side's feature rows."""
import numpy as np

f32 = np.float32


def rank_order(scores):
    """positions of one list in ranked order: descending score, equal scores (-0 == +0) by ascending position, NaN scores last
    by ascending position"""
    s = np.asarray(scores, f32)
    nan = np.isnan(s)
    with np.errstate(invalid="ignore"):  # widening a signalling NaN raises the flag; NaNs get a key of their own below
        key = np.where(nan, 0.0, -s.astype(np.float64)) + 0.0  # -(+0) = -0: adding +0 folds the zeros' signs away
    return np.lexsort((np.arange(s.size), key, nan)).astype(np.int32)


def rank_orders(scores, cand_indptr):
    out = np.zeros(len(scores), np.int32)
    for t in range(len(cand_indptr) - 1):
        a, b = int(cand_indptr[t]), int(cand_indptr[t + 1])
        out[a:b] = rank_order(scores[a:b])
    return out


def csr(rows):
    """[(indices, values)] -> (indptr int64, indices int32, values float32)"""
    ptr = np.zeros(len(rows) + 1, np.int64)
    for i, (a, _) in enumerate(rows):
        ptr[i + 1] = ptr[i] + len(a)
    idx = np.concatenate([np.asarray(a, np.int32) for a, _ in rows] + [np.zeros(0, np.int32)])
    val = np.concatenate([np.asarray(b, f32) for _, b in rows] + [np.zeros(0, f32)])
    return ptr, idx.astype(np.int32), val.astype(f32)


def compose(user, user_lead, item, item_lead):
    """the row of one (user, candidate) pair: user lead | item lead | user rest | item rest"""
    (ui, uv), (ii, iv) = user, item
    ui, ii = np.asarray(ui, np.int32), np.asarray(ii, np.int32)
    uv, iv = np.asarray(uv, f32), np.asarray(iv, f32)
    idx = np.concatenate([ui[:user_lead], ii[:item_lead], ui[user_lead:], ii[item_lead:]])
    val = np.concatenate([uv[:user_lead], iv[:item_lead], uv[user_lead:], iv[item_lead:]])
    return idx, val


def compose_plain(user, item):
    """the WRONG order: the user's row, then the item's, without the lead interleave"""
    return compose(user, 0, item, 0)


def pointer(lists):
    ptr = np.zeros(len(lists) + 1, np.int64)
    ptr[1:] = np.cumsum([len(c) for c in lists])
    flat = np.concatenate([np.asarray(c, np.int32) for c in lists] + [np.zeros(0, np.int32)]).astype(np.int32)
    return ptr, flat
