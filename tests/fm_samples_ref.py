"""What the tests of gorse_fm_set_train_samples / gorse_fm_set_test_samples share: the small world (users, items, samples), its
materialisation in numpy (the rows and per-sample embeddings the padded route takes), the numpy restatement of the per-batch
accumulation plan (fm.hip's build_plan applied to the materialised rows) and a Python restatement of Dataset.Get."""
import numpy as np

import fm_attention_ref as A
import fm_rank_ref as K
import fm_ref as R

f32 = np.float32
NF = 203          # W's tail holds 11 elements; features 180.. are never used
SHARED = 100      # the label every user with entries carries
BOTH = 95         # a feature user 7 and item 6 both carry
N_USERS, N_ITEMS, N, BS = 37, 23, 150, 64


def _ids(*v):
    return np.array(v, np.int32)


def _vals(*v):
    return np.array(v, f32)


class World:
    """37 users, 23 items, 150 samples in batches of 64 (the last holds 22).  Users' features lie in [0, 110), items' in
    [90, 180).  User t with odd t leads with its id feature t (lead 1), the others have lead 0; every user but user 0 (no
    entries at all) carries SHARED, so that a batch of 64 rows without user 0 holds 64 positions of one feature: more than one
    pass of the accumulation loop at every lane width (4 entries x 64 / G groups per pass).  User 0 appears in the last batch
    only.  User 5 and item 4 hold a zero-valued entry inside a segment; item 3 has an empty feature row; item 9's embedding row
    is all zero; BOTH is in user 7's and in item 6's row and sample 3 is (7, 6); sample 140 is (0, 3): a row with no entry."""

    def __init__(self, dims=(), n=N, seed=1):
        rng = np.random.default_rng(seed)
        self.dims = tuple(dims)
        self.users, self.ulead = [], np.zeros(N_USERS, np.int32)
        for t in range(N_USERS):
            if t == 0:
                self.users.append((_ids(), _vals()))
                continue
            k = int(rng.integers(0, 4))
            idx = [SHARED] + list(rng.choice(np.arange(40, 90), k, replace=False))
            val = list(rng.normal(0.8, 0.5, k + 1))
            if t % 2:
                idx, val = [t] + idx, [1.0] + val
                self.ulead[t] = 1
            self.users.append((np.array(idx, np.int32), np.array(val, f32)))
        i5, v5 = self.users[5]
        self.users[5] = (np.concatenate([i5[:2], _ids(33), i5[2:]]), np.concatenate([v5[:2], _vals(0.0), v5[2:]]))
        i7, v7 = self.users[7]
        self.users[7] = (np.concatenate([i7, _ids(BOTH)]), np.concatenate([v7, _vals(-0.7)]))
        self.items, self.ilead = [], np.zeros(N_ITEMS, np.int32)
        for c in range(N_ITEMS):
            if c == 3:
                self.items.append((_ids(), _vals()))
                continue
            k = int(rng.integers(1, 5))
            idx = list(rng.choice(np.arange(120, 180), k, replace=False))
            val = list(rng.normal(0.6, 0.6, k))
            if c % 3 != 2:
                idx, val = [101 + c % 6] + idx, [1.0] + val  # the item-id entry; 101..106 lie in the users' range
                self.ilead[c] = 1
            self.items.append((np.array(idx, np.int32), np.array(val, f32)))
        i4, v4 = self.items[4]
        self.items[4] = (np.concatenate([i4[:1], _ids(150), i4[1:]]), np.concatenate([v4[:1], _vals(0.0), v4[1:]]))
        i6, v6 = self.items[6]
        self.items[6] = (np.concatenate([i6, _ids(BOTH)]), np.concatenate([v6, _vals(1.3)]))
        self.embs = []
        for D in self.dims:
            e = rng.normal(0, 1, (N_ITEMS, D)).astype(f32)
            e[9] = 0
            self.embs.append(A.to_bf16(e))
        self.user = rng.integers(1, N_USERS, n).astype(np.int32)
        self.item = rng.integers(0, N_ITEMS, n).astype(np.int32)
        fixed = {3: (7, 6), 10: (5, 4), 11: (12, 3), 12: (13, 9), 130: (0, 5), 140: (0, 3)}
        for i, (u, c) in fixed.items():
            if i < n:
                self.user[i], self.item[i] = u, c
        self.target = np.where(rng.random(n) < 0.5, 1.0, -1.0).astype(f32)
        self.n = n

    def head(self, n):
        """the world with its first n samples only"""
        w = World.__new__(World)
        w.__dict__.update(self.__dict__)
        w.user, w.item, w.target, w.n = self.user[:n].copy(), self.item[:n].copy(), self.target[:n].copy(), n
        return w

    def user_csr(self):
        return K.csr(self.users)

    def item_csr(self):
        return K.csr(self.items)

    def rows(self):
        return [K.compose(self.users[u], int(self.ulead[u]), self.items[c], int(self.ilead[c])) for u, c in zip(self.user, self.item)]

    def materialise(self, extra=0):
        """(idx, val, target, embs) of the padded route: the composed rows zero-padded to the longest row + extra, the
        embeddings gathered per sample"""
        rows = self.rows()
        idx, val = R.pad(rows, max(1, max(len(a) for a, _ in rows)) + extra)
        return idx, val, self.target, [e[self.item] for e in self.embs]


def plan_of_padded(idx, val, bs):
    """fm.hip's build_plan restated on padded rows: per batch the (feature, batch-local row, value) sequence of the positions
    with a nonzero value, sorted by feature then position"""
    out = []
    n, w = idx.shape
    for r0 in range(0, n, bs):
        bi, bv = idx[r0:r0 + bs].reshape(-1), val[r0:r0 + bs].reshape(-1)
        p = np.flatnonzero(bv != 0)
        p = p[np.lexsort((p, bi[p]))]
        out.append((bi[p].astype(np.int32), (p // w).astype(np.int32), bv[p].astype(f32)))
    return out


def dataset_get(user_labels, item_labels, item_embs, n_users, n_items, n_user_labels, u, c):
    """Dataset.Get (model/ctr/data.go:221-267) without context labels, restated: the user-id entry, the item-id entry (offset
    past the users), the user's labels (offset past users and items), the item's labels (offset past the user labels as
    well), and the item's embeddings.  user_labels / item_labels: per row a list of (label id, value)."""
    idx, val, position = [int(u)], [1.0], n_users
    idx.append(position + int(c))
    val.append(1.0)
    position += n_items
    for lab, v in user_labels[u]:
        idx.append(position + int(lab))
        val.append(float(v))
    position += n_user_labels
    for lab, v in item_labels[c]:
        idx.append(position + int(lab))
        val.append(float(v))
    return np.array(idx, np.int32), np.array(val, f32), [e[c] for e in item_embs]


class LabelWorld:
    """A data.go Dataset in sample form: n_users users and n_items items with labels drawn from their own label ranges, one
    embedding per item and field (item 2 has none: an all-zero row), a training and a test list of samples.  Feature indices
    follow the unified index: users | items | user labels | item labels."""

    def __init__(self, dims=(), n_users=19, n_items=11, n_ul=7, n_il=5, n_train=150, n_test=61, seed=3):
        rng = np.random.default_rng(seed)
        self.n_users, self.n_items, self.n_ul, self.n_il = n_users, n_items, n_ul, n_il
        self.n_features = n_users + n_items + n_ul + n_il

        def labels(n, k_labels):
            out = []
            for _ in range(n):
                k = int(rng.integers(0, 4))
                labs = rng.choice(k_labels, k, replace=False)
                out.append([(int(lab), float(f32(v))) for lab, v in zip(labs, rng.normal(0.7, 0.4, k))])
            return out

        self.user_labels, self.item_labels = labels(n_users, n_ul), labels(n_items, n_il)
        self.embs = []
        for D in dims:
            e = rng.normal(0, 1, (n_items, D)).astype(f32)
            e[2] = 0
            self.embs.append(A.to_bf16(e))
        self.train = self._samples(rng, n_train)
        self.test = self._samples(rng, n_test)

    def _samples(self, rng, n):
        return (rng.integers(0, self.n_users, n).astype(np.int32), rng.integers(0, self.n_items, n).astype(np.int32),
                np.where(rng.random(n) < 0.5, 1.0, -1.0).astype(f32))

    def sides(self):
        """(user ids, user rows, item ids, item rows) as feature indices: what ctr.SampleDataset and FM.SetItems take"""
        base = self.n_users + self.n_items
        return (np.arange(self.n_users, dtype=np.int32), [[(base + lab, v) for lab, v in r] for r in self.user_labels],
                self.n_users + np.arange(self.n_items, dtype=np.int32),
                [[(base + self.n_ul + lab, v) for lab, v in r] for r in self.item_labels])

    def get(self, u, c):
        return dataset_get(self.user_labels, self.item_labels, self.embs, self.n_users, self.n_items, self.n_ul, u, c)
