"""Python face of the host mirror of model/ctr (gorse_amd/host/gorse_ctr.*, in libgorse_host.so): the factorization
machine's Fit loop and EvaluateClassification with their Go names, like cf.py for model/cf.  The model's numerics run on the
MI355X through the gorse_fm_* entry points; nothing here computes them on the CPU."""
import ctypes as C

import numpy as np

from . import cf

_f32p, _i32p, _i64p = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
_u16p = C.POINTER(C.c_uint16)
SGD, Adam = 0, 1
_configured = False


def host():
    global _configured
    H = cf.host()
    if not _configured:
        H.gh_ctr_metric.restype = C.c_float
        H.gh_ctr_metric.argtypes = [C.c_int32, _f32p, C.c_int32, _f32p, C.c_int32]
        H.gh_ctr_dataset_new.restype = C.c_void_p
        H.gh_ctr_dataset_new.argtypes = [C.c_int64]
        H.gh_ctr_dataset_free.argtypes = [C.c_void_p]
        H.gh_ctr_dataset_add.argtypes = [C.c_void_p, C.c_int64, _i64p, _i32p, _f32p, _f32p]
        H.gh_fm_new.restype = C.c_void_p
        H.gh_fm_new.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_int32, C.c_int64]
        H.gh_fm_free.argtypes = [C.c_void_p]
        H.gh_fm_fit.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, _i32p, _f32p]
        H.gh_fm_evaluate.argtypes = [C.c_void_p, C.c_void_p, _f32p]
        H.gh_fm_log.argtypes = [C.c_void_p, _i32p, _f32p, _f32p, C.c_int32]
        H.gh_fm_params.argtypes = [C.c_void_p, _f32p, _f32p, _f32p]
        H.gh_ctr_dataset_set_embeddings.argtypes = [C.c_void_p, C.c_int32, _i32p, C.POINTER(_u16p)]
        H.gh_fm_field_params.argtypes = [C.c_void_p, C.c_int32, _f32p, _f32p, _f32p, _f32p, _f32p]
        H.gh_ctr_fm_set_items.argtypes = [C.c_void_p, C.c_int64, _i32p, _i64p, _i32p, _f32p, C.c_int32, C.POINTER(_u16p)]
        H.gh_ctr_fm_rank_users.argtypes = [C.c_void_p, C.c_int64, _i32p, _i64p, _i32p, _f32p, _i64p, _i32p, _i32p, _f32p]
        H.gh_fm_set_test.argtypes = [C.c_void_p, C.c_void_p]
        H.gh_fm_evaluate_resident.argtypes = [C.c_void_p, _f32p]
        H.gh_fm_set_host_evaluate.restype = None
        H.gh_fm_set_host_evaluate.argtypes = [C.c_void_p, C.c_int32]
        H.gh_ctr_samples_new.restype = C.c_void_p
        H.gh_ctr_samples_new.argtypes = [C.c_int64]
        H.gh_ctr_samples_free.argtypes = [C.c_void_p]
        H.gh_ctr_samples_set_side.restype = None
        H.gh_ctr_samples_set_side.argtypes = [C.c_void_p, C.c_int32, C.c_int64, _i32p, _i64p, _i32p, _f32p]
        H.gh_ctr_samples_set_embeddings.restype = None
        H.gh_ctr_samples_set_embeddings.argtypes = [C.c_void_p, C.c_int32, _i32p, C.POINTER(_u16p)]
        H.gh_ctr_samples_add.restype = None
        H.gh_ctr_samples_add.argtypes = [C.c_void_p, C.c_int64, _i32p, _i32p, _f32p]
        H.gh_ctr_samples_materialise.restype = C.c_void_p
        H.gh_ctr_samples_materialise.argtypes = [C.c_void_p]
        H.gh_ctr_dataset_shape.restype = None
        H.gh_ctr_dataset_shape.argtypes = [C.c_void_p, _i64p]
        H.gh_ctr_dataset_read.restype = None
        H.gh_ctr_dataset_read.argtypes = [C.c_void_p, _i64p, _i32p, _f32p, _f32p]
        H.gh_ctr_dataset_read_embeddings.argtypes = [C.c_void_p, C.c_int32, _u16p]
        H.gh_fm_fit_samples.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, _i32p, _f32p]
        _configured = True
    return H


def _f32(a):
    a = np.ascontiguousarray(a, np.float32)
    return a if a.size else np.zeros(1, np.float32)


def _metric(i, pos, neg):
    p, n = _f32(pos), _f32(neg)
    return float(host().gh_ctr_metric(i, p.ctypes.data_as(_f32p), len(pos), n.ctypes.data_as(_f32p), len(neg)))


def Precision(pos, neg):
    return _metric(0, pos, neg)


def Recall(pos, neg):
    return _metric(1, pos, neg)


def Accuracy(pos, neg):
    return _metric(2, pos, neg)


def AUC(pos, neg):
    return _metric(3, pos, neg)


class Score:
    def __init__(self, v):
        self.Precision, self.Recall, self.Accuracy, self.AUC = (float(x) for x in v)

    def __eq__(self, o):
        return (self.Precision, self.Recall, self.Accuracy, self.AUC) == (o.Precision, o.Recall, o.Accuracy, o.AUC)

    def __repr__(self):
        return "Score(Precision=%g, Recall=%g, Accuracy=%g, AUC=%g)" % (self.Precision, self.Recall, self.Accuracy, self.AUC)


class Dataset:
    """dataset.CTRSplit: rows of (feature indices, values, target +-1) over n_features features."""

    def __init__(self, n_features, rows=None):
        self.n_features = int(n_features)
        self.p = C.c_void_p(host().gh_ctr_dataset_new(self.n_features))
        self.n = 0
        self.dims = ()
        if rows is not None:
            self.add_rows(*rows)

    def __del__(self):
        if getattr(self, "p", None):
            host().gh_ctr_dataset_free(self.p)
            self.p = None

    def add_rows(self, indptr, indices, values, target):
        ip = np.ascontiguousarray(indptr, np.int64)
        ii = np.ascontiguousarray(indices, np.int32)
        vv = np.ascontiguousarray(values, np.float32)
        tt = np.ascontiguousarray(target, np.float32)
        if ii.size == 0:
            ii, vv = np.zeros(1, np.int32), np.zeros(1, np.float32)
        host().gh_ctr_dataset_add(self.p, tt.size, ip.ctypes.data_as(_i64p), ii.ctypes.data_as(_i32p),
                                  vv.ctypes.data_as(_f32p), tt.ctypes.data_as(_f32p))
        self.n += tt.size

    def set_embeddings(self, embs):
        """item embeddings of the rows added so far: one Count() x D matrix of bf16 bit patterns (uint16) per field, an
        all-zero row where a sample has none; an empty list removes them"""
        embs = [np.ascontiguousarray(e, np.uint16) for e in embs]
        if any(e.ndim != 2 or e.shape[0] != self.n for e in embs):
            raise ValueError("one Count() x D matrix per field")
        dims = np.array([e.shape[1] for e in embs] or [0], np.int32)
        ptrs = (_u16p * max(1, len(embs)))(*[e.ctypes.data_as(_u16p) for e in embs])
        host().gh_ctr_dataset_set_embeddings(self.p, len(embs), dims.ctypes.data_as(_i32p), ptrs)
        self.dims = tuple(int(e.shape[1]) for e in embs)

    def Count(self):
        return self.n

    def rows(self):
        """(indptr, indices, values, target, [one Count() x D uint16 matrix per field]) as the set holds them"""
        shape = np.zeros(3, np.int64)
        host().gh_ctr_dataset_shape(self.p, shape.ctypes.data_as(_i64p))
        n, nnz, nf = (int(x) for x in shape)
        ptr, idx = np.zeros(n + 1, np.int64), np.zeros(max(1, nnz), np.int32)
        val, tgt = np.zeros(max(1, nnz), np.float32), np.zeros(max(1, n), np.float32)
        host().gh_ctr_dataset_read(self.p, ptr.ctypes.data_as(_i64p), idx.ctypes.data_as(_i32p), val.ctypes.data_as(_f32p),
                                   tgt.ctypes.data_as(_f32p))
        embs = []
        for k in range(nf):
            D = host().gh_ctr_dataset_read_embeddings(self.p, k, None)
            e = np.zeros((max(1, n), D), np.uint16)
            host().gh_ctr_dataset_read_embeddings(self.p, k, e.ctypes.data_as(_u16p))
            embs.append(e[:n])
        return ptr, idx[:nnz], val[:nnz], tgt[:n], embs


class SampleDataset:
    """The reference's own form of a CTR data set (model/ctr/data.go:152-267) without context labels: users and items as label
    rows (ids and labels are feature indices, negative = unknown to the index, as FM.SetItems takes them), one n_items x D
    uint16 (bf16) table per embedding field, and per sample (user row, item row, target).  A training set and its test set
    share one item side."""

    def __init__(self, n_features, user_ids, user_rows, item_ids, item_rows, embs=(), samples=None):
        self.n_features = int(n_features)
        self.p = C.c_void_p(host().gh_ctr_samples_new(self.n_features))
        self.n = 0
        for side, (ids, rows) in enumerate(((user_ids, user_rows), (item_ids, item_rows))):
            ids, ptr, lab, val = FM._label_rows(ids, rows)
            host().gh_ctr_samples_set_side(self.p, side, ids.size, ids.ctypes.data_as(_i32p), ptr.ctypes.data_as(_i64p),
                                           lab.ctypes.data_as(_i32p), val.ctypes.data_as(_f32p))
        embs = [np.ascontiguousarray(e, np.uint16) for e in embs]
        if any(e.ndim != 2 or e.shape[0] != len(item_rows) for e in embs):
            raise ValueError("one n_items x D table per field")
        dims = np.array([e.shape[1] for e in embs] or [0], np.int32)
        ptrs = (_u16p * max(1, len(embs)))(*[e.ctypes.data_as(_u16p) for e in embs])
        host().gh_ctr_samples_set_embeddings(self.p, len(embs), dims.ctypes.data_as(_i32p), ptrs)
        self.dims = tuple(int(e.shape[1]) for e in embs)
        if samples is not None:
            self.add_samples(*samples)

    def __del__(self):
        if getattr(self, "p", None):
            host().gh_ctr_samples_free(self.p)
            self.p = None

    def add_samples(self, user, item, target):
        u, i = np.ascontiguousarray(user, np.int32), np.ascontiguousarray(item, np.int32)
        t = np.ascontiguousarray(target, np.float32)
        if u.size != t.size or i.size != t.size:
            raise ValueError("one user, one item and one target per sample")
        if t.size:
            host().gh_ctr_samples_add(self.p, t.size, u.ctypes.data_as(_i32p), i.ctypes.data_as(_i32p), t.ctypes.data_as(_f32p))
        self.n += t.size

    def Count(self):
        return self.n

    def Materialise(self):
        """Dataset.Get for every sample: the Dataset the padded route takes"""
        p = host().gh_ctr_samples_materialise(self.p)
        if not p:
            raise ValueError("malformed samples")
        d = Dataset.__new__(Dataset)
        d.n_features, d.p, d.n, d.dims = self.n_features, C.c_void_p(p), self.n, self.dims
        return d


class FM:
    """ctr.AFM (model/ctr/fm.go), trained and scored on the device; a training set with item embeddings (Dataset.set_embeddings)
    trains the attention branch as well."""

    def __init__(self, nFactors=8, nEpochs=10, batchSize=1024, lr=0.01, reg=0.0, optimizer=Adam, seed=0):
        self.d = int(nFactors)
        self.p = C.c_void_p(host().gh_fm_new(self.d, nEpochs, batchSize, lr, reg, optimizer, seed))
        self.nf = 0
        self.dims = ()

    def __del__(self):
        if getattr(self, "p", None):
            host().gh_fm_free(self.p)
            self.p = None

    def Fit(self, train, test, Verbose=10, Patience=0, cancel=None):
        s = np.zeros(4, np.float32)
        cp = cancel.ctypes.data_as(_i32p) if cancel is not None else None
        rc = host().gh_fm_fit(self.p, train.p, test.p, Verbose, Patience, cp, s.ctypes.data_as(_f32p))
        if rc != 0:
            raise cf.HostError(rc)
        self.nf = train.n_features
        self.dims = train.dims
        return Score(s)

    def FitSamples(self, train, test, Verbose=10, Patience=0, cancel=None):
        """Fit from SampleDatasets: the item side goes to the device once and stays resident (RankUsers works afterwards
        without SetItems), per sample three numbers; every bit of the result is Fit's on the Materialise()d sets"""
        s = np.zeros(4, np.float32)
        cp = cancel.ctypes.data_as(_i32p) if cancel is not None else None
        rc = host().gh_fm_fit_samples(self.p, train.p, test.p, Verbose, Patience, cp, s.ctypes.data_as(_f32p))
        if rc != 0:
            raise cf.HostError(rc)
        self.nf = train.n_features
        self.dims = train.dims
        return Score(s)

    def Evaluate(self, test):
        s = np.zeros(4, np.float32)
        rc = host().gh_fm_evaluate(self.p, test.p, s.ctypes.data_as(_f32p))
        if rc != 0:
            raise cf.HostError(rc)
        return Score(s)

    def SetTest(self, test):
        """makes the test split resident on the device for EvaluateResident (Fit does it itself for its own test set)"""
        rc = host().gh_fm_set_test(self.p, test.p)
        if rc != 0:
            raise cf.HostError(rc)

    def EvaluateResident(self):
        """EvaluateClassification of the resident split, scored and counted on the device"""
        s = np.zeros(4, np.float32)
        rc = host().gh_fm_evaluate_resident(self.p, s.ctypes.data_as(_f32p))
        if rc != 0:
            raise cf.HostError(rc)
        return Score(s)

    def SetHostEvaluate(self, on):
        """True: Fit evaluates through Evaluate's route (gather, upload, download, sort on the host) instead of the resident split"""
        host().gh_fm_set_host_evaluate(self.p, int(bool(on)))

    def log(self):
        """[(epoch, cost, AUC)] of every evaluation of the last Fit"""
        cap = 4096
        e, c, a = np.zeros(cap, np.int32), np.zeros(cap, np.float32), np.zeros(cap, np.float32)
        n = host().gh_fm_log(self.p, e.ctypes.data_as(_i32p), c.ctypes.data_as(_f32p), a.ctypes.data_as(_f32p), cap)
        return [(int(e[i]), float(c[i]), float(a[i])) for i in range(min(n, cap))]

    def params(self):
        B = np.zeros(1, np.float32)
        W = np.zeros(self.nf, np.float32)
        V = np.zeros((self.nf, self.d), np.float32)
        host().gh_fm_params(self.p, B.ctypes.data_as(_f32p), W.ctypes.data_as(_f32p), V.ctypes.data_as(_f32p))
        return B[0], W, V

    def field_params(self, field):
        """(H, Wa, ba, We, be) of one embedding field after Fit"""
        D, d = self.dims[field], self.d
        arrs = [np.zeros(shp, np.float32) for shp in ((d, D), (D, d), (d,), (D, d), (d,))]
        host().gh_fm_field_params(self.p, field, *[a.ctypes.data_as(_f32p) for a in arrs])
        return tuple(arrs)

    @staticmethod
    def _label_rows(ids, rows):
        """ids: each entity's own feature index (negative: unknown to the index); rows: per entity [(label index, value)] with a
        negative index for an unknown label"""
        ids = np.ascontiguousarray(ids, np.int32)
        ptr = np.zeros(len(rows) + 1, np.int64)
        ptr[1:] = np.cumsum([len(r) for r in rows])
        lab = np.array([l for r in rows for l, _ in r] or [0], np.int32)
        val = np.array([v for r in rows for _, v in r] or [0], np.float32)
        if ids.size != len(rows):
            raise ValueError("one id per label row")
        return ids, ptr, lab, val

    def SetItems(self, ids, rows, embs=()):
        """the resident catalogue of RankUsers: items as label rows, one n_items x D uint16 (bf16) table per field"""
        ids, ptr, lab, val = self._label_rows(ids, rows)
        embs = [np.ascontiguousarray(e, np.uint16) for e in embs]
        ptrs = (_u16p * max(1, len(embs)))(*[e.ctypes.data_as(_u16p) for e in embs])
        rc = host().gh_ctr_fm_set_items(self.p, ids.size, ids.ctypes.data_as(_i32p), ptr.ctypes.data_as(_i64p),
                                        lab.ctypes.data_as(_i32p), val.ctypes.data_as(_f32p), len(embs), ptrs)
        if rc != 0:
            raise cf.HostError(rc)

    def RankUsers(self, ids, rows, cands):
        """users as label rows and each one's candidates (catalogue rows) -> per user [(item, score)], best first"""
        ids, ptr, lab, val = self._label_rows(ids, rows)
        cptr = np.zeros(len(cands) + 1, np.int64)
        cptr[1:] = np.cumsum([len(c) for c in cands])
        flat = np.array([c for cl in cands for c in cl] or [0], np.int32)
        items, scores = np.zeros(max(1, int(cptr[-1])), np.int32), np.zeros(max(1, int(cptr[-1])), np.float32)
        rc = host().gh_ctr_fm_rank_users(self.p, ids.size, ids.ctypes.data_as(_i32p), ptr.ctypes.data_as(_i64p),
                                         lab.ctypes.data_as(_i32p), val.ctypes.data_as(_f32p), cptr.ctypes.data_as(_i64p),
                                         flat.ctypes.data_as(_i32p), items.ctypes.data_as(_i32p), scores.ctypes.data_as(_f32p))
        if rc != 0:
            raise cf.HostError(rc)
        return [[(int(items[j]), scores[j]) for j in range(int(cptr[t]), int(cptr[t + 1]))] for t in range(len(cands))]
