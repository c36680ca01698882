"""gorse_fm_set_items / gorse_fm_rank_users on the MI355X.  The yardstick for scores is the EXISTING predict / predict_embeddings on
the rows this file materialises itself (fm_rank_ref.compose + fm_ref.pad), user by user: every bit must agree, because the
operation order is the same by contract.  Two cases pin the call to the float64 restatement as well (1e-5 of a row's scale, the
project's bar).  The order is compared with fm_rank_ref.rank_order, which test_fm_rank_order_cpu.py checks without a device."""
import numpy as np
import pytest

import fm_attention_ref as A
import fm_rank_ref as K
import fm_ref as R
from gorse_amd import capi

pytestmark = pytest.mark.gpu
f32, f64, u32 = np.float32, np.float64, np.uint32
BAR = 1e-5
NF = 300


# the recipes of test_gpu_fm_attention.py (_model, _embs), restated
def _model(nf, d, dims, seed, sd=0.3, h_sd=0.3, bias_sd=0.1):
    rng = np.random.default_rng(seed)
    B, W, V = f32(rng.normal(0, 0.5)), rng.normal(0, sd, nf).astype(f32), rng.normal(0, sd, (nf, d)).astype(f32)
    fields = []
    for D in dims:
        H, Wa, ba, We, be = A.init_field(rng, D, d, h_sd)
        fields.append((H, Wa, rng.normal(0, bias_sd, d).astype(f32), We, rng.normal(0, bias_sd, d).astype(f32)))
    return B, W, V, fields


def _embs(n, dims, seed, absent_every=7):
    rng = np.random.default_rng(seed)
    out = []
    for D in dims:
        e = rng.normal(0, 1, (n, D)).astype(f32)
        if absent_every:
            e[::absent_every] = 0  # items without an embedding carry an all-zero row (fm.go:555-561)
        out.append(A.to_bf16(e))
    return out


def _handle(nf, d, dims, B, W, V, fields):
    fm = capi.FM(nf, d, embedding_dims=dims)
    fm.set_params(B, W, V)
    for k, fld in enumerate(fields):
        fm.set_embedding_params(k, *fld)
    return fm


def _side(n, lo, hi, seed, kmin=1, kmax=6):
    """n feature rows over [lo, hi) and a lead of 0 or 1 each (0 for an empty row)"""
    rng = np.random.default_rng(seed)
    rows, lead = [], []
    for _ in range(n):
        k = int(rng.integers(kmin, kmax + 1))
        rows.append((rng.choice(np.arange(lo, hi), k, replace=False).astype(np.int32), rng.normal(0.5, 1.0, k).astype(f32)))
        lead.append(min(k, int(rng.integers(0, 2))))
    return rows, np.array(lead, np.int32)


class Case:
    """a model, a catalogue and a block of users; users' features lie in [0, 160), items' in [120, NF): they share [120, 160)"""

    def __init__(self, d, dims, n_items=60, n_users=5, seed=1, model=None, **model_kw):
        self.d, self.dims = d, tuple(dims)
        self.B, self.W, self.V, self.fields = model or _model(NF, d, dims, 100 + seed, **model_kw)
        self.items, self.ilead = _side(n_items, 120, NF, 200 + seed)
        self.users, self.ulead = _side(n_users, 0, 160, 300 + seed)
        self.embs = _embs(n_items, dims, 400 + seed)

    def handle(self, items=True):
        fm = _handle(NF, self.d, self.dims, self.B, self.W, self.V, self.fields)
        if items:
            self.set_items(fm)
        return fm

    def set_items(self, fm):
        fm.set_items(*K.csr(self.items), lead=self.ilead, embs=self.embs)

    def rank(self, fm, cands, bs, **kw):
        uptr, uidx, uval = K.csr(self.users)
        cptr, flat = K.pointer(cands)
        return fm.rank_users(uptr, uidx, uval, cptr, flat, bs, user_lead=self.ulead, **kw)

    def rows(self, t, cl, compose=None):
        """user t's materialised rows for the candidate list cl"""
        if compose is None:
            rows = [K.compose(self.users[t], int(self.ulead[t]), self.items[c], int(self.ilead[c])) for c in cl]
        else:
            rows = [compose(self.users[t], self.items[c]) for c in cl]
        return R.pad(rows)

    def predict(self, fm, idx, val, cl, bs):
        if self.dims:
            return fm.predict_embeddings(idx, val, [e[np.asarray(cl)] for e in self.embs], bs)
        return fm.predict(idx, val)

    def expect(self, fm, cands, bs, compose=None):
        """the existing scoring entry point, one call per user on that user's rows alone"""
        out = [np.zeros(0, f32)]
        for t, cl in enumerate(cands):
            if len(cl):
                idx, val = self.rows(t, cl, compose)
                out.append(self.predict(fm, idx, val, cl, bs))
        return np.concatenate(out).astype(f32)


def _cand_lists(lens, n_items, seed):
    """lists of the given lengths; every list of two or more repeats its first item, and item 7 opens every list"""
    rng = np.random.default_rng(seed)
    out = []
    for n in lens:
        cl = rng.integers(0, n_items, n).astype(np.int32)
        if n >= 1:
            cl[0] = 7
        if n >= 2:
            cl[-1] = cl[0]
        out.append(cl)
    return out


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, f32).view(u32), np.asarray(b, f32).view(u32))


@pytest.fixture(autouse=True)
def _default_hooks():
    capi.lib().gorse_hip_test_set_fm_rank(0, 0)
    yield
    capi.lib().gorse_hip_test_set_fm_rank(0, 0)


# ---- 1. score bits --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(), (3, 4), (63,), (64,), (65,), (200, 64)], ids=str)
@pytest.mark.parametrize("d", [1, 8, 16, 24, 64, 65, 128])
def test_score_bits(d, dims):
    """every G / NF instantiation, column-tile edges, two fields; users with 0, 1, bs, bs + 1 and 2 bs + 3 candidates in one
    call; repeated items inside a list and across users"""
    case = Case(d, dims, seed=d + 7 * len(dims))
    fm = case.handle()
    for bs in (1, 5, 64):
        cands = _cand_lists([0, 1, bs, bs + 1, 2 * bs + 3], len(case.items), bs)
        got, order = case.rank(fm, cands, bs)
        want = case.expect(fm, cands, bs)
        assert got.size == want.size == sum(len(c) for c in cands)
        assert _same_bits(got, want), (bs, int(np.sum(got.view(u32) != want.view(u32))))
        assert np.array_equal(order, K.rank_orders(got, K.pointer(cands)[0]))
        st = fm.rank_stats()
        assert st["rows"] == want.size and st["slices"] == sum(-(-len(c) // bs) for c in cands)


# ---- 2. row composition ---------------------------------------------------------------------------------------------------
def _composition_case(dims):
    case = Case(16, dims, n_items=6, n_users=6, seed=3)
    one = lambda *v: np.array(v, f32)  # noqa: E731
    ids = lambda *v: np.array(v, np.int32)  # noqa: E731
    uv = one(0.7, -1.3, 0.4)
    case.users = [(ids(5, 6, 7), uv), (ids(5, 6, 7), uv), (ids(5, 6, 7), uv), (ids(), one()),
                  (ids(5, 121, 7), one(1.1, 0.0, 2.0)),    # a zero value in the middle of a segment
                  (ids(130, 8), one(0.9, -0.6))]            # feature 130 is in item 5 as well
    case.ulead = ids(0, 1, 3, 0, 1, 1)                      # lead 0 / 1 / the whole row
    iv = one(-0.8, 1.2, 0.5)
    case.items = [(ids(200, 201, 202), iv), (ids(200, 201, 202), iv), (ids(200, 201, 202), iv), (ids(), one()),
                  (ids(200, 201, 203), one(1.4, 0.0, -0.9)), (ids(130, 204), one(1.6, 0.3))]
    case.ilead = ids(0, 1, 3, 0, 2, 1)
    return case


@pytest.mark.parametrize("dims", [(), (3, 4)], ids=str)
def test_row_composition(dims):
    """every user of the case against every item: lead 0 / 1 / whole row on both sides, empty rows, zero values inside a
    segment, a feature on both sides; each row equals the materialised row in fm.go:183-206's order"""
    case = _composition_case(dims)
    fm = case.handle()
    cands = [np.arange(6, dtype=np.int32) for _ in range(6)]
    got, _ = case.rank(fm, cands, 64)
    want = case.expect(fm, cands, 64)
    assert _same_bits(got, want)
    if not dims:  # user 3 x item 3: nothing but the bias
        assert _same_bits(got[3 * 6 + 3], case.B)
    # user_lead = None and lead = None mean zero leads
    uptr, uidx, uval = K.csr(case.users)
    cptr, flat = K.pointer(cands)
    fm.set_items(*K.csr(case.items), lead=None, embs=case.embs)
    got0, _ = fm.rank_users(uptr, uidx, uval, cptr, flat, 64, user_lead=None)
    assert _same_bits(got0, case.expect(fm, cands, 64, compose=K.compose_plain))


def test_the_segment_order_matters():
    """user id | item id | user labels | item labels is not user row ++ item row: on rows with a lead on both sides the plain
    concatenation gives other bits, so a kernel that walked the segments in the wrong order would fail test_row_composition"""
    case = Case(16, (), n_items=30, n_users=4, seed=11)
    case.users, _ = _side(4, 0, 160, 5, kmin=3, kmax=6)
    case.items, _ = _side(30, 120, NF, 6, kmin=3, kmax=6)
    case.ulead, case.ilead = np.ones(4, np.int32), np.ones(30, np.int32)
    fm = case.handle()
    cands = [np.arange(30, dtype=np.int32) for _ in range(4)]
    got, _ = case.rank(fm, cands, 64)
    right = case.expect(fm, cands, 64)
    wrong = case.expect(fm, cands, 64, compose=K.compose_plain)
    assert _same_bits(got, right)
    assert not _same_bits(right, wrong), "the input does not tell the two orders apart"
    assert not _same_bits(got, wrong)


# ---- 3. slices are per user -----------------------------------------------------------------------------------------------
def test_slices_are_per_user():
    case = Case(16, (64,), n_items=120, n_users=2, seed=21, h_sd=1.0)
    fm = case.handle()
    rng = np.random.default_rng(2)
    cands = [rng.permutation(120)[:40].astype(np.int32) for _ in range(2)]
    bs = 64
    # the concatenated 80 rows as ONE batch sequence (slices of 64 + 16) against two users' own slices (40, 40)
    rows = [case.rows(t, cands[t]) for t in range(2)]
    w = max(r[0].shape[1] for r in rows)
    idx = np.concatenate([np.pad(r[0], ((0, 0), (0, w - r[0].shape[1]))) for r in rows])
    val = np.concatenate([np.pad(r[1], ((0, 0), (0, w - r[1].shape[1]))) for r in rows])
    flat = np.concatenate(cands)
    embs = [e[flat] for e in case.embs]
    # on the CPU first: the input must have the gap before the device is asked about it
    shared64, scale = A.predict(case.B, case.W, case.V, case.fields, idx, val, embs, bs)
    own = [A.predict(case.B, case.W, case.V, case.fields, idx[s], val[s], [e[s] for e in embs], bs)
           for s in (slice(0, 40), slice(40, 80))]
    own64, own_scale = np.concatenate([o[0] for o in own]), np.concatenate([o[1] for o in own])
    assert np.max(np.abs(shared64 - own64) / scale) >= 100 * BAR, "the restatement sees no gap on this input"
    got, _ = case.rank(fm, cands, bs)
    assert _same_bits(got, case.expect(fm, cands, bs))                   # two separate predict_embeddings calls
    assert np.all(np.abs(got - own64) <= BAR * own_scale)
    shared = fm.predict_embeddings(idx, val, embs, bs)                   # one call over the 80 concatenated rows
    assert np.max(np.abs(got - shared) / scale) >= 50 * BAR


# ---- 4. chunk boundaries --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(), (65,)], ids=str)
def test_chunk_boundaries(dims):
    bs = 5
    case = Case(24, dims, seed=31)
    fm = case.handle()
    cands = _cand_lists([0, 1, bs, bs + 1, 2 * bs + 3], len(case.items), 4)
    base, base_order = case.rank(fm, cands, bs)
    assert fm.rank_stats()["rounds"] == 1
    assert _same_bits(base, case.expect(fm, cands, bs))
    total = sum(len(c) for c in cands)
    for rows in (bs, bs + 1, 3 * bs - 1):
        capi.lib().gorse_hip_test_set_fm_rank(rows, 0)
        got, order = case.rank(fm, cands, bs)
        st = fm.rank_stats()
        assert _same_bits(got, base) and np.array_equal(order, base_order), rows
        assert st["rounds"] > 1 and st["rounds"] >= -(-total // rows), (rows, st)
    # the last user's first two slices are full (2 bs rows): no round of bs + 1 rows holds both, so that user's slices fall
    # into different rounds, and the bits are still the same
    capi.lib().gorse_hip_test_set_fm_rank(bs + 1, 0)
    got, _ = case.rank(fm, cands, bs)
    assert len(cands[-1]) >= 2 * bs > bs + 1 and fm.rank_stats()["rounds"] >= 2 and _same_bits(got, base)
    # a hook below the batch size is raised to it: a slice is never split
    capi.lib().gorse_hip_test_set_fm_rank(2, 0)
    got, _ = case.rank(fm, cands, bs)
    assert _same_bits(got, base) and fm.rank_stats()["rounds"] <= fm.rank_stats()["slices"]


# ---- 5. against the float64 restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(), (64, 5)], ids=str)
def test_against_the_float64_restatement(dims):
    case = Case(16, dims, seed=41)
    fm = case.handle()
    bs = 8
    cands = _cand_lists([3, bs, 2 * bs + 3, 0, 30], len(case.items), 9)
    got, _ = case.rank(fm, cands, bs)
    at = 0
    for t, cl in enumerate(cands):
        if not len(cl):
            continue
        idx, val = case.rows(t, cl)
        want, scale = A.predict(case.B, case.W, case.V, case.fields, idx, val, [e[cl] for e in case.embs], bs)
        g = got[at:at + len(cl)]
        err = np.max(np.abs(g - want) / scale)
        print("dims %s user %d: max err / scale %.3g" % (dims, t, err))
        assert np.all(np.abs(g - want) <= BAR * scale + 1e-30), (t, err)
        at += len(cl)


# ---- 6. order -------------------------------------------------------------------------------------------------------------
L_HOOK = 96


def test_order_with_ties_nans_and_long_lists():
    """duplicate candidates give exact ties, feature 299 (W = NaN) gives NaN scores; list lengths around a wave, around the
    device sort's cap (set to 96 here) and the trivial ones; the lists beyond the cap are the host's and are counted"""
    case = Case(8, (), n_items=40, seed=51)
    case.W = case.W.copy()
    case.W[299] = np.nan
    for c in (3, 11, 12, 30):
        a, b = case.items[c]
        case.items[c] = (np.append(a[a != 299], 299).astype(np.int32), np.append(b[a != 299], 1.0).astype(f32))
    lens = [1, 2, 63, 64, 65, L_HOOK - 1, L_HOOK, L_HOOK + 1, 0, 3 * L_HOOK]
    case.users, case.ulead = _side(len(lens), 0, 160, 52)
    fm = case.handle()
    capi.lib().gorse_hip_test_set_fm_rank(0, L_HOOK)
    cands = _cand_lists(lens, 40, 53)
    cptr, _ = K.pointer(cands)
    scores, order = case.rank(fm, cands, 64)
    assert np.isnan(scores).any() and not np.isnan(scores).all()
    assert any(np.unique(scores[cptr[t]:cptr[t + 1]]).size < lens[t] for t in range(len(lens)))  # exact ties exist
    assert _same_bits(scores, case.expect(fm, cands, 64))
    want = K.rank_orders(scores, cptr)
    assert np.array_equal(order, want)
    assert fm.rank_stats()["host_sorted"] == sum(n > L_HOOK for n in lens) == 2
    # unstable ties would show: a list that is ONE item repeated has one score and must come back in position order
    same = [np.full(n, 5, np.int32) for n in lens]
    s2, o2 = case.rank(fm, same, 64)
    assert np.array_equal(o2, np.concatenate([np.arange(n) for n in lens]))
    # either output alone
    only_s, none_o = case.rank(fm, cands, 64, order=None)
    none_s, only_o = case.rank(fm, cands, 64, scores=None)
    assert none_o is None and none_s is None
    assert _same_bits(only_s, scores) and np.array_equal(only_o, want)
    assert fm.rank_stats()["host_sorted"] == 2  # the host still sorts the long lists, from scores it fetched for itself
    # at the default cap nothing is left to the host
    capi.lib().gorse_hip_test_set_fm_rank(0, 0)
    s3, o3 = case.rank(fm, cands, 64)
    assert np.array_equal(o3, want) and fm.rank_stats()["host_sorted"] == 0


@pytest.mark.parametrize("bias", [0.0, -0.0])
def test_order_of_zero_scores(bias):
    """zero parameters and B = +-0: every score is a zero, and zeros of either sign rank by position"""
    case = Case(8, (), n_items=20, seed=61, model=(f32(bias), np.zeros(NF, f32), np.zeros((NF, 8), f32), []))
    fm = case.handle()
    cands = _cand_lists([1, 7, 65, 130, 2], 20, 3)
    scores, order = case.rank(fm, cands, 64)
    assert np.all(scores == 0) and _same_bits(scores, case.expect(fm, cands, 64))
    assert np.array_equal(order, np.concatenate([np.arange(len(c)) for c in cands]))


def test_sort_on_arbitrary_bit_patterns():
    """the ranking step alone on scores the forward pass cannot produce at will: -0 next to +0, NaNs of both signs and several
    payloads, infinities, subnormals -- device lists and host lists"""
    fm = capi.FM(8, 4)
    pool = np.array([0, 0x80000000, 0x7fc00000, 0xffc00000, 0x7f800001, 0xffffffff, 0x7f800000, 0xff800000, 1, 0x80000001,
                     0x3f800000, 0xbf800000, 0x3f800000, 0x40490fdb], u32).view(f32)
    rng = np.random.default_rng(7)
    lens = [1, 2, 63, 64, 65, 95, 96, 97, 500, 4096, 4097]
    ptr = np.zeros(len(lens) + 1, np.int64)
    ptr[1:] = np.cumsum(lens)
    scores = np.ascontiguousarray(pool[rng.integers(0, pool.size, int(ptr[-1]))])
    scores[ptr[3]:ptr[3] + 4] = np.array([0x80000000, 0, 0x80000000, 0], u32).view(f32)
    want = K.rank_orders(scores, ptr)
    for cap in (0, 96):
        capi.lib().gorse_hip_test_set_fm_rank(0, cap)
        order = np.full(scores.size, -1, np.int32)
        capi.check(capi.lib().gorse_hip_test_fm_rank_sort(fm.h, len(lens), capi._p(ptr, capi._i64p), capi._p(scores, capi._f32p),
                                                          capi._p(order, capi._i32p)))
        assert np.array_equal(order, want), cap


# ---- 7. nothing else moves ------------------------------------------------------------------------------------------------
def test_nothing_else_moves():
    dims, d, n, bs = (5, 9), 21, 70, 32
    case = Case(d, dims, seed=71, sd=0.2)
    rng = np.random.default_rng(72)
    rows = [(rng.choice(150, int(rng.integers(1, 7)), replace=False).astype(np.int32), rng.normal(1, 0.5, 6).astype(f32))
            for _ in range(n)]
    idx, val = R.pad([(a, b[:len(a)]) for a, b in rows], 6)
    tgt = np.where(rng.random(n) < 0.5, 1, -1).astype(f32)
    temb = _embs(n, dims, 73)
    fm, twin = case.handle(), case.handle(items=False)  # the twin never sees a catalogue
    for h in (fm, twin):
        h.set_train(idx, val, tgt)
        for k, e in enumerate(temb):
            h.set_train_embeddings(k, e)
    before = fm.predict_embeddings(idx, val, temb, bs)
    cands = _cand_lists([0, 1, 9, 40], len(case.items), 5)
    case.users, case.ulead = case.users[:4], case.ulead[:4]
    first, first_order = case.rank(fm, cands, 16)
    for a, b in zip(fm.get_params(), (case.B, case.W, case.V)):
        assert _same_bits(a, b)
    for k in range(len(dims)):
        for a, b in zip(fm.get_embedding_params(k), case.fields[k]):
            assert _same_bits(a, b)
    assert _same_bits(fm.predict_embeddings(idx, val, temb, bs), before)
    # one Adam epoch with a partial last batch: the handle that ranked equals the one that never did, in every bit
    c1, c2 = fm.epoch(bs, capi.OPT_ADAM, 0.01, 0.01), twin.epoch(bs, capi.OPT_ADAM, 0.01, 0.01)
    assert f32(c1).view(u32) == f32(c2).view(u32)
    for a, b in zip(fm.get_params(), twin.get_params()):
        assert _same_bits(a, b)
    for k in range(len(dims)):
        for a, b in zip(fm.get_embedding_params(k), twin.get_embedding_params(k)):
            assert _same_bits(a, b)
    # the catalogue survived the epoch; the parameters moved, so the scores follow them
    after, _ = case.rank(fm, cands, 16)
    assert not _same_bits(after, first) and _same_bits(after, case.expect(fm, cands, 16))
    # other contents change the ranking accordingly
    other = Case(d, dims, seed=74)
    case.items, case.ilead, case.embs = other.items, other.ilead, other.embs
    case.set_items(fm)
    moved, moved_order = case.rank(fm, cands, 16)
    assert _same_bits(moved, case.expect(fm, cands, 16)) and not _same_bits(moved, after)
    assert np.array_equal(moved_order, K.rank_orders(moved, K.pointer(cands)[0]))
    # set_embedding_dims drops the catalogue
    fm.set_embedding_dims(dims)
    with pytest.raises(capi.GorseHipError) as e:
        case.rank(fm, cands, 16)
    assert e.value.code == capi.ERR_INVALID


# ---- 8. errors ------------------------------------------------------------------------------------------------------------
def test_errors_leave_outputs_and_catalogue_alone():
    case = Case(16, (6,), n_items=20, seed=81)
    fm = case.handle(items=False)
    cands = _cand_lists([0, 4, 9, 1, 3], 20, 8)
    uptr, uidx, uval = K.csr(case.users)
    cptr, flat = K.pointer(cands)
    total = int(cptr[-1])

    def call(code, uptr=uptr, uidx=uidx, uval=uval, ulead=case.ulead, cptr=cptr, flat=flat, bs=4, cancel=None):
        s, o = np.full(total, 7.5, f32), np.full(total, -9, np.int32)
        with pytest.raises(capi.GorseHipError) as e:
            fm.rank_users(uptr, uidx, uval, cptr, flat, bs, user_lead=ulead, cancel=cancel, scores=s, order=o)
        assert e.value.code == code, e.value
        if code != capi.ERR_CANCELLED:  # on cancel the outputs are unspecified
            assert np.all(s == f32(7.5)) and np.all(o == -9)
        if resident:  # the catalogue that was resident before the refusal still answers, with the same bits
            s2, o2 = case.rank(fm, cands, 4)
            assert _same_bits(s2, resident[0]) and np.array_equal(o2, resident[1])

    resident = []
    call(capi.ERR_INVALID)  # no catalogue yet
    case.set_items(fm)
    good, good_order = case.rank(fm, cands, 4)
    assert _same_bits(good, case.expect(fm, cands, 4))
    resident[:] = [good, good_order]

    def still_answers():
        s, o = case.rank(fm, cands, 4)
        assert _same_bits(s, good) and np.array_equal(o, good_order)

    # rank_users
    call(capi.ERR_INVALID, bs=0)
    call(capi.ERR_INVALID, bs=-3)
    bad = flat.copy(); bad[5] = 20
    call(capi.ERR_RANGE, flat=bad)
    bad = flat.copy(); bad[0] = -1
    call(capi.ERR_RANGE, flat=bad)
    bad = uidx.copy(); bad[-1] = NF
    call(capi.ERR_RANGE, uidx=bad)
    bad = uidx.copy(); bad[0] = -2
    call(capi.ERR_RANGE, uidx=bad)
    bad = case.ulead.copy(); bad[2] = uptr[3] - uptr[2] + 1
    call(capi.ERR_INVALID, ulead=bad)
    bad = case.ulead.copy(); bad[1] = -1
    call(capi.ERR_INVALID, ulead=bad)
    bad = cptr.copy(); bad[2] = bad[1] - 1
    call(capi.ERR_INVALID, cptr=bad)
    bad = uptr.copy(); bad[1], bad[2] = bad[2], bad[1] - 1
    call(capi.ERR_INVALID, uptr=bad)
    call(capi.ERR_CANCELLED, cancel=np.ones(1, np.int32))
    still_answers()

    # set_items: every refusal leaves the resident catalogue answering
    iptr, iidx, ival = K.csr(case.items)

    def refuse(code, iptr=iptr, iidx=iidx, ival=ival, lead=case.ilead, embs=case.embs):
        with pytest.raises(capi.GorseHipError) as e:
            fm.set_items(iptr, iidx, ival, lead=lead, embs=embs)
        assert e.value.code == code, e.value
        still_answers()

    bad = iidx.copy(); bad[3] = NF
    refuse(capi.ERR_RANGE, iidx=bad)
    bad = iidx.copy(); bad[0] = -1
    refuse(capi.ERR_RANGE, iidx=bad)
    bad = iptr.copy(); bad[4] = bad[3] - 1
    refuse(capi.ERR_INVALID, iptr=bad)
    bad = case.ilead.copy(); bad[6] = iptr[7] - iptr[6] + 1
    refuse(capi.ERR_INVALID, lead=bad)
    # a catalogue that cannot fit: eight million empty items with eight 4096-wide bf16 tables are 524 GB, more than the device's
    # 288 GB of memory; the refusal comes before any table is read, so a token buffer stands in for each
    big = capi.FM(NF, 4, embedding_dims=(4096,) * 8)
    n_big = 8_000_000
    zeros = np.zeros(n_big + 1, np.int64)
    tiny = np.zeros(4096, np.uint16)
    u16p = capi.C.POINTER(capi.C.c_uint16)
    ptrs = (u16p * 8)(*[capi._p(tiny, u16p) for _ in range(8)])
    rc = capi.lib().gorse_fm_set_items(big.h, n_big, capi._p(zeros, capi._i64p), None, None, None, ptrs)
    assert rc == capi.ERR_NOMEM
    # n_items = 0 drops the catalogue
    fm.set_items(np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, f32))
    resident.clear()
    call(capi.ERR_INVALID)


# ---- 9. host twin ---------------------------------------------------------------------------------------------------------
def test_host_twin_ranks_label_rows():
    """ctr.FM.SetItems / RankUsers on label rows (ids and labels the index may not know) against the capi call on rows this
    test encodes itself the way BatchPredict does: the id entry when known, then the known labels; unknown ids give lead 0"""
    from gorse_amd import ctr
    nf, d, dims, n, bs = 120, 8, (6,), 64, 16
    rng = np.random.default_rng(91)
    rows = [(rng.choice(nf, int(rng.integers(1, 6)), replace=False).astype(np.int32), rng.normal(1, 0.5, 5).astype(f32))
            for _ in range(n)]
    ptr, idx, val = K.csr([(a, b[:len(a)]) for a, b in rows])
    tgt = np.where(rng.random(n) < 0.5, 1, -1).astype(f32)
    train = ctr.Dataset(nf, rows=(ptr, idx, val, tgt))
    train.set_embeddings(_embs(n, dims, 92))
    m = ctr.FM(nFactors=d, nEpochs=2, batchSize=bs, lr=0.01, reg=0.0, optimizer=ctr.Adam, seed=3)
    m.Fit(train, train, Verbose=1)

    def side(count, id0, label0, seed):
        r = np.random.default_rng(seed)
        ids = np.array([-1 if i % 4 == 1 else id0 + i for i in range(count)], np.int32)  # every fourth is unknown to the index
        labels = [[(-1 if r.random() < 0.25 else int(label0 + r.integers(0, 20)), f32(r.normal(0.5, 1.0)))
                   for _ in range(int(r.integers(0, 4)))] for _ in range(count)]
        return ids, labels

    def encode(ids, labels):
        rows = [(np.array(([i] if i >= 0 else []) + [l for l, _ in ls if l >= 0], np.int32),
                 np.array(([1.0] if i >= 0 else []) + [v for l, v in ls if l >= 0], f32)) for i, ls in zip(ids, labels)]
        return rows, (ids >= 0).astype(np.int32)

    n_items, n_users = 30, 5
    iids, ilabels = side(n_items, 40, 100, 93)
    uids, ulabels = side(n_users, 0, 80, 94)
    E = _embs(n_items, dims, 95)
    cands = _cand_lists([0, 1, bs, bs + 1, 2 * bs + 3], n_items, 96)
    m.SetItems(iids, ilabels, embs=E)
    got = m.RankUsers(uids, ulabels, cands)

    fm = capi.FM(nf, d, embedding_dims=dims)
    fm.set_params(*m.params())
    fm.set_embedding_params(0, *m.field_params(0))
    irows, ilead = encode(iids, ilabels)
    urows, ulead = encode(uids, ulabels)
    assert ulead[1] == 0 and ilead[1] == 0 and ulead[0] == 1 and ilead[0] == 1
    fm.set_items(*K.csr(irows), lead=ilead, embs=E)
    cptr, flat = K.pointer(cands)
    scores, order = fm.rank_users(*K.csr(urows), cptr, flat, bs, user_lead=ulead)
    # the capi call itself, on these leads, is the materialised rows' score
    case = Case(d, dims, n_items=n_items, n_users=n_users, seed=1)
    case.users, case.ulead, case.items, case.ilead, case.embs = urows, ulead, irows, ilead, E
    assert _same_bits(scores, case.expect(fm, cands, bs))
    for t, cl in enumerate(cands):
        c0 = int(cptr[t])
        want = [(int(cl[p]), scores[c0 + p]) for p in order[c0:c0 + len(cl)]]
        assert [i for i, _ in got[t]] == [i for i, _ in want], t
        assert _same_bits([s for _, s in got[t]], [s for _, s in want]), t
