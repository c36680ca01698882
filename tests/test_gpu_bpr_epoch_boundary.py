"""The boundary between two BPR update launches (csrc/bpr.hip epoch_impl, csrc/mf.hip mf_epoch_begin / _end, KernelProfile::events).

An update launch carries its events on its own dispatch (hipExtLaunchKernelGGL): ONE stop event is the chunk's "consumed" event (the
preparation of the chunk after next waits on it), the epoch's end event when the chunk is the epoch's last, and the end of the
profile's update span; the start event is the span's begin, or the begin of an epoch that does not follow another.  Checked here, at
the smallest shapes at which the hand-off can go wrong and with chunks of 4096 samples so that every buffer is reused many times:
  * no chunk is applied twice, skipped, or read while the next preparation overwrites it: reg = 0 and a tiny step, so every item
    row moves by the sum of the per-sample deltas of the epoch's triplets (the bound is derived in _bounds, from the data);
  * the same on the per-sample schedule, where bpr_fold_kernel follows each update kernel and carries the stop event;
  * the profile's launch counts and spans, the epochs' device times against them and against the wall clock;
  * more epochs than the epoch ring and more chunks than the chunk ring in flight, nothing read in between;
  * the synchronous entry point with a loss (a memset in front of the first launch: the epoch's begin is recorded).
"""
import time

import numpy as np
import pytest

from gorse_amd import capi

pytestmark = pytest.mark.gpu

I, PER, D = 512, 8, 16
CHUNK, N = 4096, 40960  # 10 chunks per epoch: each of the two buffers is reused five times
SEED, BASE = 11, 1 << 33
LR = 5e-7
EPOCH_RING, CHUNK_RING = 16, 4  # csrc/mf_internal.hpp kEpochRing, kChunkRing


POPULAR = 8  # U = 1000: two of a user's eight feedbacks are on items 0..7 (~250 feedbacks each: hot items, which take >= 64)


def _dataset(U):
    rng = np.random.default_rng(U)
    if U < 4096:
        rows = [np.concatenate([rng.choice(POPULAR, 2, replace=False), POPULAR + rng.choice(I - POPULAR, PER - 2, replace=False)])
                for _ in range(U)]
    else:
        rows = [rng.choice(I, PER, replace=False) for _ in range(U)]
    uidx = np.concatenate([np.sort(r) for r in rows]).astype(np.int32)
    uptr = np.arange(U + 1, dtype=np.int64) * PER
    P = rng.normal(0, 0.1, (U, D)).astype(np.float32)
    Q = rng.normal(0, 2e-5, (I, D)).astype(np.float32)
    return uptr, uidx, P, Q


def _ulp32(x):
    return float(np.spacing(np.float32(x)))


def _sample_terms(P, Q, u, i, j):
    """per-sample deltas from the initial state (reg = 0), float64: Q[i] += step, Q[j] -= step"""
    ok = u >= 0
    u, i, j = u[ok], i[ok], j[ok]
    P64, Q64 = P.astype(np.float64), Q.astype(np.float64)
    x = np.einsum("nd,nd->n", P64[u], Q64[i] - Q64[j])
    step = LR / (1.0 + np.exp(x))[:, None] * P64[u]
    return u, i, j, step


def _accumulate(P, Q, u, i, j):
    """(sum of the deltas per item row, sum of their magnitudes per row element, updates per row, samples per user)"""
    u, i, j, step = _sample_terms(P, Q, u, i, j)
    move, mass = np.zeros((I, D)), np.zeros((I, D))
    np.add.at(move, i, step)
    np.add.at(move, j, -step)
    np.add.at(mass, i, np.abs(step))
    np.add.at(mass, j, np.abs(step))
    count = np.bincount(i, minlength=I) + np.bincount(j, minlength=I)
    return move, mass, count, np.bincount(u, minlength=P.shape[0])


def _bounds(P, Q, mass, count, per_user):
    """What |moved - expected| of an element of item row r may be when every sample was applied exactly once (reg = 0):
      * drift: a sample computes from rows that have moved.  A row of Q is at most |mass_r|_2 away from where it began (all its
        updates aligned), p_u at most n_u LR 2 max|q| (n_u samples, each moving it by LR sigma (q_i - q_j)).  So x = p_u.(q_i - q_j)
        is off by eps <= 2 max|p| max_r|mass_r|_2 + max|dp| 2 max|q|; d ln sigma(-x) / dx lies in (-1, 0), so the sample's delta is
        off by a factor within e^(+-eps), and by LR max|dp| through p_u itself: (e^eps - 1) mass_r + count_r LR max|dp|;
      * fp32 arithmetic of a delta (16-term dot product, exp, a division: a few ulp each, 1e-5 relative at most): 1e-5 mass_r;
      * fp32 accumulation: every update is one add onto an accumulator no larger than A_r = max|q_r| + max mass_r (the row, a replica
        row, a series' running sum), and a replica's sum is added on once more by a fold: at most 3 count_r adds of half an ulp of A_r.
    Nothing here is taken from what the device returns."""
    dq = np.sqrt((mass * mass).sum(axis=1))
    pmax = float(np.sqrt((P.astype(np.float64) ** 2).sum(axis=1)).max())
    qmax = float(np.sqrt((Q.astype(np.float64) ** 2).sum(axis=1)).max()) + float(dq.max())
    dp = float(per_user.max()) * LR * 2.0 * qmax
    eps = 2.0 * pmax * float(dq.max()) + dp * 2.0 * qmax
    mass_el = mass.max(axis=1)
    a = np.abs(Q).max(axis=1).astype(np.float64) + mass_el
    rounding = 3.0 * count * 0.5 * np.array([_ulp32(v) for v in a])
    return (np.expm1(eps) + 1e-5) * mass_el + count * LR * dp + rounding


class _Reference:
    """the epochs' triplets (gorse_bpr_sample_triplets) and what they add up to, computed once per data set"""

    def __init__(self, U, epochs):
        self.U = U
        self.uptr, self.uidx, self.P, self.Q = _dataset(U)
        mf = capi.MF(U, I, D, self.uptr, self.uidx)
        self.trip = [mf.bpr_sample_triplets(N, SEED, ep, BASE) for ep in range(1, epochs + 1)]
        mf.close()
        self.parts = [_accumulate(self.P, self.Q, *t) for t in self.trip]

    def upto(self, k):
        move, mass, count, per_user = (sum(p[x] for p in self.parts[:k]) for x in range(4))
        return move, _bounds(self.P, self.Q, mass, count, per_user)

    def without_chunk(self, k, epoch, chunk):
        """the sum over k epochs with one chunk of one epoch left out: what a skipped chunk would leave behind"""
        u, i, j = (a[chunk * CHUNK:(chunk + 1) * CHUNK] for a in self.trip[epoch - 1])
        return self.upto(k)[0] - _accumulate(self.P, self.Q, u, i, j)[0]


_refs = {}


def _reference(U, epochs=3):
    if (U, epochs) not in _refs:
        _refs[(U, epochs)] = _Reference(U, epochs)
    return _refs[(U, epochs)]


def _worst_ratio(moved, expect, bound):
    return float((np.abs(moved - expect).max(axis=1) / bound).max())


def _train(ref, epochs, mode, profiling, user_runs, after=None):
    L = capi.lib()
    L.gorse_hip_test_set_bpr_chunk(CHUNK)
    mf = None
    try:
        mf = capi.MF(ref.U, I, D, ref.uptr, ref.uidx)
        assert mf.bpr_user_runs() == user_runs
        mf.set_factors(ref.P, ref.Q)
        mf.epoch_times(reset=True)
        if profiling:
            mf.set_profiling(True)
            mf.reset_profile()
        t0 = time.perf_counter()
        for ep in range(1, epochs + 1):
            mf.bpr_epoch_enqueue(N, LR, 0.0, SEED, ep, BASE, mode=mode)
        mf.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        out = after(mf, wall) if after else None
        gP, gQ = mf.get_factors()
        return gQ.astype(np.float64) - ref.Q.astype(np.float64), out
    finally:
        L.gorse_hip_test_set_bpr_chunk(0)
        if mf is not None:
            mf.close()


def _check_moves(ref, moved, epochs, label):
    expect, bound = ref.upto(epochs)
    worst = _worst_ratio(moved, expect, bound)
    rel = float((np.abs(moved - expect).max(axis=1) / np.abs(expect).max(axis=1)).max())
    # the check has teeth: one chunk of 10 x epochs left out lies far outside the bound (no device result enters here)
    skipped = _worst_ratio(ref.without_chunk(epochs, min(2, epochs), 3), expect, bound)
    print("%s: worst |moved - expected| / bound = %.3f (%.2e of the row's largest expected move); one skipped chunk would give %.1f"
          % (label, worst, rel, skipped))
    assert skipped > 3.0
    assert worst < 1.0, (label, worst)


@pytest.mark.parametrize("mode,profiling", [(capi.BPR_HOGWILD_ATOMIC, False), (capi.BPR_HOGWILD_STORES, False),
                                            (capi.BPR_HOGWILD_ATOMIC, True), (capi.BPR_HOGWILD_STORES, True)])
def test_chunk_hand_off_under_small_chunks(mode, profiling):
    """U = 4096 (the smallest handle of the user-run schedule), three epochs of ten chunks enqueued back to back, one synchronisation."""
    ref = _reference(4096)
    moved, _ = _train(ref, 3, mode, profiling, True)
    _check_moves(ref, moved, 3, "user runs, mode %d, profiling %s" % (mode, profiling))


@pytest.mark.parametrize("mode,profiling", [(capi.BPR_HOGWILD_ATOMIC, False), (capi.BPR_HOGWILD_STORES, False),
                                            (capi.BPR_HOGWILD_ATOMIC, True), (capi.BPR_HOGWILD_STORES, True)])
def test_chunk_hand_off_on_the_per_sample_schedule(mode, profiling):
    """U = 1000 is below the user-run gate; the handle has hot items, so bpr_fold_kernel follows each update kernel and the chunk's
    stop event is the fold kernel's."""
    ref = _reference(1000)
    stats = np.zeros(3, np.int64)

    def after(mf, wall):
        capi.check(capi.lib().gorse_hip_test_bpr_fold_stats(mf.h, stats.ctypes.data))

    moved, _ = _train(ref, 3, mode, profiling, False, after)
    assert stats[1] > 0, "the handle has no hot items: no fold kernel ran"
    _check_moves(ref, moved, 3, "per sample, mode %d, profiling %s, %d hot items" % (mode, profiling, stats[1]))


@pytest.mark.parametrize("U,user_runs", [(4096, True), (1000, False)])
def test_spans_and_counts(U, user_runs):
    """K epochs of C chunks with profiling on: K C update spans, the preparation's spans as the schedule issues them (user runs at
    this shape: bin count + bin finish = 2 sample spans and 1 sort span per chunk; per sample: 1 sampler span, no sort), every epoch
    timed, and sum of the update spans <= the epochs' device time <= 1.05 x wall."""
    K, C = 3, N // CHUNK
    ref = _reference(U)

    def after(mf, wall):
        n, ms, flying = mf.epoch_times()
        return (n, ms, flying, wall, mf.get_profile(capi.PROF_BPR_UPDATE), mf.get_profile(capi.PROF_BPR_SAMPLE),
                mf.get_profile(capi.PROF_BPR_SORT))

    _, (n, ms, flying, wall, upd, smp, srt) = _train(ref, K, capi.BPR_HOGWILD_STORES, True, user_runs, after)
    print("U %d: %d epochs, device %.3f ms, wall %.3f ms; update %s, sample %s, sort %s" % (U, n, ms, wall, upd, smp, srt))
    assert upd[0] == K * C and upd[1] > 0
    assert smp[0] == (2 if user_runs else 1) * K * C and smp[1] > 0
    assert srt[0] == (K * C if user_runs else 0)
    assert n == K and flying == 0
    assert upd[1] <= ms <= 1.05 * wall


def test_event_rings():
    """More epochs than the epoch ring (each of more chunks than the chunk ring) enqueued without a harvest in between: every epoch is
    counted once, as timed or -- when its slot was due for reuse before it had finished -- not at all (at most the ring's size minus
    one wait unread at any time, so at least that many are timed), nothing stays in flight, and every chunk was applied once."""
    K = EPOCH_RING + 4
    assert N // CHUNK > CHUNK_RING
    ref = _reference(4096, K)

    def after(mf, wall):
        return mf.epoch_times()

    for profiling in (False, True):
        moved, (n, ms, flying) = _train(ref, K, capi.BPR_HOGWILD_STORES, profiling, True, after)
        print("profiling %s: %d epochs enqueued, %d timed (%.3f ms), %d in flight" % (profiling, K, n, ms, flying))
        assert flying == 0 and EPOCH_RING - 1 <= n <= K and ms > 0
        _check_moves(ref, moved, K, "%d epochs in flight, profiling %s" % (K, profiling))


def test_synchronous_epoch_with_a_loss():
    """gorse_bpr_epoch with loss_out: the memset of the loss precedes the first launch on the update stream, so the epoch's begin is
    a recorded event; its device time is positive and covers the update spans."""
    ref = _reference(4096)
    L = capi.lib()
    L.gorse_hip_test_set_bpr_chunk(CHUNK)
    mf = capi.MF(ref.U, I, D, ref.uptr, ref.uidx)
    try:
        mf.set_factors(ref.P, ref.Q)
        mf.bpr_epoch(N, LR, 0.0, SEED, 1, BASE)  # buffers, code objects
        mf.set_factors(ref.P, ref.Q)
        mf.epoch_times(reset=True)
        mf.set_profiling(True)
        mf.reset_profile()
        loss = mf.bpr_epoch(N, LR, 0.0, SEED, 1, BASE, want_loss=True)
        n, ms, flying = mf.epoch_times()
        launches, upd_ms = mf.get_profile(capi.PROF_BPR_UPDATE)
        mf.set_profiling(False)
        print("synchronous epoch with a loss: device %.3f ms, %d update spans %.3f ms, loss %r" % (ms, launches, upd_ms, loss))
        assert n == 1 and flying == 0 and launches == N // CHUNK
        assert ms > 0 and ms >= 0.95 * upd_ms
        moved = mf.get_factors()[1].astype(np.float64) - ref.Q.astype(np.float64)
        _check_moves(ref, moved, 1, "synchronous epoch")
    finally:
        L.gorse_hip_test_set_bpr_chunk(0)
        mf.close()
