"""gorse_fm_rank_users and gorse_fm_evaluate score through one path (fm_resident.hip) and work in one round scratch of the
handle.  Nothing of one call may reach the other through it: on a handle that holds a catalogue and a test split, rank, evaluate,
rank, evaluate each return, in every bit, what a fresh handle with the same parameters returns for that call alone."""
import numpy as np
import pytest

import fm_attention_ref as A
from gorse_amd import capi

pytestmark = pytest.mark.gpu
f32, u32 = np.float32, np.uint32
D_FACTORS, DIMS, BS, ROUND = 24, (65,), 7, 14


@pytest.fixture(autouse=True)
def _hooks():
    capi.lib().gorse_hip_test_set_fm_rank(ROUND, 0)
    capi.lib().gorse_hip_test_set_fm_evaluate(ROUND, 0)
    yield
    capi.lib().gorse_hip_test_set_fm_rank(0, 0)
    capi.lib().gorse_hip_test_set_fm_evaluate(0, 0)


def _csr(idx, val):
    keep = val != 0
    return np.concatenate([[0], np.cumsum(keep.sum(1))]).astype(np.int64), idx[keep], val[keep]


def _bits(x):
    return np.ascontiguousarray(x, f32).view(u32)


def test_the_shared_scratch_carries_nothing_between_rank_and_evaluate():
    B, W, V, fields = A.model(D_FACTORS, DIMS, 71)
    i_idx, i_val, _, i_emb = A.rows(12, DIMS, 72)  # the catalogue: 12 items
    u_idx, u_val, _, _ = A.rows(3, DIMS, 73)       # 3 users with 10, 0 and 9 candidates
    rng = np.random.default_rng(74)
    cptr = np.array([0, 10, 10, 19], np.int64)
    cand = rng.integers(0, 12, 19).astype(np.int32)
    t_idx, t_val, t_tgt, t_emb = A.rows(40, DIMS, 75)  # the test split: 40 rows
    n_pos = int((t_tgt > 0).sum())
    assert 12 <= n_pos <= 28 and n_pos % BS != 0  # about half, and the positives' last slice is partial

    def handle():
        fm = capi.FM(A.NF, D_FACTORS, embedding_dims=DIMS)
        fm.set_params(B, W, V)
        fm.set_embedding_params(0, *fields[0])
        fm.set_items(*_csr(i_idx, i_val), embs=i_emb)
        fm.set_test(t_idx, t_val, t_tgt, t_emb)
        return fm

    def rank(fm):
        scores, order = fm.rank_users(*_csr(u_idx, u_val), cptr, cand, BS)
        st = fm.rank_stats()
        assert (st["rows"], st["slices"]) == (19, 4) and st["rounds"] > 1
        return _bits(scores), order

    def evaluate(fm):
        counts, auc_sum, logits = fm.evaluate(BS, logits=True)
        st = fm.evaluate_stats()
        assert st["rows"] == 40 and st["slices"] == -(-n_pos // BS) + -(-(40 - n_pos) // BS) and st["rounds"] > 1
        return counts, _bits(auc_sum), _bits(logits)

    alone = []
    for call in (rank, evaluate):
        fm = handle()
        alone.append(call(fm))
        fm.close()
    assert not np.isnan(alone[0][0].view(f32)).any() and alone[1][0]["nan"] == 0
    fm = handle()
    for step, (call, want) in enumerate(zip((rank, evaluate, rank, evaluate), alone * 2)):
        got = call(fm)
        for g, w in zip(got, want):
            assert g == w if isinstance(w, dict) else np.array_equal(g, w), (step, g, w)
    fm.close()
