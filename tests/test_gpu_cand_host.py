"""logics::RecommendSequentialBulk (gorse_amd/host/gorse_vectors.hpp): the bulk twin of RecommendSequential over one candidate chain,
against the per-user host loop on string ids -- lists equal, scores in every bit --, against tests/cand_ref.py, and on the
reference's own known answers for the single list recommenders (tests/golden/recommend_sequential_kats.json)."""
import pytest

import cand_host_suite as H
from gorse_amd import vectors as V

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def db():
    return V.Open("hip://")


@pytest.mark.parametrize("seed", [3, 4])
def test_bulk_equals_per_user(db, seed):
    users, positives, excludes, stages = H.world(db, seed)
    want = H.per_user(db, users, positives, excludes, stages)
    got = V.RecommendSequentialBulk(db, users, positives, excludes, stages)
    H.same_lists(got, want, "bulk against the per-user loop")
    H.same_lists(got, H.restatement(db, users, positives, excludes, stages), "bulk against cand_ref")
    assert sum(map(len, got)) > 10 * len(users)
    # the stages in another order give other lists: the exclude set grows from stage to stage
    swapped = [stages[3], stages[1], stages[2], stages[0]]
    got2 = V.RecommendSequentialBulk(db, users, positives, excludes, swapped)
    H.same_lists(got2, H.per_user(db, users, positives, excludes, swapped), "swapped stages")
    assert [[s.Id for s in g] for g in got2] != [[s.Id for s in g] for g in got]


@pytest.mark.parametrize("case", H.kats(), ids=lambda c: c["name"])
def test_reference_known_answers(db, case):
    for query in case["queries"]:
        stage = H.kat_stage(case, query)
        H.check_kat(query, V.RecommendSequentialBulk(db, ["user_1"], [[]], [case["exclude"]], [stage])[0])
        H.check_kat(query, V.RecommendSequential(db, "user_1", [], case["exclude"], [stage]))


def test_no_users_and_no_stages(db):
    assert V.RecommendSequentialBulk(db, [], [], [], []) == []
    assert V.RecommendSequentialBulk(db, ["u"], [[]], [["x"]], []) == [[]]
    with pytest.raises(ValueError, match="CacheSize"):  # the chain's k per stage
        V.RecommendSequentialBulk(db, ["u"], [[]], [[]], [V.SeqStage("shared", 257, lists=[V.Score("a", 1.0, [])])])
