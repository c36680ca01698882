"""The host mirror of the neighbourhood recommenders on hip:// (gorse_amd/host/gorse_vectors.hpp): ItemToItemRecommendBulk and
UserToUserRecommendBulk -- one bulk search for the lists, one gorse_nbr_recommend for all users -- equal the per-user calls list for
list and bit for bit, for the embedding, tags and auto kinds; and the reference's known answers through both."""
import pytest

import nbr_host_suite as S
from gorse_amd import vectors as V

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def db():
    return V.Open("hip://")


@pytest.mark.parametrize("kind", ["embedding", "tags", "auto"])
def test_bulk_equals_per_user(db, kind):
    coll, ids, positives, excludes, feedback = S.world(db, kind, 21)
    for n, categories in ((10, None), (3, ["b"])):
        bulk = V.ItemToItemRecommendBulk(db, coll, kind, positives, excludes, categories, n)
        assert len(bulk) == len(positives) and any(len(b) == n for b in bulk) and any(len(b) == 0 for b in bulk)
        for t, b in enumerate(bulk):
            S.same(b, V.ItemToItemRecommend(db, coll, kind, positives[t], excludes[t], categories, n), ("item-to-item", kind, n, t))
            assert not set(s.Id for s in b) & set(excludes[t])
    users = ids[:len(excludes)]
    for n in (10, 40):
        bulk = V.UserToUserRecommendBulk(db, coll, kind, users + ["no-such-user"], excludes + [[]], feedback, n)
        assert len(bulk) == len(users) + 1 and bulk[-1] == [] and any(len(b) == n for b in bulk)
        for t, u in enumerate(users):
            S.same(bulk[t], V.UserToUserRecommend(db, coll, kind, u, excludes[t], feedback, n), ("user-to-user", kind, n, t))
            assert not set(s.Id for s in bulk[t]) & set(excludes[t])
    # the per-user call is the restatement (tests/nbr_ref.py) on this device's neighbour lists, too
    for t in (1, 2, 3):
        S.same(V.ItemToItemRecommend(db, coll, kind, positives[t], excludes[t], None, 10),
               S.ref_item_to_item(db, coll, kind, positives[t], excludes[t], None, 10), ("ref", kind, t))
        S.same(V.UserToUserRecommend(db, coll, kind, users[t], excludes[t], feedback, 10),
               S.ref_user_to_user(db, coll, kind, users[t], excludes[t], feedback, 10), ("ref", kind, t))


@pytest.mark.parametrize("case", S.kats(), ids=lambda c: c["name"])
def test_reference_known_answers(db, case):
    per_user, bulk = S.run_kat(db, case, False), S.run_kat(db, case, True)
    S.check_kat(case, per_user)
    S.check_kat(case, bulk)
    S.same(bulk, per_user)


def test_cache_size_beyond_the_device_call_is_refused(db):
    coll, ids, positives, excludes, feedback = S.world(db, "embedding", 22, n=40, n_users=4)
    with pytest.raises(ValueError):
        V.ItemToItemRecommendBulk(db, coll, "embedding", positives, excludes, None, 257)
