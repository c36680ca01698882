"""Who owns which element in the sole-writer fold of the BPR user-run launches (gorse_amd/csrc/hot_rows.hpp fold_share, reached through
the host library's hook gh_test_bpr_fold_owner; csrc/bpr_fold.hpp run_folders takes a thread's share from that function once per launch and
walks it in every periodic pass and in the last one).  Such a launch folds with loads and stores, so the atomics' place is taken by
one invariant: every element of every slot has exactly one owner thread.  Checked for tiers of one slot, for the C2 shape (926 hot
slots, 2,780 of the accumulated tier) and a smaller one, at every user-run width, with 64 folder workgroups (32 per tier: what a
handle with the tier launches) and with 32 (no workgroups behind the hot tier's: they own every slot):
  * every element is claimed exactly once;
  * a tier's slots are owned by its own workgroups only -- the last pass, which each workgroup begins when it decides to, shares no
    row out differently than the periodic passes did;
  * an owner's elements come in aligned groups of the 8 or 16 bytes one access of the kernel moves;
  * the work is spread: no thread owns more than one group above the tier's mean.
That the kernel's last pass indeed walks the share its periodic passes walk is what tests/test_gpu_bpr_fold_sole_writer.py shows on
the device (exact counts after many passes)."""
import ctypes as C

import numpy as np
import pytest

from gorse_amd import cf

HOT_BLOCKS, THREADS = 32, 256  # csrc/bpr_plan.hpp kFolderBlocks, the update kernels' workgroup


def owners(n_hot, n_acc, d, folders):
    L = C.CDLL(cf.HOST_LIB)
    L.gh_test_bpr_fold_owner.restype = C.c_int32
    L.gh_test_bpr_fold_owner.argtypes = [C.c_int32] * 5 + [C.c_void_p, C.c_void_p]
    n = (n_hot + n_acc) * d
    owner, claims = np.full(n, -7, np.int32), np.full(n, -7, np.int32)
    group = L.gh_test_bpr_fold_owner(n_hot, n_acc, d, folders, HOT_BLOCKS, owner.ctypes.data, claims.ctypes.data)
    return group, owner.reshape(n_hot + n_acc, d), claims.reshape(n_hot + n_acc, d)


@pytest.mark.parametrize("folders", [32, 64])
@pytest.mark.parametrize("d", [8, 16, 32, 64, 128])
@pytest.mark.parametrize("n_hot,n_acc", [(1, 0), (0, 1), (1, 1), (926, 2780), (128, 384)])
def test_every_element_has_one_owner_of_its_own_tier(n_hot, n_acc, d, folders):
    group, owner, claims = owners(n_hot, n_acc, d, folders)
    assert group * 4 in (8, 16) and d % group == 0
    assert (claims == 1).all(), "elements claimed %s times" % np.unique(claims)
    assert (owner >= 0).all() and (owner < folders * THREADS).all()
    block = owner // THREADS
    if folders > HOT_BLOCKS:  # two tiers, each among its own workgroups
        assert (block[:n_hot] < HOT_BLOCKS).all() and (block[n_hot:] >= HOT_BLOCKS).all()
    # aligned groups: the elements of a group share their owner, and neighbouring groups of a slot do not (more threads than a slot has groups)
    g = owner.reshape(n_hot + n_acc, d // group, group)
    assert (g == g[:, :, :1]).all()
    assert d // group < 2 or (g[:, 1:, 0] != g[:, :-1, 0]).all()
    # spread: groups per thread within one of the tier's mean
    for lo, hi, blocks in ((0, n_hot, HOT_BLOCKS), (n_hot, n_hot + n_acc, folders - HOT_BLOCKS)) if folders > HOT_BLOCKS else \
            ((0, n_hot + n_acc, folders),):
        if hi > lo:
            per = np.bincount(owner[lo:hi, ::group].ravel(), minlength=folders * THREADS)
            assert per.max() <= -(-(hi - lo) * (d // group) // (blocks * THREADS))
