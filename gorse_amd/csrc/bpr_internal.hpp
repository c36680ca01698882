// bpr_internal.hpp -- what the units of the BPR step share: the test state, the two device helpers both update kernels call, the
// HotRows of a launch as the host fills it, and the host entry points that cross units.  One unit per stage:
//   bpr_prepare.hip       the samplers, the counting sort by user with its scan, the binned chunk preparation and the grouping pass
//   bpr_update.hip        the per-sample update kernel (bpr_update_kernel) and its fold kernel
//   bpr_update_users.hip  the user-run update kernel (bpr_update_user_kernel)
//   bpr.hip               the epoch driver, the sequential schedule, the schedule choice and every extern "C" entry
// bpr_fold.hpp is the device header of the folds, which both update units include.  The rules the host decides by live in
// bpr_plan.hpp, which has no HIP in it.
#pragma once
#include "bpr_fold.hpp"

namespace gorse {
static_assert(kRunsPerBlock == kGroupsPerBlock && kFoldThreads == kBlock && kFlatThreads == 256, "bpr_plan.hpp states the update workgroup's geometry");

// which item updates may take the store route (gorse_hip_test_set_bpr_store_mode)
// Cold negatives by store: measured at C3 whole (profiles/r04_b_probe_bpr_stores_*.txt): update kernel 89 -> 60 ms per epoch, 4 % of the updates of cold rows
// overwritten, NDCG@10 0.6100 against 0.6096 with atomics only (sequential oracle 0.6126); the positive side stays atomic -- by store
// it costs 0.003-0.005 of NDCG for 6 % more speed
constexpr int kDefaultStoreMode = 1;

// The switches of the tests and probes (defined in bpr.hip next to their setters); nothing of it reaches a kernel other than as a
// launch argument (HotRows, exp_mode).
struct BprTestState {
    int variant = 0;                                // GORSE_TEST_BPR_* switches of the tests (gorse_hip_test_set_variant)
    int store_mode = kDefaultStoreMode;             // 1 = NEG_STORE of bpr_update_user_kernel where the handle has cold items, 0 = atomics only
    uint32_t fold_period = kDefaultFoldPeriod;      // gorse_hip_test_set_bpr_fold_period
    int acc_fold_every = kDefaultAccFoldEvery;      // gorse_hip_test_set_bpr_acc_fold_every
    uint64_t folder_timeout = kFolderTimeout;       // gorse_hip_test_set_bpr_folder_timeout
    int64_t chunk_override = 0;                     // probe: gorse_hip_test_set_bpr_chunk
    int exp_mode_exact = 0;                         // exp flavour of the sequential schedule; tests flip it to 1 for bit parity
    int user_runs = 1;                              // the compiled default of the Hogwild schedule: 1 = user runs, 0 = per-sample groups
};
extern BprTestState g_bpr;

// ---- memory access flavours ------------------------------------------------------------------
template <int MODE>
__device__ __forceinline__ float load_row(const float *p) {
    if (MODE == MODE_EXACT)
        return *p;
    else  // agent-scope load: served by L2 (never stale for written-back data), bypasses the CU's L1
        return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ float bpr_exp(float x, int exp_mode) {
    return exp_mode == 1 ? exp_restated(x) : (exp_mode == 2 ? __expf(x) : expf(x));
}

// the replica rows of a slot lie next to each other (r04_a: 4 KB apart or n_hot rows apart makes no difference); n_hot stays 0 (no
// replicas, no folders) until the launch opens them: open_hot
inline HotRows make_hot(const gorse_mf *h) {
    return HotRows{h->hot_slot.p, h->hot_items.p, h->hot_meta.p, h->hot_rep.p, h->hot_done.p, 0, h->d, 0, g_bpr.fold_period, 0, g_bpr.acc_fold_every,
                   h->hot_base.p, 0, g_bpr.folder_timeout};
}
inline bool has_hot(const gorse_mf *h) { return h->n_hot > 0 || h->n_acc > 0; }  // any row that takes an item's updates for it
// an update launch with folders: the replicas open, the launch's set of arrival stripes by launch parity (the set of the launch before
// is zeroed by this one's folders; gorse_mf_create zeroed both)
inline int open_hot(gorse_mf *h, HotRows &hot) {
    hot.n_hot = h->n_hot;
    hot.n_acc = h->n_acc;
    hot.set = (int)(h->hot_launches++ & 1);
    return bpr_folders(h->n_hot, h->n_acc);
}

// bpr_prepare.hip.  `trip`: 3 x cap ints (us | is | js); start / stop (may be null): events bound to the kernel's own dispatch
int32_t bpr_launch_sampler(gorse_mf *h, uint64_t seed, uint64_t epoch, int64_t base, int64_t n, int32_t *trip, size_t cap, hipStream_t st,
                           hipEvent_t start = nullptr, hipEvent_t stop = nullptr);
int32_t bpr_launch_prepare_users(gorse_mf *h, uint64_t seed, uint64_t epoch, int64_t base, int64_t n, int32_t *trip, int32_t *sorted,
                                 int32_t *bucket, int32_t *rank, size_t cap, hipStream_t st);
int32_t bpr_launch_user_sort(gorse_mf *h, const int32_t *trip, int32_t *sorted, int32_t *bucket, int32_t *rank, int64_t n, size_t cap,
                             hipStream_t st);
int32_t bpr_ensure_user_sort(gorse_mf *h);
int32_t bpr_ensure_trip(gorse_mf *h, int64_t want);
// bpr_update.hip: the per-sample kernel in the flavour of `mode` (MODE_ATOMIC / MODE_EXACT / MODE_RACY) over samples order[begin .. end)
int32_t bpr_launch_update(gorse_mf *h, int mode, const int32_t *us, const int32_t *is, const int32_t *js, const int32_t *order, int64_t begin,
                          int64_t end, float lr, float reg, int exp_mode, double *loss, hipStream_t st, hipEvent_t start = nullptr,
                          hipEvent_t stop = nullptr);
// bpr_update_users.hip: the user-run kernel over a chunk sorted by user; stores: the cold negatives by store (MODE_STORES)
int32_t bpr_launch_update_users(gorse_mf *h, const int32_t *sorted, const int32_t *bucket, size_t cap, float lr, float reg, int exp_mode,
                                double *loss, hipStream_t st, bool stores, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);

}  // namespace gorse
