// bpr_plan.hpp -- the host rules of the BPR step (bpr.hip and the units it drives: bpr_prepare.hip, bpr_update.hip,
// bpr_update_users.hip), each written once: which schedule a handle takes and which kernel mode its update launch receives, the
// capacity of a chunk, the route a chunk's preparation takes, and the grids, folder counts, flags and LDS of the launches.  The
// launch code calls these functions and holds no copy of their arithmetic; a constant that a kernel reads too (kFolderBlocks,
// kFolderBlocksAcc, kScanTile, kFinCap, kFinStage, kFinShift) has its one definition here.  A rule that a test switch
// (GORSE_TEST_BPR_*, include/gorse_hip_test.h) or an A/B macro overrides takes the bits or the macro's value as an argument.
// No HIP in here: tests/cpp/bpr_plan_main.cpp checks every rule by value under AddressSanitizer and UBSan without a device.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/gorse_hip_test.h"
#include "bpr_bins.hpp"
#include "hot_rows.hpp"

namespace gorse {

constexpr int MODE_ATOMIC = GORSE_BPR_HOGWILD_ATOMIC;
constexpr int MODE_EXACT = GORSE_BPR_SEQUENTIAL;
constexpr int MODE_RACY = GORSE_BPR_HOGWILD_RACY;
constexpr int MODE_STORES = GORSE_BPR_HOGWILD_STORES;  // MODE_ATOMIC with the cold negatives by store (user-run schedule only)

// ---- the schedule ---------------------------------------------------------------------------------------------------------------
// Hogwild schedule: user runs (bpr_update_user_kernel) or per-sample groups (bpr_update_kernel).  GORSE_TEST_BPR_USER_RUNS / _PER_SAMPLE
// of gorse_hip_test_set_variant override the library's default (USER_RUNS wins where both are set).
inline bool bpr_user_runs_enabled(int variant, bool by_default) {
    return (variant & GORSE_TEST_BPR_USER_RUNS) ? true : ((variant & GORSE_TEST_BPR_PER_SAMPLE) ? false : by_default);
}
enum BprSchedule { kBprSequential = 0, kBprPerSample = 1, kBprUserRuns = 2 };
struct BprSchedulePlan {
    BprSchedule schedule;
    int kernel_mode;  // what the update launch receives: launch_update's mode, or on user runs MODE_ATOMIC / MODE_STORES (the store route)
};
// user runs need enough users to fill the chip with one 16-lane group each (kUserRunUsers groups = one wave per SIMD) and a
// register-resident factor width (user_run_width); otherwise the per-sample schedule is the faster one (S-ml100k: 943 users).
// `forced`: GORSE_TEST_BPR_USER_RUNS, the schedule whatever the number of users.  The per-sample schedule has no store route: mode 3 is
// mode 0 there.  gorse_mf_create gives a handle the accumulated tier by the same two constants (hot_rows.hpp acc_rows_eligible): the
// tier is only correct on handles that run user runs.
inline BprSchedulePlan bpr_schedule(int mode, int d, int64_t U, bool user_runs_enabled, bool forced) {
    if (mode == MODE_EXACT) return BprSchedulePlan{kBprSequential, MODE_EXACT};
    if ((mode == MODE_ATOMIC || mode == MODE_STORES) && user_runs_enabled && user_run_width(d) && (U >= kUserRunUsers || forced))
        return BprSchedulePlan{kBprUserRuns, mode};
    return BprSchedulePlan{kBprPerSample, mode == MODE_STORES ? MODE_ATOMIC : mode};
}

// ---- the chunk --------------------------------------------------------------------------------------------------------------------
// Samples per chunk.  The user-run schedule loads p_u once per RUN (a user's samples inside one chunk), so a chunk should hold
// a few dozen samples per user: 4M samples serve the S-ml1m and C3-shard shapes (<= 125K users); the full C3 set (1M users)
// takes 32M, the 10M-user set 128M -- 64 bytes of triplet / pair / sort buffers per sample of capacity, 8.2 GB of the 288 at most.
// (override_samples > 0: gorse_hip_test_set_bpr_chunk)
inline int64_t bpr_chunk_capacity(int64_t U, int64_t override_samples) {
    if (override_samples > 0) return override_samples;
    const int64_t lo = (int64_t)1 << 22, hi = (int64_t)1 << 27;
    return std::min(std::max(lo, 32 * U), hi);
}
// samples per triplet buffer for a call that asks for `want`
inline size_t bpr_trip_capacity(int64_t want, int64_t chunk) {
    size_t cap = (size_t)std::min<int64_t>(std::max<int64_t>(want, 1), chunk);
    return (cap + 1) & ~(size_t)1;  // even: trip + cap is read as (sample id, user) pairs of 8 bytes
}

// ---- the preparation of a chunk (bpr_prepare.hip launch_prepare_users) --------------------------------------------------------------
constexpr int kFinCap = 6144;    // samples of a bin at most (bpr_bin_finish_kernel)
constexpr int kFinStage = 6144;  // row entries staged at most
constexpr int kFinShift = 9;     // log2 of the user ids per bin at most (one thread each in the scan)
constexpr size_t kItemsBatchFrom = (size_t)8 << 20;  // feedbacks of a handle beyond which the users' rows cannot all sit in the L2s
struct BprPrepRoute {
    PrepBins pb;
    bool binned;       // the preparation by user bins (bpr_bins.hpp), else an atomic per sample on its user's counter
    bool finish;       // binned: the bins finished in one LDS-resident pass (bpr_bin_finish_kernel), else three kernels through global memory
    bool batch_items;  // the item draws of the three-kernel and unbinned forms: four positions per thread (bpr_sample_items_batch_kernel)
};
// the finish of the bins in one LDS-resident pass (bpr_bin_finish_kernel) where a bin's expected samples are safely under
// its capacity (the 10M-user set: ~27,500 per bin), a bin's users have a counter each, and the users' rows sit in the L2s:
// where they do not (C3 shapes) the item draws are bpr_sample_items_batch_kernel's, four chains of look-ups per thread, which
// the finish kernel does not have; GORSE_TEST_BPR_THREE_KERNELS: the three kernels whatever the shape
inline BprPrepRoute bpr_prep_route(int64_t U, int64_t n, size_t uidx_n, int variant) {
    BprPrepRoute r;
    r.pb = prep_bins(U, n);
    r.binned = r.pb.ok && !(variant & GORSE_TEST_BPR_NO_BINS);
    r.finish = r.binned && !(variant & GORSE_TEST_BPR_THREE_KERNELS) && r.pb.shift <= kFinShift && n / r.pb.nbins <= kFinCap / 4 * 3 &&
               uidx_n <= kItemsBatchFrom;
    r.batch_items = uidx_n > kItemsBatchFrom;
    return r;
}

// the flat kernels of the preparation and of launch_user_sort (a sample per thread, grid-stride beyond the cap)
constexpr int kFlatThreads = 256;
inline int64_t bpr_flat_grid(int64_t n) { return std::min<int64_t>((n + kFlatThreads - 1) / kFlatThreads, 256 * 8); }

// exclusive scan of m counters (bpr_prepare.hip exclusive_scan_i32): the whole scan by ONE workgroup, tile after tile, up to
// kScanSmallTiles tiles; three launches (tile sums, scan of the tile sums, tile rescans) beyond
constexpr int kScanTile = 2048;  // elements per workgroup of the scan (256 threads x 8)
constexpr int kScanSmallTiles = 16;
inline int64_t bpr_scan_tiles(int64_t m) { return (m + kScanTile - 1) / kScanTile; }
inline bool bpr_scan_one_workgroup(int64_t m) { return bpr_scan_tiles(m) <= kScanSmallTiles; }

// ---- the update launches ------------------------------------------------------------------------------------------------------------
constexpr int kRunsPerBlock = 16;             // 16-lane groups of an update workgroup (cf_device.hpp kGroupsPerBlock): a run or a sample each
constexpr int64_t kUpdateBlocks = 256 * 16;  // worker workgroups at most: 16 workgroups of 4 waves per CU, grid-stride beyond that
constexpr int kFolderBlocks = 32;
// the tier's folders: 2,780 rows x 64 elements at C2 are 178 K (slot, element) pairs, 22 per thread of 32 workgroups and pass -- on
// the hot tier's 8,192 threads (11 pairs each today) they would not fit the period
constexpr int kFolderBlocksAcc = 32;
// folder workgroups of a launch that opens the rows (bpr_internal.hpp open_hot): none on a handle without hot or accumulated rows
inline int bpr_folders(int n_hot, int n_acc) { return n_hot > 0 || n_acc > 0 ? kFolderBlocks + (n_acc > 0 ? kFolderBlocksAcc : 0) : 0; }

// user runs (bpr_update_users.hip launch_update_users): a run per group; nFactors 8: two runs per group while GORSE_BPR_D8_PAIRS is on
inline int64_t bpr_user_run_workers(int64_t U, int d, bool d8_pairs) {
    const int64_t per = (int64_t)kRunsPerBlock * (d == 8 && d8_pairs ? 2 : 1);
    return std::min<int64_t>((U + per - 1) / per, kUpdateBlocks);
}
// the negative's slot look-up is one more gather per sample: where a draw has a fair chance of meeting a hot item (hot_rows.hpp;
// gorse_mf_create counted the negatives into the replica counts by the same rule)
// -- and always with the accumulated tier, where every item has a row
inline bool bpr_neg_replicas(int n_hot, int n_acc, int64_t I) { return n_acc > 0 || (n_hot > 0 && hot_neg_replicas(n_hot, I)); }
// cold items by store only in GORSE_BPR_HOGWILD_STORES and where the handle has any (n_cold) -- the atomics-only instantiation otherwise
// (store_mode: gorse_hip_test_set_bpr_store_mode)
inline bool bpr_neg_store(bool stores, int64_t n_cold, int store_mode) { return stores && n_cold > 0 && store_mode == 1; }
// The sole-writer fold (bpr_fold.hpp, above HotRows): with the tier neg_rep is 1 and every item's class word is >= 0, so without the
// store route no worker instruction of the user-run kernel addresses Q for writing -- the folders are the only writers of the rows they
// fold.  sole_writer: the value of GORSE_BPR_FOLD_SOLE_WRITER; has_base: the handle has the table of Q's rows as the launch found them.
inline bool bpr_fold_sole(bool sole_writer, int n_acc, bool neg_store, bool has_base) { return sole_writer && n_acc > 0 && !neg_store && has_base; }

// per-sample groups (bpr_update.hip launch_update_mode): a sample per group; folders only in GORSE_BPR_HOGWILD_ATOMIC
inline int64_t bpr_sample_workers(int64_t n) { return std::min<int64_t>((n + kRunsPerBlock - 1) / kRunsPerBlock, kUpdateBlocks); }
inline int bpr_sample_folders(int mode, int n_hot, int n_acc) { return mode == MODE_ATOMIC ? bpr_folders(n_hot, n_acc) : 0; }
// 16-float chunks of a factor row held in registers (the kernel's NC), 0 = the rows staged in LDS: three rows per group
inline int bpr_sample_chunks(int d) { return d == 16 ? 1 : (d == 32 ? 2 : (d == 64 ? 4 : (d == 128 ? 8 : 0))); }
inline size_t bpr_sample_lds_bytes(int d) { return bpr_sample_chunks(d) ? 0 : (size_t)kRunsPerBlock * 3 * d * sizeof(float); }
// bpr_fold_kernel after a per-sample launch with folders: an element of a hot or accumulated row per thread
constexpr int kFoldThreads = 256;
inline int64_t bpr_fold_grid(int n_hot, int n_acc, int d) {
    return std::min<int64_t>(((int64_t)(n_hot + n_acc) * d + kFoldThreads - 1) / kFoldThreads, 512);
}

}  // namespace gorse
