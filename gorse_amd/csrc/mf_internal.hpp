// mf_internal.hpp -- the gorse_mf handle: everything one model keeps resident in HBM.
#pragma once
#include <vector>

#include "cf_device.hpp"

#include "hot_rows.hpp"

#define GORSE_HOT_DONE_STRIPES 32  // words of the workers' arrival counter (bpr_fold.hpp worker_done), GORSE_HOT_DONE_STRIDE words apart
#define GORSE_HOT_DONE_STRIDE 64
// hot_done: two sets of arrival stripes (update launches alternate between them) and one line for the folders' pass counts (two words:
// the hot tier's, the accumulated tier's)
#define GORSE_HOT_DONE_WORDS (2 * GORSE_HOT_DONE_STRIPES * GORSE_HOT_DONE_STRIDE + GORSE_HOT_DONE_STRIDE)
#ifndef GORSE_HOT_REPLICAS
#define GORSE_HOT_REPLICAS 8  // replica rows of the hottest items (the most a slot gets, gorse_mf_create; bpr_fold.hpp kHotReplicas)
#endif

struct gorse_mf {
    int device = 0;
    int64_t U = 0, I = 0, nnz = 0;
    int64_t max_user_row = 0, max_item_row = 0;  // longest feedback rows
    int d = 0;
    bool has_item_csr = false;
    hipStream_t stream = nullptr;   // update kernels, copies
    hipStream_t stream2 = nullptr;  // sampler running ahead of the update kernels
    hipEvent_t ev_sampled[2] = {nullptr, nullptr};
    // A chunk's update launch carries ONE stop event, attached to its last kernel's dispatch (hipExtLaunchKernelGGL): the chunk's
    // "consumed" event the preparation of the chunk after next waits on, the epoch's end event when the chunk is the epoch's last, and
    // the profile's end of the update span -- no marker packet follows the kernel.  ev_consumed[b] = the stop event of the launch that
    // last read buffer b (null: nothing to wait for).  It is borrowed: the profile's stop event while profiling is on
    // (KernelProfile::events; mf_prof_resolve drops it before the profile takes its events back), the epoch's own end event for an
    // epoch's last chunk, a slot of ev_chunk otherwise.  A waiter is issued two chunks after the launch and a slot of ev_chunk is
    // attached again four chunks after it, so the wait has always been issued (and has taken hold of that launch) by then.
    hipEvent_t ev_consumed[2] = {nullptr, nullptr};
    static constexpr int kChunkRing = 4;
    hipEvent_t ev_chunk[kChunkRing] = {};
    // epoch pacing (gorse_mf_epoch_throttle / gorse_mf_epoch_times): a ring of (begin, end) event pairs, one per BPR epoch, on the
    // update stream; created with the first epoch.  ep_seq = epochs issued, ep_done = epochs whose events have been read.
    // end = the stop event of the epoch's last update launch: ev_ep_end[slot] is what the readers use, either the ring's own event
    // (ev_ep_end_own) or, while profiling is on, the profile's.  begin = the start event of the epoch's first update launch, or a
    // recorded event where something else of the epoch precedes that launch on the stream (epoch_impl, csrc/bpr.hip).
    static constexpr int kEpochRing = 16;
    hipEvent_t ev_ep_begin[kEpochRing] = {}, ev_ep_end[kEpochRing] = {}, ev_ep_end_own[kEpochRing] = {};
    bool ep_events = false;
    // An epoch that is enqueued while the one before it is still in flight, with nothing else issued on the handle in between (ep_chain:
    // set by the epoch, cleared by every other entry point through use()), begins where that one ended: its begin IS the previous slot's
    // end event (ep_begin_prev) and no event of its own is recorded -- one barrier packet less in front of its update kernel.
    bool ep_begin_prev[kEpochRing] = {};
    mutable bool ep_chain = false;
    uint64_t ep_seq = 0, ep_done = 0;
    double ep_ms = 0.0;     // device milliseconds of the epochs read so far (since the last reset)
    int64_t ep_timed = 0;   // how many epochs that sum covers
    int64_t ep_untimed = 0; // epochs whose events were overwritten before anybody read them (more than kEpochRing in flight)
    // factors, row-major, row stride d (rows 16-byte aligned whenever d % 4 == 0)
    gorse::DevBuf<float> P, Q, Qsync;
    // dataset.CFSplit user->items (stored order + row-sorted copy) and item->users
    gorse::DevBuf<int64_t> uptr, iptr;
    gorse::DevBuf<int32_t> uidx, uidx_sorted, iidx;
    // BPR triplet chunk buffers (double-buffered: sampler fills one while the other is applied)
    gorse::DevBuf<int32_t> trip[2];
    size_t trip_cap = 0;  // samples per buffer
    // user-run schedule (bpr_prepare.hip, bpr_update_users.hip): the chunk's triplets counting-sorted by user
    gorse::DevBuf<int32_t> sorted[2];  // su | si | sj, each trip_cap long
    gorse::DevBuf<int32_t> ubucket[2]; // U + 2 run offsets per triplet buffer (sorted on stream2)
    gorse::DevBuf<int32_t> urank[2];   // arrival rank of a sample inside its user's run, per triplet buffer
    gorse::DevBuf<int32_t> scan_tmp2;  // per-tile sums of the sort's scan (the sort may run on the sampler stream)
    gorse::DevBuf<int32_t> ubins;      // binned preparation: bin totals, bin starts at kMaxBins (preparations are serial: one copy)
    gorse::DevBuf<int32_t> ubinmat;    // binned preparation: the tile x bin count matrix
    int64_t chunk_seq = 0;             // chunks enqueued so far: buffer = chunk_seq & 1, across calls
    // hot-row replicas of the Hogwild schedule (bpr_fold.hpp): popular items' updates land here.  hot_meta[slot] = hot_code(first row,
    // log2 replica count) (hot_rows.hpp), the same word hot_slot holds for the slot's item; hot_rep holds hot_rows rows of d floats.
    gorse::DevBuf<int32_t> hot_slot, hot_items, hot_meta, hot_done;
    gorse::DevBuf<float> hot_rep;
    int n_hot = 0;
    int64_t hot_rows = 0;       // replica rows in all (the sum of the slots' counts)
    // the accumulated tier (hot_rows.hpp acc_rows_layout): n_acc warm items with one row each behind the hot_rows replica rows of
    // hot_rep; their slots are entries n_hot .. n_hot + n_acc of hot_items / hot_meta
    int n_acc = 0;
    // handles with the tier: n_hot + n_acc rows of d floats, the slots' rows of Q as an update launch in the sole-writer form found
    // them (bpr_fold.hpp, above HotRows); written and read by that launch's folders only, its content means nothing between two launches
    gorse::DevBuf<float> hot_base;
    int fold_sole_last = 0;     // whether the last update launch with folders took that form (gorse_hip_test_bpr_fold_tier_stats)
    uint64_t hot_launches = 0;  // update launches with folders so far: the parity picks the launch's set of arrival stripes
    int64_t n_cold = 0;  // items of class "cold" in hot_slot (-2): updates by write-through store (bpr_update_users.hip)
    int64_t cold_window = 0;               // what n_cold was computed for (gorse_mf_set_bpr_cold_window)
    std::vector<int32_t> h_item_count;     // training feedbacks per item and
    std::vector<int32_t> h_hot_slot;       // the class of every item (hot_code, -1 warm, -2 cold) as last uploaded: host copies for a re-classification
    gorse::DevBuf<int32_t> order;  // sequential mode: samples sorted by dependency level
    gorse::DevBuf<double> loss;
    gorse::DevBuf<int32_t> fail_count;
    // ALS scratch
    gorse::DevBuf<float> gram, gram_partial, als_scratch;
    // ALS row plan per side (0 = user rows, 1 = item rows), built at create time (als.hip):
    // rows with at most kAlsLongRow feedbacks are solved by one wave each (list sorted by length,
    // longest first); longer rows are cut into chunks whose partial Gram matrices are reduced
    // in chunk order by the long-row solver.
    struct AlsPlan {
        gorse::DevBuf<int32_t> short_rows;               // n_short row ids
        gorse::DevBuf<int32_t> chunk_row, chunk_cnt;     // n_chunks
        gorse::DevBuf<int32_t> chunk_order;              // n_chunks: the chunks longest first
        gorse::DevBuf<int64_t> chunk_beg;                // n_chunks: offset into the side's indices
        gorse::DevBuf<int32_t> long_rows, long_first, long_nch;  // n_long
        gorse::DevBuf<int32_t> long_ident, long_one;             // n_long: 0, 1, 2, ... and 1, 1, 1, ... (the solve after als_partial_reduce_kernel)
        int32_t max_nch = 0;                                     // most chunks of one row
        // rows with feedback (the rows S = sum x x^T runs over, model.go:645-658), cut into Gram chunks
        gorse::DevBuf<int32_t> fb_rows, g_cnt;
        gorse::DevBuf<int64_t> g_beg;
        int64_t n_short = 0, n_chunks = 0, n_long = 0, n_fb_rows = 0, n_gchunks = 0;
    } als_plan[2];
    std::vector<int64_t> h_uptr, h_iptr;      // host copies of the CSR row pointers (row plans are rebuilt from them)
    int64_t als_lo[2] = {0, 0}, als_hi[2] = {0, 0};  // row range of each side this handle solves (gorse_als_set_ranges)
    gorse::DevBuf<float> als_partial;  // n_chunks x (d*d + d) partial Gram matrices + column sums
    gorse::DevBuf<float> als_reduced;  // n_long x (d*d + d): a long row's partials added up (als_partial_reduce_kernel)
    // Evaluate's resident split (eval.hip): the test rows, every user's sampled negatives, and the candidate CSR of the users
    // with test feedback (user ids ascending, "test items then negatives" per user)
    gorse::DevBuf<int64_t> ev_tptr, ev_upos, ev_cpos, ev_cptr;
    gorse::DevBuf<int32_t> ev_tidx, ev_neg, ev_neglen, ev_has, ev_clen, ev_users, ev_cand;
    int64_t ev_users_n = 0, ev_cand_n = 0;
    bool ev_valid = false;
    uint64_t ev_generation = 0;  // bumped by every gorse_mf_sample_user_negatives (gorse_mf_resident_generation)
    // gorse_mf_evaluate / _resident (mf_eval.hip): the 1 / log2 and IDCG tables, the stage events (both made by the first call), and
    // the last call's users counted, candidates scored and device milliseconds (per-user kernel | sum chain)
    gorse::DevBuf<float> mfe_tab;
    hipEvent_t mfe_ev[3] = {nullptr, nullptr, nullptr};
    int64_t mfe_users = 0, mfe_cands = 0;
    double mfe_ms[2] = {0.0, 0.0};
    // generic staging
    gorse::DevBuf<char> stage, rank_in;
    // gorse_mf_recommend (recommend.hip): its inputs, the fast path's buffers, the literal path's candidate lists; the last call's split
    gorse::DevBuf<char> rec_in, rec_buf, rec_lit;
    gorse::DevBuf<char> rec_seen;  // gorse_mf_recommend's seen rows, sorted (row pointer | items); the candidate chain brings its own
    int64_t rec_fast = 0, rec_literal = 0;
    double rec_ms = 0.0;
    gorse::KernelProfile prof{GORSE_PROF_NCLASSES};

    int32_t use() const {
        ep_chain = false;  // (an entry point that issues nothing restores it: gorse_mf_epoch_throttle / _times)
        hipError_t e = hipSetDevice(device);
        if (e != hipSuccess) return gorse::fail(GORSE_ERR_HIP, "hipSetDevice(%d): %s", device, hipGetErrorString(e));
        return GORSE_OK;
    }
};

namespace gorse {
// implemented in mf.hip / als.hip, used across files (the BPR units' own: bpr_internal.hpp)
int32_t mf_sync_streams(gorse_mf *h);
// epoch pacing: mark the begin / end of one epoch on the update stream; read the finished ones (wait = block for all of them)
// (begin: `record` = the caller issues other work of the epoch in front of its first update launch, *attach = the start event that
// launch takes otherwise; end: `attached` = the stop event the epoch's last update launch took -- mf_epoch_end_event() or the
// profile's -- or null to record one)
int32_t mf_epoch_begin(gorse_mf *h, bool chained, bool record, hipEvent_t *attach);
hipEvent_t mf_epoch_end_event(gorse_mf *h);
int32_t mf_epoch_end(gorse_mf *h, hipEvent_t attached);
int32_t mf_prof_resolve(gorse_mf *h);  // KernelProfile::resolve of the handle's profile, after letting go of the events borrowed from it
int32_t mf_epoch_harvest(gorse_mf *h, bool wait);
int32_t mf_delta_export_async(gorse_mf *h, float *dst);        // mf.hip: dst <- Q - Q_sync, enqueued on h->stream
int32_t mf_delta_import_async(gorse_mf *h, const float *src);  // mf.hip: Q <- Q_sync + src; Q_sync <- Q
int32_t als_build_plan(gorse_mf *h, int side, const int64_t *ptr, int64_t rows, int64_t lo, int64_t hi);
int32_t mf_score_device(gorse_mf *h, const int32_t *us, const int32_t *is, int64_t n, float *out);  // mf_rank.hip: internalPredict, device pointers

// Users' lists ON THE DEVICE, as Rank and Evaluate take them: n_users user ids, their candidate CSR (n_cand entries in all) and, for
// an evaluation, the target rows -- row users[t] of the CSR (tgt_by_user) or row t.
struct UserLists {
    int64_t n_users = 0;
    const int32_t *users = nullptr;
    const int64_t *cand_ptr = nullptr;
    const int32_t *cand = nullptr;
    int64_t n_cand = 0;
    const int64_t *tgt_ptr = nullptr;
    const int32_t *tgt = nullptr;
    bool tgt_by_user = false;
};
// mf_rank.hip: a caller's host lists, validated (ids in range, row pointers from 0 and monotone; the target CSR only when
// target_indptr is given) and copied to h->rank_in behind everything enqueued on the handle; *n_counted (may be null) = users with
// a target.  n_users == 0: empty lists.
int32_t upload_user_lists(gorse_mf *h, int64_t n_users, const int32_t *users, const int64_t *cand_indptr, const int32_t *cand,
                          const int64_t *target_indptr, const int32_t *targets, UserLists *lists, int64_t *n_counted);
// mf_rank.hip: the lists gorse_mf_sample_user_negatives left on the handle (eval.hip), with its test split as the target rows
int32_t resident_user_lists(gorse_mf *h, UserLists *lists);
// mf_rank.hip: Rank + TopKFilter over the lists; the rank lists go to the host arrays (n_users * topk padded with -1, lengths),
// enqueued on h->stream -- the caller synchronises
int32_t mf_rank_device(gorse_mf *h, const UserLists &L, int32_t topk, int32_t *rank_out, int32_t *rank_len);

// recommend.hip, in two halves so that the candidate chain (cand.hip) searches under its own device-resident exclusion rows.
// check: gorse_mf_recommend's validation of everything but the seen rows.
// core: the search.  The seen rows are a CSR on the device with ASCENDING rows (d_sptr from 0; NULL: no seen rows).  dev == NULL: the
// result rows go to the host arrays (each may be NULL), as gorse_mf_recommend returns them.  dev != NULL (k <= 256): the n_users * k
// rows and the counts are left in the caller's device buffers instead -- the threshold path's chunks copied device to device, the
// literal path's few rows uploaded at the end -- and the host arrays are not written.  Returns with the handle's stream idle.
struct MfDeviceRows {
    int32_t *items = nullptr;
    float *scores = nullptr;
    int32_t *cnt = nullptr;
};
int32_t mf_recommend_check(gorse_mf *h, int64_t n_users, const int32_t *users, int32_t k);
int32_t mf_recommend_core(gorse_mf *h, int64_t n_users, const int32_t *users, int32_t k, const uint8_t *item_ok, const int64_t *d_sptr,
                          const int32_t *d_seen, int32_t *items_out, float *scores_out, int32_t *count_out, const MfDeviceRows *dev);
}
