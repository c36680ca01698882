// bpr.hip -- the driver of the BPR training step on gfx950.  Reference: model/cf/model.go:446-494.
//
// This unit holds the epoch (epoch_impl: the chunk loop and its two-stream pipeline), the sequential parity schedule (build_levels,
// run_sequential), the choice of the schedule and every extern "C" entry.  The kernels live in one unit per stage:
//   bpr_prepare.hip       : bpr_sample_kernel (the whole triplet per thread: per-sample and sequential schedules,
//                           gorse_bpr_sample_triplets); bpr_sample_user_kernel, scan + bpr_scatter_ids, bpr_sample_items[_batch]_kernel
//                           (the user-run schedule's preparation without bins); bpr_bin_count / _offsets / _scatter / _sort / _finish
//                           (the preparation by user bins); bpr_group_positives_kernel; bpr_rank / bpr_scatter_by (triplets sorted by
//                           user) and the scan kernels.  The sample stream itself is stated once, in bpr_stream.hpp.
//   bpr_update_users.hip  : bpr_update_user_kernel, model.go:469-488 -- one 16-lane group applies ALL samples of one user (the
//                           user-run schedule: the production Hogwild form for >= 4096 users and nFactors 8/16/32/64/128).
//   bpr_update.hip        : bpr_update_kernel, the per-sample form (the sequential parity schedule, the racy diagnostic, and the
//                           Hogwild schedule of shapes with few users or another factor width), and bpr_fold_kernel.
//   bpr_fold.hpp          : HotRows and the folder workgroups of an update launch (device header of both update units).
// The rules the host decides by -- schedule, chunk capacity, preparation route, grids, folder counts -- are bpr_plan.hpp's, each
// written once; bpr_internal.hpp has the prototypes that cross units and the test state.
// HBM-bound: algorithmic bytes per sample = 6*d*4 (three rows read + three written) + 12 (indices).
// Test switches: the six GORSE_TEST_BPR_* bits of include/gorse_hip_test.h choose between equivalent schedules and preparations;
// the chunk loop of epoch_impl has two forms, the product's and GORSE_TEST_BPR_STABLE_RANK's.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "bpr_internal.hpp"

using namespace gorse;

// the switches of the tests and probes (bpr_internal.hpp); nothing of it reaches a kernel
BprTestState gorse::g_bpr;

namespace {

// Dependency levels: level(s) = 1 + max(level of the last earlier sample touching P[u], Q[i], Q[j]).
// Samples of one level touch pairwise disjoint rows, and every pair of conflicting samples keeps its
// stream order across levels, so running level after level reproduces the sequential (Jobs = 1,
// common/parallel/parallel.go:34-43) result exactly.
void build_levels(int64_t U, int64_t I, const int32_t *u, const int32_t *i, const int32_t *j, int64_t n,
                  std::vector<int32_t> &order, std::vector<int64_t> &level_ptr) {
    std::vector<int32_t> lastP((size_t)U, 0), lastQ((size_t)I, 0), lvl((size_t)n, 0);
    int32_t maxl = 0;
    for (int64_t s = 0; s < n; s++) {
        if ((u[s] | i[s] | j[s]) < 0) continue;  // skipped sample: level 0 = never launched
        int32_t l = std::max(lastP[u[s]], std::max(lastQ[i[s]], lastQ[j[s]])) + 1;
        lvl[s] = l;
        lastP[u[s]] = l;
        lastQ[i[s]] = l;
        lastQ[j[s]] = l;
        maxl = std::max(maxl, l);
    }
    level_ptr.assign((size_t)maxl + 2, 0);
    for (int64_t s = 0; s < n; s++) level_ptr[lvl[s] + 1]++;
    for (int32_t l = 0; l <= maxl; l++) level_ptr[l + 1] += level_ptr[l];
    order.resize((size_t)n);
    std::vector<int64_t> cur(level_ptr.begin(), level_ptr.end() - 1);
    for (int64_t s = 0; s < n; s++) order[cur[lvl[s]]++] = (int32_t)s;
}

// sequential schedule over device-resident triplets (us/is/js) whose host copy is (hu, hi, hj)
int32_t run_sequential(gorse_mf *h, const int32_t *d_us, const int32_t *d_is, const int32_t *d_js, const int32_t *hu,
                       const int32_t *hi, const int32_t *hj, int64_t n, float lr, float reg, int exp_mode,
                       const volatile int32_t *cancel, double *d_loss) {
    std::vector<int32_t> order;
    std::vector<int64_t> level_ptr;
    build_levels(h->U, h->I, hu, hi, hj, n, order, level_ptr);
    GORSE_TRY(h->order.ensure((size_t)n));
    GORSE_HIP_CHECK(hipMemcpyAsync(h->order.p, order.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    const size_t nlev = level_ptr.size() - 1;
    for (size_t l = 1; l < nlev; l++) {  // level 0 holds skipped samples
        if (cancel && *cancel && (l & 255) == 0) {
            GORSE_HIP_CHECK(hipStreamSynchronize(h->stream));
            return fail(GORSE_ERR_CANCELLED, "cancelled");
        }
        GORSE_TRY(bpr_launch_update(h, MODE_EXACT, d_us, d_is, d_js, h->order.p, level_ptr[l], level_ptr[l + 1], lr, reg,
                                    exp_mode, d_loss, h->stream));
    }
    GORSE_HIP_CHECK(hipStreamSynchronize(h->stream));  // `order` (host vector) was copied asynchronously
    return GORSE_OK;
}

// Hogwild schedule: 1 = user runs (bpr_update_user_kernel), 0 = per-sample groups (bpr_update_kernel).  The
// environment variable GORSE_BPR_SCHEDULE = "users" | "samples" overrides the compiled default (read once);
// GORSE_TEST_BPR_USER_RUNS / _PER_SAMPLE of gorse_hip_test_set_variant override both.
bool user_runs_default() {
    static const int v = [] {
        const char *e = getenv("GORSE_BPR_SCHEDULE");
        if (e && !strcmp(e, "users")) return 1;
        if (e && !strcmp(e, "samples")) return 0;
        return g_bpr.user_runs;
    }();
    return v != 0;
}
// the schedule of handle h for a call in `mode`, and the kernel mode its update launch receives (bpr_plan.hpp bpr_schedule)
BprSchedulePlan schedule_of(const gorse_mf *h, int mode) {
    return bpr_schedule(mode, h->d, h->U, bpr_user_runs_enabled(g_bpr.variant, user_runs_default()),
                        (g_bpr.variant & GORSE_TEST_BPR_USER_RUNS) != 0);
}

int32_t check_mode(int mode) {
    if (mode != MODE_ATOMIC && mode != MODE_EXACT && mode != MODE_RACY && mode != MODE_STORES)
        return fail(GORSE_ERR_INVALID, "unknown BPR mode %d", mode);
    return GORSE_OK;
}

int32_t epoch_impl(gorse_mf *h, int64_t n_samples, float lr, float reg, uint64_t seed, uint64_t epoch, int64_t base,
                   int mode, const volatile int32_t *cancel, double *loss_out, bool sync) {
    if (!h) return fail(GORSE_ERR_INVALID, "handle is NULL");
    if (n_samples < 0) return fail(GORSE_ERR_INVALID, "n_samples < 0");
    GORSE_TRY(check_mode(mode));
    const bool chained = h->ep_chain;  // the previous epoch was the last thing issued on this handle (mf_internal.hpp: ep_begin_prev)
    GORSE_TRY(h->use());
    if (n_samples == 0) {
        if (loss_out) *loss_out = 0;
        return GORSE_OK;
    }
    GORSE_TRY(bpr_ensure_trip(h, n_samples));
    double *d_loss = loss_out ? h->loss.p : nullptr;
    // Epoch pacing: the (begin, end) pair gorse_mf_epoch_throttle / _times read (csrc/mf.hip).  Between two update kernels the update
    // stream carries the wait on the chunk's preparation and nothing else: the epoch's end, the chunk's "consumed" event and the
    // profile's span are the launch's own events (ev_consumed, mf_internal.hpp).  An epoch that does not begin where the one before it
    // ended takes its begin from its first update launch (ep_begin) -- unless something else of the epoch comes first on the stream (the
    // loss memset, the sequential schedule's sampler, the sort of GORSE_TEST_BPR_STABLE_RANK) or the profile needs that launch's start
    // event: then the begin is recorded where the stream reaches the epoch, as the only marker packet of the epoch.
    const BprSchedulePlan plan = schedule_of(h, mode);
    const bool uruns = plan.schedule == kBprUserRuns;
    const bool stable_rank = uruns && (g_bpr.variant & GORSE_TEST_BPR_STABLE_RANK);  // the sort on the update stream, by one thread
    hipEvent_t ep_begin = nullptr, ep_end = nullptr;
    GORSE_TRY(mf_epoch_begin(h, chained, d_loss || mode == MODE_EXACT || stable_rank || h->prof.on, &ep_begin));
    if (d_loss) GORSE_HIP_CHECK(hipMemsetAsync(d_loss, 0, sizeof(double), h->stream));
    const int64_t cap = (int64_t)h->trip_cap;
    if (plan.schedule == kBprSequential) {
        std::vector<int32_t> host((size_t)cap * 3);
        for (int64_t s0 = 0; s0 < n_samples; s0 += cap) {
            const int64_t m = std::min(cap, n_samples - s0);
            int32_t *tb = h->trip[0].p;
            GORSE_TRY(bpr_launch_sampler(h, seed, epoch, base + s0, m, tb, (size_t)cap, h->stream));
            GORSE_HIP_CHECK(hipMemcpyAsync(host.data(), tb, (size_t)cap * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
            GORSE_HIP_CHECK(hipStreamSynchronize(h->stream));
            GORSE_TRY(run_sequential(h, tb, tb + cap, tb + 2 * cap, host.data(), host.data() + cap, host.data() + 2 * cap, m,
                                     lr, reg, g_bpr.exp_mode_exact, cancel, d_loss));
        }
    } else {
        // two-stream pipeline: stream2 samples (and item-sorts) chunk c+1 while stream applies chunk c; the
        // buffer parity runs on across calls so that back-to-back enqueued epochs overlap as well
        if (uruns) GORSE_TRY(bpr_ensure_user_sort(h));
        int64_t c = 0;
        for (int64_t s0 = 0; s0 < n_samples; s0 += cap, c++) {
            const int b = (int)(h->chunk_seq & 1);
            h->chunk_seq++;
            const int64_t m = std::min(cap, n_samples - s0);
            if (cancel && *cancel) {
                GORSE_TRY(mf_sync_streams(h));
                return fail(GORSE_ERR_CANCELLED, "cancelled");
            }
            int32_t *tb = h->trip[b].p;
            const hipStream_t prep = h->stream2;
            // the update launch that last read this buffer (none: the first two chunks of a handle, or the streams were drained since)
            if (h->ev_consumed[b]) GORSE_HIP_CHECK(hipStreamWaitEvent(prep, h->ev_consumed[b], 0));
            // user runs: the whole preparation of chunk c + 1 (launch_prepare_users) runs on the preparation stream under the update
            // kernel of chunk c; otherwise (the per-sample schedule, GORSE_TEST_BPR_STABLE_RANK) the sampler alone, its span the launch's own
            if (uruns && !stable_rank) {
                GORSE_TRY(bpr_launch_prepare_users(h, seed, epoch, base + s0, m, tb, h->sorted[b].p, h->ubucket[b].p, h->urank[b].p,
                                                   (size_t)cap, prep));
            } else {
                hipEvent_t sa = nullptr, sb = nullptr;
                h->prof.events(GORSE_PROF_BPR_SAMPLE, &sa, &sb);
                GORSE_TRY(bpr_launch_sampler(h, seed, epoch, base + s0, m, tb, (size_t)cap, prep, sa, sb));
            }
            GORSE_HIP_CHECK(hipEventRecord(h->ev_sampled[b], prep));
            GORSE_HIP_CHECK(hipStreamWaitEvent(h->stream, h->ev_sampled[b], 0));
            if (stable_rank) {  // the triplets ranked by one thread and scattered, on the update stream
                const int tok = h->prof.begin(GORSE_PROF_BPR_SORT, h->stream);
                GORSE_TRY(bpr_launch_user_sort(h, tb, h->sorted[b].p, h->ubucket[b].p, h->urank[b].p, m, (size_t)cap, h->stream));
                h->prof.end(tok, h->stream);
            }
            // the launch's events: start = the profile's span, or the epoch's begin (first chunk, not chained, profiling off); stop = the
            // profile's, the epoch's end (last chunk) or a slot of the chunk ring -- whichever it is, it is the chunk's consumed event
            hipEvent_t start = nullptr, stop = nullptr;
            h->prof.events(GORSE_PROF_BPR_UPDATE, &start, &stop);
            const bool last = s0 + cap >= n_samples;
            if (!start && c == 0) start = ep_begin;
            if (!stop) stop = last ? mf_epoch_end_event(h) : h->ev_chunk[(h->chunk_seq - 1) % gorse_mf::kChunkRing];
            if (uruns)
                GORSE_TRY(bpr_launch_update_users(h, h->sorted[b].p, h->ubucket[b].p, (size_t)cap, lr, reg, g_bpr.exp_mode_exact, d_loss,
                                                  h->stream, plan.kernel_mode == MODE_STORES, start, stop));
            else  // (the per-sample schedule has no store route: mode 3 is mode 0 there)
                GORSE_TRY(bpr_launch_update(h, plan.kernel_mode, tb, tb + cap, tb + 2 * cap, nullptr, 0, m, lr, reg, 0, d_loss, h->stream, start,
                                            stop));
            h->ev_consumed[b] = stop;
            if (last) ep_end = stop;
            if (cancel && (c & 7) == 7) GORSE_TRY(mf_sync_streams(h));
        }
    }
    GORSE_TRY(mf_epoch_end(h, ep_end));  // (the sequential schedule has no launch to bind it to: recorded)
    h->ep_chain = true;
    if (sync || loss_out) {
        if (loss_out)
            GORSE_HIP_CHECK(hipMemcpyAsync(loss_out, h->loss.p, sizeof(double), hipMemcpyDeviceToHost, h->stream));
        GORSE_TRY(mf_sync_streams(h));
        GORSE_TRY(mf_epoch_harvest(h, true));  // every epoch issued so far is done: their device times are read now
    }
    return GORSE_OK;
}

}  // namespace

extern "C" void gorse_hip_test_set_exact_exp(int32_t mode) { g_bpr.exp_mode_exact = mode; }

extern "C" int32_t gorse_mf_bpr_schedule(gorse_mf *h, int32_t *user_runs) {
    if (!h || !user_runs) return fail(GORSE_ERR_INVALID, "NULL argument");
    *user_runs = schedule_of(h, MODE_ATOMIC).schedule == kBprUserRuns ? 1 : 0;
    return GORSE_OK;
}
extern "C" void gorse_hip_test_set_variant(int32_t v) {
    g_bpr.variant = v & (GORSE_TEST_BPR_USER_RUNS | GORSE_TEST_BPR_PER_SAMPLE | GORSE_TEST_BPR_STABLE_RANK | GORSE_TEST_BPR_THREE_KERNELS |
                         GORSE_TEST_BPR_ARRIVAL_ORDER | GORSE_TEST_BPR_NO_BINS);
}
extern "C" void gorse_hip_test_set_bpr_chunk(int64_t samples) { g_bpr.chunk_override = samples; }
extern "C" int32_t gorse_hip_test_bpr_fail_count(gorse_mf *h, int32_t *count) {
    if (!h || !count) return fail(GORSE_ERR_INVALID, "NULL argument");
    GORSE_TRY(h->use());
    GORSE_TRY(mf_sync_streams(h));
    GORSE_HIP_CHECK(hipMemcpy(count, h->fail_count.p, sizeof(int32_t), hipMemcpyDeviceToHost));
    return GORSE_OK;
}
extern "C" void gorse_hip_test_bpr_finish_capacities(int32_t *samples, int32_t *row_entries) {
    if (samples) *samples = kFinCap;
    if (row_entries) *row_entries = kFinStage;
}
extern "C" void gorse_hip_test_set_bpr_store_mode(int32_t store_mode) {
    // only bit 0 selects a form the library carries (cold negatives by store); the forms bits 1 and 2 asked for were removed
    g_bpr.store_mode = store_mode < 0 ? kDefaultStoreMode : (store_mode & 1);
}
extern "C" void gorse_hip_test_set_bpr_fold_period(int32_t ticks) { g_bpr.fold_period = ticks > 0 ? (uint32_t)ticks : kDefaultFoldPeriod; }
extern "C" void gorse_hip_test_set_bpr_acc_fold_every(int32_t periods) { g_bpr.acc_fold_every = periods > 0 ? periods : kDefaultAccFoldEvery; }
extern "C" int32_t gorse_hip_test_bpr_fold_stats(gorse_mf *h, int64_t *out3) {
    if (!h || !out3) return fail(GORSE_ERR_INVALID, "NULL argument");
    GORSE_TRY(h->use());
    GORSE_TRY(mf_sync_streams(h));
    int32_t passes = 0;
    if (h->hot_done.p)
        GORSE_HIP_CHECK(hipMemcpy(&passes, h->hot_done.p + kFoldPassesWord, sizeof(int32_t), hipMemcpyDeviceToHost));
    out3[0] = passes, out3[1] = h->n_hot, out3[2] = h->hot_rows;
    return GORSE_OK;
}
extern "C" void gorse_hip_test_set_bpr_folder_timeout(int64_t ticks) { g_bpr.folder_timeout = ticks > 0 ? (uint64_t)ticks : kFolderTimeout; }
extern "C" int32_t gorse_hip_test_bpr_fold_tier_stats(gorse_mf *h, int64_t *out6) {
    if (!h || !out6) return fail(GORSE_ERR_INVALID, "NULL argument");
    GORSE_TRY(h->use());
    GORSE_TRY(mf_sync_streams(h));
    int32_t passes[2] = {0, 0};
    if (h->hot_done.p)
        GORSE_HIP_CHECK(hipMemcpy(passes, h->hot_done.p + kFoldPassesWord, sizeof(passes), hipMemcpyDeviceToHost));
    out6[0] = passes[0], out6[1] = h->n_acc > 0 ? passes[1] : 0, out6[2] = h->n_hot, out6[3] = h->hot_rows, out6[4] = h->n_acc;
    out6[5] = h->fold_sole_last;
    return GORSE_OK;
}
extern "C" int32_t gorse_hip_test_bpr_hot_state(gorse_mf *h, int32_t *items, int32_t *replicas, float *rep) {
    if (!h) return fail(GORSE_ERR_INVALID, "handle is NULL");
    GORSE_TRY(h->use());
    GORSE_TRY(mf_sync_streams(h));
    const size_t n = (size_t)h->n_hot;
    std::vector<int32_t> meta(n);
    if (n > 0) {
        if (items) GORSE_HIP_CHECK(hipMemcpy(items, h->hot_items.p, n * sizeof(int32_t), hipMemcpyDeviceToHost));
        GORSE_HIP_CHECK(hipMemcpy(meta.data(), h->hot_meta.p, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    if (replicas)
        for (size_t s = 0; s < n; s++) replicas[s] = 1 << hot_lg(meta[s]);
    if (rep && h->hot_rows > 0)
        GORSE_HIP_CHECK(hipMemcpy(rep, h->hot_rep.p, (size_t)h->hot_rows * h->d * sizeof(float), hipMemcpyDeviceToHost));
    return GORSE_OK;
}

extern "C" int32_t gorse_hip_test_bpr_acc_state(gorse_mf *h, int32_t *items, float *rows) {
    if (!h) return fail(GORSE_ERR_INVALID, "handle is NULL");
    GORSE_TRY(h->use());
    GORSE_TRY(mf_sync_streams(h));
    const size_t n = (size_t)h->n_acc;
    if (n == 0) return GORSE_OK;
    if (items) GORSE_HIP_CHECK(hipMemcpy(items, h->hot_items.p + h->n_hot, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (rows)
        GORSE_HIP_CHECK(hipMemcpy(rows, h->hot_rep.p + (size_t)h->hot_rows * h->d, n * h->d * sizeof(float), hipMemcpyDeviceToHost));
    return GORSE_OK;
}
extern "C" int32_t gorse_hip_test_bpr_item_classes(gorse_mf *h, int32_t *slot, int64_t *out2) {
    if (!h) return fail(GORSE_ERR_INVALID, "handle is NULL");
    GORSE_TRY(h->use());
    GORSE_TRY(mf_sync_streams(h));
    if (slot && h->hot_slot.p) GORSE_HIP_CHECK(hipMemcpy(slot, h->hot_slot.p, (size_t)h->I * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (out2) out2[0] = h->n_acc, out2[1] = h->n_cold;
    return GORSE_OK;
}

extern "C" int32_t gorse_bpr_epoch(gorse_mf *h, int64_t n_samples, float lr, float reg, uint64_t seed, uint64_t epoch,
                                   int64_t sample_base, int32_t mode, const volatile int32_t *cancel, double *loss_out) {
    return epoch_impl(h, n_samples, lr, reg, seed, epoch, sample_base, mode, cancel, loss_out, true);
}

extern "C" int32_t gorse_bpr_epoch_enqueue(gorse_mf *h, int64_t n_samples, float lr, float reg, uint64_t seed,
                                           uint64_t epoch, int64_t sample_base, int32_t mode) {
    if (mode == MODE_EXACT) return fail(GORSE_ERR_INVALID, "the sequential schedule cannot be enqueued asynchronously");
    return epoch_impl(h, n_samples, lr, reg, seed, epoch, sample_base, mode, nullptr, nullptr, false);
}

extern "C" int32_t gorse_bpr_sample_triplets(gorse_mf *h, int64_t n, uint64_t seed, uint64_t epoch, int64_t sample_base,
                                             int32_t *u, int32_t *i, int32_t *j) {
    if (!h) return fail(GORSE_ERR_INVALID, "handle is NULL");
    if (n < 0 || (n > 0 && (!u || !i || !j))) return fail(GORSE_ERR_INVALID, "bad arguments");
    if (n == 0) return GORSE_OK;
    GORSE_TRY(h->use());
    GORSE_TRY(bpr_ensure_trip(h, n));
    GORSE_TRY(mf_sync_streams(h));
    const int64_t cap = (int64_t)h->trip_cap;
    for (int64_t s0 = 0; s0 < n; s0 += cap) {
        const int64_t m = std::min(cap, n - s0);
        int32_t *tb = h->trip[0].p;
        GORSE_TRY(bpr_launch_sampler(h, seed, epoch, sample_base + s0, m, tb, (size_t)cap, h->stream));
        GORSE_HIP_CHECK(hipMemcpyAsync(u + s0, tb, (size_t)m * 4, hipMemcpyDeviceToHost, h->stream));
        GORSE_HIP_CHECK(hipMemcpyAsync(i + s0, tb + cap, (size_t)m * 4, hipMemcpyDeviceToHost, h->stream));
        GORSE_HIP_CHECK(hipMemcpyAsync(j + s0, tb + 2 * cap, (size_t)m * 4, hipMemcpyDeviceToHost, h->stream));
        GORSE_HIP_CHECK(hipStreamSynchronize(h->stream));
    }
    return GORSE_OK;
}

extern "C" int32_t gorse_hip_test_bpr_prepare_chunk(gorse_mf *h, int64_t n, uint64_t seed, uint64_t epoch, int64_t sample_base,
                                                    int32_t *off /*U + 2*/, int32_t *si /*n*/, int32_t *sj /*n*/) {
    if (!h || !off || !si || !sj) return fail(GORSE_ERR_INVALID, "NULL argument");
    GORSE_TRY(h->use());
    GORSE_TRY(bpr_ensure_trip(h, n));
    if (n < 0 || n > (int64_t)h->trip_cap) return fail(GORSE_ERR_INVALID, "n outside one chunk (%zu samples)", h->trip_cap);
    // (whatever the library's default schedule: a handle whose shape takes user runs)
    if (bpr_schedule(MODE_ATOMIC, h->d, h->U, true, (g_bpr.variant & GORSE_TEST_BPR_USER_RUNS) != 0).schedule != kBprUserRuns)
        return fail(GORSE_ERR_INVALID, "this handle does not run the user-run schedule");
    GORSE_TRY(bpr_ensure_user_sort(h));
    GORSE_TRY(mf_sync_streams(h));
    const size_t cap = h->trip_cap;
    GORSE_TRY(bpr_launch_prepare_users(h, seed, epoch, sample_base, n, h->trip[0].p, h->sorted[0].p, h->ubucket[0].p, h->urank[0].p, cap,
                                       h->stream));
    GORSE_HIP_CHECK(hipMemcpyAsync(off, h->ubucket[0].p, (size_t)(h->U + 2) * 4, hipMemcpyDeviceToHost, h->stream));
    GORSE_HIP_CHECK(hipMemcpyAsync(si, h->sorted[0].p + cap, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
    GORSE_HIP_CHECK(hipMemcpyAsync(sj, h->sorted[0].p + 2 * cap, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
    GORSE_HIP_CHECK(hipStreamSynchronize(h->stream));
    return GORSE_OK;
}

extern "C" int32_t gorse_bpr_apply_triplets(gorse_mf *h, const int32_t *u, const int32_t *i, const int32_t *j, int64_t n,
                                            float lr, float reg, int32_t mode) {
    if (!h) return fail(GORSE_ERR_INVALID, "handle is NULL");
    if (n < 0 || (n > 0 && (!u || !i || !j))) return fail(GORSE_ERR_INVALID, "bad arguments");
    GORSE_TRY(check_mode(mode));
    if (n == 0) return GORSE_OK;
    for (int64_t s = 0; s < n; s++)
        if (u[s] >= h->U || i[s] >= h->I || j[s] >= h->I)
            return fail(GORSE_ERR_RANGE, "triplet %lld (%d,%d,%d) out of range", (long long)s, u[s], i[s], j[s]);
    GORSE_TRY(h->use());
    GORSE_TRY(bpr_ensure_trip(h, n));
    GORSE_TRY(mf_sync_streams(h));
    const BprSchedulePlan plan = schedule_of(h, mode);
    const int64_t cap = (int64_t)h->trip_cap;
    for (int64_t s0 = 0; s0 < n; s0 += cap) {
        const int64_t m = std::min(cap, n - s0);
        int32_t *tb = h->trip[0].p;
        GORSE_HIP_CHECK(hipMemcpyAsync(tb, u + s0, (size_t)m * 4, hipMemcpyHostToDevice, h->stream));
        GORSE_HIP_CHECK(hipMemcpyAsync(tb + cap, i + s0, (size_t)m * 4, hipMemcpyHostToDevice, h->stream));
        GORSE_HIP_CHECK(hipMemcpyAsync(tb + 2 * cap, j + s0, (size_t)m * 4, hipMemcpyHostToDevice, h->stream));
        if (plan.schedule == kBprSequential) {
            GORSE_TRY(run_sequential(h, tb, tb + cap, tb + 2 * cap, u + s0, i + s0, j + s0, m, lr, reg, g_bpr.exp_mode_exact,
                                     nullptr, nullptr));
        } else if (plan.schedule == kBprUserRuns) {
            GORSE_TRY(bpr_ensure_user_sort(h));
            GORSE_TRY(bpr_launch_user_sort(h, tb, h->sorted[0].p, h->ubucket[0].p, h->urank[0].p, m, (size_t)cap, h->stream));
            GORSE_TRY(bpr_launch_update_users(h, h->sorted[0].p, h->ubucket[0].p, (size_t)cap, lr, reg, g_bpr.exp_mode_exact, nullptr,
                                              h->stream, plan.kernel_mode == MODE_STORES));
            GORSE_HIP_CHECK(hipStreamSynchronize(h->stream));
        } else {
            GORSE_TRY(bpr_launch_update(h, plan.kernel_mode, tb, tb + cap, tb + 2 * cap, nullptr, 0, m, lr, reg, 0, nullptr, h->stream));
            GORSE_HIP_CHECK(hipStreamSynchronize(h->stream));
        }
    }
    return GORSE_OK;
}
