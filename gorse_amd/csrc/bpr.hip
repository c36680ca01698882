// bpr.hip -- BPR training step on gfx950.  Reference: model/cf/model.go:446-494.
//
// The sample stream itself -- which draws make sample s, in which order -- is stated once, in bpr_stream.hpp; every sampling and
// preparation kernel below composes its functions.
// Kernels per chunk of samples (the user-run schedule: the production Hogwild form for >= 4096 users and nFactors 8/16/32/64/128;
// launch_prepare_users runs the preparation AHEAD on its own stream, by user bins where the shape has them: see "the preparation
// by user BINS" below -- the form without bins is):
//   bpr_sample_user_kernel : model.go:452-458 -- sample s draws its USER from the counter-based Philox stream of sample s and
//                            takes its rank in that user's run.
//   scan + bpr_scatter_ids : counting sort of the chunk's SAMPLE IDS by user (the order in which a Hogwild epoch applies its
//                            samples is free: parallel.go:44-68).
//   bpr_sample_items_kernel: model.go:459-468 -- one thread per sorted position replays its sample's stream and draws the
//                            positive and the negative; (i, j) are written in sorted order.
//   bpr_update_user_kernel : model.go:469-488 -- one 16-lane group applies ALL samples of one user: p_u is loaded
//                            once, updated in registers and stored once; q_i / q_j are gathered ahead (64-byte
//                            contiguous segments per load) and updated with fp32 atomics (hot items through replica
//                            rows) -- or, the negative of a COLD item, by one write-through store of fma(t, lr, row).
// Other schedules:
//   bpr_sample_kernel      : model.go:449-468 -- one thread per sample draws the whole triplet (the same stream): the
//                            per-sample and sequential schedules, gorse_bpr_sample_triplets.
//   bpr_update_kernel      : the per-sample form (one group per sample, three rows updated in place): the
//                            sequential parity schedule, the racy diagnostic, and the Hogwild schedule of shapes
//                            with few users or another factor width.
// HBM-bound: algorithmic bytes per sample = 6*d*4 (three rows read + three written) + 12 (indices).
// Test switches: the six GORSE_TEST_BPR_* bits of include/gorse_hip_test.h choose between equivalent schedules and preparations;
// the chunk loop of epoch_impl has two forms, the product's and GORSE_TEST_BPR_STABLE_RANK's.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "bpr_bins.hpp"
#include "mf_internal.hpp"
#include <utility>

using namespace gorse;

namespace {

int g_variant = 0;  // GORSE_TEST_BPR_* switches of the tests (gorse_hip_test_set_variant); nothing of it reaches a kernel
constexpr int MODE_ATOMIC = GORSE_BPR_HOGWILD_ATOMIC;
constexpr int MODE_EXACT = GORSE_BPR_SEQUENTIAL;
constexpr int MODE_RACY = GORSE_BPR_HOGWILD_RACY;
constexpr int MODE_STORES = GORSE_BPR_HOGWILD_STORES;  // MODE_ATOMIC with the cold negatives by store (user-run schedule only)

// ---- sampling (the draws themselves: bpr_stream.hpp) ------------------------------------------
__global__ __launch_bounds__(256) void bpr_sample_kernel(int32_t U, int32_t I, const int64_t *__restrict__ uptr,
                                                         const int32_t *__restrict__ uidx,
                                                         const int32_t *__restrict__ usorted, uint64_t seed,
                                                         uint64_t epoch, int64_t sample_base, int64_t n,
                                                         int32_t *__restrict__ us, int32_t *__restrict__ is,
                                                         int32_t *__restrict__ js, int32_t *__restrict__ fail_count) {
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n; s += (int64_t)gridDim.x * blockDim.x) {
        Philox g;
        g.init(seed, epoch, (uint64_t)(sample_base + s));
        int32_t u = draw_user(g, U, uptr);
        int32_t pi = -1, nj = -1;
        if (u >= 0) {
            const int64_t beg = uptr[u], cnt = uptr[u + 1] - beg;
            pi = uidx[beg + g.int31n((int32_t)cnt)];
            nj = draw_negative(g, I, usorted + beg, cnt);
        }
        if (u < 0 || nj < 0) {
            atomicAdd(fail_count, 1);
            u = pi = nj = -1;
        }
        us[s] = u;
        is[s] = pi;
        js[s] = nj;
    }
}

// ---- sampling for the user-run schedule: user first, items by run -----------------------------
// The same triplets as bpr_sample_kernel (sample s = the Philox stream keyed by (seed, epoch, sample_base + s)), produced in two
// passes so that what is random about the memory accesses shrinks from ~13 cache lines per sample to ~3:
//   bpr_sample_user_kernel  : sample s draws its USER only (model.go:452-458; one look at the row pointers) and takes its
//                             arrival rank in that user's run (the count pass of the counting sort by user);
//   scan + bpr_scatter_ids  : position of sample s in the user-sorted order -> perm[position] = s, su[position] = its user
//                             (8 bytes scattered per sample instead of the whole triplet);
//   bpr_sample_items_kernel : one thread per SORTED position replays the stream of its sample up to the user draw (no memory:
//                             the first non-empty row drawn IS the user) and draws the positive and the negative
//                             (model.go:459-468) -- neighbouring threads hold samples of the same user, whose two item rows are
//                             read while they sit in the cache -- and writes (i, j) straight to the sorted position.
// A sample whose negative cannot be found (kMaxDraws rejections: a user holding nearly every item) keeps its place in the run
// with j = -1; bpr_update_user_kernel skips it.
__global__ __launch_bounds__(256) void bpr_sample_user_kernel(int32_t U, const int64_t *__restrict__ uptr, uint64_t seed,
                                                              uint64_t epoch, int64_t sample_base, int64_t n,
                                                              int32_t *__restrict__ key, int32_t *__restrict__ fail_count,
                                                              int32_t *__restrict__ bucket, int32_t *__restrict__ rank) {
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n; s += (int64_t)gridDim.x * blockDim.x) {
        const int32_t u = redraw_user(seed, epoch, (uint64_t)(sample_base + s), U, uptr);
        if (u < 0) atomicAdd(fail_count, 1);
        key[s] = u;
        rank[s] = atomicAdd(&bucket[u < 0 ? U : u], 1);
    }
}

__global__ __launch_bounds__(256) void bpr_scatter_ids_kernel(const int32_t *__restrict__ key, const int32_t *__restrict__ rank,
                                                              const int32_t *__restrict__ bucket, int64_t n, int32_t U,
                                                              int2 *__restrict__ pairs) {
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n; s += (int64_t)gridDim.x * blockDim.x) {
        const int32_t k = key[s] < 0 ? U : key[s];
        const int64_t pos = (int64_t)bucket[k] + rank[s];
        pairs[pos] = make_int2((int32_t)s, key[s]);  // (sample id, user) at the sorted position: one 8-byte store
    }
}

__global__ __launch_bounds__(256) void bpr_sample_items_kernel(int32_t U, int32_t I, const int64_t *__restrict__ uptr,
                                                               const int32_t *__restrict__ uidx,
                                                               const int32_t *__restrict__ usorted, uint64_t seed,
                                                               uint64_t epoch, int64_t sample_base, int64_t n,
                                                               const int2 *__restrict__ pairs, int32_t *__restrict__ si,
                                                               int32_t *__restrict__ sj, int32_t *__restrict__ fail_count) {
    // one thread per SORTED position: neighbouring threads hold samples of the same user, so the user's row pointers and its
    // two item rows are shared by the lanes of a wave (and by the waves that follow) while they sit in the cache
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
        const int2 pr = pairs[t];  // (sample id, user)
        const int32_t u = pr.y;
        if (u < 0) continue;  // no user could be drawn: the positions behind the last run, never read
        const int64_t rbeg = uptr[u];
        const int64_t cnt = uptr[u + 1] - rbeg;
        Philox g;
        g.init(seed, epoch, (uint64_t)(sample_base + pr.x));
        replay_user(g, U, u);
        int32_t pi = uidx[rbeg + g.int31n((int32_t)cnt)];
        const int32_t nj = draw_negative(g, I, usorted + rbeg, cnt);
        if (nj < 0) {
            atomicAdd(fail_count, 1);
            pi = -1;
        }
        si[t] = pi;
        sj[t] = nj;
    }
}

__global__ __launch_bounds__(256) void bpr_sample_items_batch_kernel(int32_t U, int32_t I, const int64_t *__restrict__ uptr,
                                                               const int32_t *__restrict__ uidx,
                                                               const int32_t *__restrict__ usorted, uint64_t seed,
                                                               uint64_t epoch, int64_t sample_base, int64_t n,
                                                               const int2 *__restrict__ pairs, int32_t *__restrict__ si,
                                                               int32_t *__restrict__ sj, int32_t *__restrict__ fail_count) {
    // bpr_sample_items_kernel with four positions per thread, in lock step: a sample is a chain of ~12 dependent loads (row pointers, the
    // positive, the binary search of the negative candidate in the sorted row); where the rows do not sit in the L2 (C3 shard: 12.5M
    // feedbacks) four chains per thread take 100 -> 81 us per 4M samples; where they do (S-ml1m) the one-sample kernel is the
    // faster one (37 against 47 us per million: more steps per wave, the redo of the samples whose first candidate is rejected).
    // The search is the same lower bound, one step of all four per round.
    constexpr int B = 4;
    const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
    for (int64_t tb = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; tb < n; tb += B * nthreads) {
        int32_t u[B], sid[B];
#pragma unroll
        for (int e = 0; e < B; e++) {
            const int64_t t = tb + e * nthreads;
            const int2 pr = t < n ? pairs[t] : make_int2(0, -1);  // (sample id, user)
            u[e] = pr.y;  // u < 0: no user could be drawn (the positions behind the last run, never read)
            sid[e] = pr.x;
        }
        int64_t rbeg[B];
        int32_t cnt[B];
#pragma unroll
        for (int e = 0; e < B; e++) {
            const int32_t uu = u[e] < 0 ? 0 : u[e];
            rbeg[e] = uptr[uu];
            cnt[e] = (int32_t)(uptr[uu + 1] - rbeg[e]);
            if (u[e] < 0 || cnt[e] <= 0) cnt[e] = 0;
        }
        int32_t pi[B], c[B];
#pragma unroll
        for (int e = 0; e < B; e++) {
            Philox g;
            g.init(seed, epoch, (uint64_t)(sample_base + sid[e]));
            // replay_user, inline: four independent chains per thread (and no draw at all for a position without a user)
            for (int k = 0; k < kMaxDraws; k++)
                if (cnt[e] == 0 || g.int31n(U) == u[e]) break;
            const int32_t r = g.int31n(cnt[e] > 0 ? cnt[e] : 1);
            c[e] = g.int31n(I);
            pi[e] = cnt[e] > 0 ? uidx[rbeg[e] + r] : -1;
        }
        int32_t lo[B], len[B];
#pragma unroll
        for (int e = 0; e < B; e++) lo[e] = 0, len[e] = cnt[e];
        while ((len[0] | len[1] | len[2] | len[3]) != 0) {  // (lengths are >= 0)
            int32_t v[B];
#pragma unroll
            for (int e = 0; e < B; e++) v[e] = len[e] > 0 ? usorted[rbeg[e] + lo[e] + (len[e] >> 1)] : 0;
#pragma unroll
            for (int e = 0; e < B; e++) {
                if (len[e] > 0) {
                    const int32_t half = len[e] >> 1;
                    if (v[e] < c[e]) {
                        lo[e] += half + 1;
                        len[e] -= half + 1;
                    } else {
                        len[e] = half;
                    }
                }
            }
        }
        int32_t at[B];
#pragma unroll
        for (int e = 0; e < B; e++) at[e] = lo[e] < cnt[e] ? usorted[rbeg[e] + lo[e]] : -1;
#pragma unroll
        for (int e = 0; e < B; e++) {
            const int64_t t = tb + e * nthreads;
            if (t >= n || u[e] < 0) continue;
            int32_t nj = c[e];
            if (at[e] == c[e])  // the candidate is one of the user's items: the rest of the draws, one at a time
                nj = redraw_negative(seed, epoch, (uint64_t)(sample_base + sid[e]), U, I, u[e], usorted + rbeg[e], cnt[e]);
            if (nj < 0) atomicAdd(fail_count, 1);
            si[t] = nj < 0 ? -1 : pi[e];
            sj[t] = nj;
        }
    }
}

// ---- the preparation by user BINS (round 5) ---------------------------------------------------
// What the three kernels above put on the memory side per sample -- one returning atomic on the user's counter and two 4-byte stores
// to random places of the sorted order, every 64-byte line of which is written in sixteen pieces by workgroups of different XCDs --
// is what the update kernel, which runs beside the preparation of the next chunk, is bound by (its item-row atomics).  The binned form
// sorts in two levels so that no global atomic and no lone store is left per sample:
//   bpr_bin_count_kernel   : a workgroup draws the users of one TILE of samples (as bpr_sample_user_kernel does), stores the keys and
//                            counts them per BIN (a range of 2^shift user ids) in LDS and writes its row of the tile x bin matrix;
//   bpr_bin_offsets_kernel : the matrix's columns -> prefix over the tiles, and the bins' totals;
//   bpr_bin_scatter_kernel : scans the bin totals (every workgroup for itself: < 8192 bins), adds its row of the matrix = its tile's
//                            place in every bin, and writes (sample id, user) there -- runs of a tile's samples of one bin, written
//                            by ONE workgroup, merge in its L2;
//   bpr_bin_finish_kernel  : a workgroup per bin does the rest in LDS -- the bin's pairs by user, the run offsets (bucket[] as the
//                            update kernel reads it), the item draws, equal positives of a run next to each other -- and writes
//                            (i, j) once: the form of the shapes whose bins fit it and whose rows sit in the L2s (S-ml1m);
//   bpr_bin_sort_kernel, bpr_sample_items[_batch]_kernel, bpr_group_positives_kernel: the same three steps through global memory,
//                            a launch each -- every other shape on the binned route (C3 shapes, the 10M-user set).
// See launch_prepare_users for which chunk takes which.
// The order of the samples inside a run is the order of arrival as before (no order is promised: the runs are multisets).
constexpr int kBinThreads = 512;     // workgroup of the count / scatter kernels
constexpr int kBinBatch = 8;         // samples of a thread whose loads are in flight together (scatter / sort kernels)

template <int NW>
__device__ __forceinline__ int32_t block_exclusive_scan(int32_t v, int32_t *lds /* NW + 1 */, int32_t *total) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int32_t x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        int32_t y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) lds[wid] = x;
    __syncthreads();
    int32_t base = 0, all = 0;
#pragma unroll
    for (int w = 0; w < NW; w++) {
        const int32_t t = lds[w];
        if (w < wid) base += t;
        all += t;
    }
    if (total) *total = all;
    __syncthreads();
    return base + x - v;
}

__global__ __launch_bounds__(kBinThreads) void bpr_bin_count_kernel(int32_t U, const int64_t *__restrict__ uptr, uint64_t seed,
                                                                    uint64_t epoch, int64_t sample_base, int64_t n, int64_t tile,
                                                                    int shift, int nbins, int32_t *__restrict__ key,
                                                                    int32_t *__restrict__ fail_count,
                                                                    int32_t *__restrict__ H) {
    __shared__ int32_t hist[kMaxBins];
    for (int b = threadIdx.x; b < nbins; b += kBinThreads) hist[b] = 0;
    __syncthreads();
    const int64_t s0 = (int64_t)blockIdx.x * tile, s1 = s0 + tile < n ? s0 + tile : n;
    // four samples per thread at a time: their first user draws' row pointers are in flight together (the draw that finds an
    // empty row -- rare -- goes on alone, same stream, same order of draws)
    constexpr int B = 4;
    for (int64_t sb = s0 + threadIdx.x; sb < s1; sb += B * kBinThreads) {
        int32_t cu[B];
        int64_t r0[B], r1[B];
#pragma unroll
        for (int e = 0; e < B; e++) {
            const int64_t s = sb + (int64_t)e * kBinThreads;
            Philox g;
            g.init(seed, epoch, (uint64_t)(sample_base + (s < s1 ? s : s0)));
            cu[e] = g.int31n(U);
            r0[e] = uptr[cu[e]];
            r1[e] = uptr[cu[e] + 1];
        }
#pragma unroll
        for (int e = 0; e < B; e++) {
            const int64_t s = sb + (int64_t)e * kBinThreads;
            if (s < s1) {
                int32_t u = r1[e] > r0[e] ? cu[e] : -1;
                if (u < 0) {  // the first draw met a user without feedback: the stream again from its start
                    u = redraw_user(seed, epoch, (uint64_t)(sample_base + s), U, uptr);
                    if (u < 0) atomicAdd(fail_count, 1);
                }
                key[s] = u;
                atomicAdd(&hist[(u < 0 ? U : u) >> shift], 1);
            }
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < nbins; b += kBinThreads) H[(int64_t)blockIdx.x * nbins + b] = hist[b];
}

// H[t][b] = tile t's count of bin b -> the exclusive prefix over the tiles, in place; bin_count[b] = the bin's total.  (The first form
// of the binned preparation reserved a tile's share of a bin with a returning atomic on the bin's cursor: a few hundred tiles on
// one address take ~0.4 us each, one after the other -- 88 us at S-ml1m, the whole gain.  r05_zd_bpr_serial_*.txt)
constexpr int kOffWaves = 16;
constexpr int kOffKeep = 16;  // tiles of a thread whose counts stay in registers
__global__ __launch_bounds__(kOffWaves * 64) void bpr_bin_offsets_kernel(int32_t *__restrict__ H, int tiles, int nbins,
                                                                         int32_t *__restrict__ bin_count) {
    __shared__ int32_t seg[kOffWaves][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int b = blockIdx.x * 64 + lane;
    const int per = (tiles + kOffWaves - 1) / kOffWaves, t0 = w * per, t1 = t0 + per < tiles ? t0 + per : tiles;
    // a share of at most kOffKeep tiles (S-ml1m: 243 tiles, 16 a thread) stays in registers between the two passes: one read of
    // the matrix, its loads in flight together
    const bool keep = per <= kOffKeep;
    int32_t held[kOffKeep];
    int32_t sum = 0;
    if (keep) {
#pragma unroll
        for (int e = 0; e < kOffKeep; e++) {
            held[e] = b < nbins && t0 + e < t1 ? H[(int64_t)(t0 + e) * nbins + b] : 0;
            sum += held[e];
        }
    } else if (b < nbins) {
        for (int t = t0; t < t1; t++) sum += H[(int64_t)t * nbins + b];
    }
    seg[w][lane] = sum;
    __syncthreads();
    int32_t run = 0, total = 0;
#pragma unroll
    for (int k = 0; k < kOffWaves; k++) {
        const int32_t v = seg[k][lane];
        if (k < w) run += v;
        total += v;
    }
    if (b < nbins) {
        if (keep) {
#pragma unroll
            for (int e = 0; e < kOffKeep; e++) {
                if (t0 + e < t1) H[(int64_t)(t0 + e) * nbins + b] = run;
                run += held[e];
            }
        } else {
            for (int t = t0; t < t1; t++) {
                const int32_t v = H[(int64_t)t * nbins + b];
                H[(int64_t)t * nbins + b] = run;
                run += v;
            }
        }
        if (w == 0) bin_count[b] = total;
    }
}

__global__ __launch_bounds__(kBinThreads) void bpr_bin_scatter_kernel(int32_t U, const int32_t *__restrict__ key, int64_t n, int64_t tile,
                                                                      int shift, int nbins, const int32_t *__restrict__ bin_count,
                                                                      const int32_t *__restrict__ H, int32_t *__restrict__ bin_start,
                                                                      int2 *__restrict__ bp) {
    __shared__ int32_t cur[kMaxBins];  // where this tile's next sample of a bin goes
    __shared__ int32_t wsum[kBinThreads / 64 + 1];
    constexpr int PER = kMaxBins / kBinThreads;  // bins per thread of the scan
    {
        // exclusive scan of the chunk's bin counts (every workgroup its own: < 8192 words); a bin's start + the counts of the tiles
        // in front of this one = this tile's place in the bin
        int32_t c[PER], v = 0;
#pragma unroll
        for (int e = 0; e < PER; e++) {
            const int b = threadIdx.x * PER + e;
            c[e] = b < nbins ? bin_count[b] : 0;
            v += c[e];
        }
        int32_t run = block_exclusive_scan<kBinThreads / 64>(v, wsum, nullptr);
#pragma unroll
        for (int e = 0; e < PER; e++) {
            const int b = threadIdx.x * PER + e;
            if (blockIdx.x == 0 && b <= nbins) bin_start[b] = run;  // bin_start[nbins] = n (nbins < kMaxBins)
            if (b < nbins) cur[b] = run + H[(int64_t)blockIdx.x * nbins + b];
            run += c[e];
        }
    }
    __syncthreads();
    // (eight keys per thread in flight: one load per iteration made the loop a chain of memory latencies -- 96 -> us per 4M samples)
    const int64_t s0 = (int64_t)blockIdx.x * tile, s1 = s0 + tile < n ? s0 + tile : n;
    for (int64_t sb = s0 + threadIdx.x; sb < s1; sb += kBinBatch * kBinThreads) {
        int32_t u[kBinBatch];
#pragma unroll
        for (int e = 0; e < kBinBatch; e++) {
            const int64_t s = sb + (int64_t)e * kBinThreads;
            u[e] = s < s1 ? key[s] : 0;
        }
#pragma unroll
        for (int e = 0; e < kBinBatch; e++) {
            const int64_t s = sb + (int64_t)e * kBinThreads;
            if (s < s1) {
                const int32_t pos = atomicAdd(&cur[(u[e] < 0 ? U : u[e]) >> shift], 1);
                bp[pos] = make_int2((int32_t)s, u[e]);  // (sample id, user): one 8-byte store
            }
        }
    }
}

// one bin: cnt[0 .. ub) <- where the runs of its users end (relative to b0), bucket[] <- where they begin, pairs[] <- the bin's
// (sample id, user) in run order.  The body of bpr_bin_sort_kernel, and of a workgroup of bpr_bin_finish_kernel that meets a bin
// larger than its LDS holds.
template <int NT>
__device__ __forceinline__ void bin_sort_body(int32_t U, int ub, int32_t ulo, int32_t b0, int32_t b1, const int2 *__restrict__ bp,
                                              int32_t *__restrict__ bucket, int2 *__restrict__ pairs, int32_t *cnt, int32_t *wsum) {
    for (int k = threadIdx.x; k < ub; k += NT) cnt[k] = 0;
    __syncthreads();
    for (int32_t eb = b0 + threadIdx.x; eb < b1; eb += kBinBatch * NT) {
        int32_t u[kBinBatch];
#pragma unroll
        for (int e = 0; e < kBinBatch; e++) u[e] = eb + e * NT < b1 ? bp[eb + e * NT].y : 0;
#pragma unroll
        for (int e = 0; e < kBinBatch; e++)
            if (eb + e * NT < b1) atomicAdd(&cnt[(u[e] < 0 ? U : u[e]) - ulo], 1);
    }
    __syncthreads();
    // exclusive scan of cnt[0 .. ub): eight counters per thread and round
    int32_t carry = 0;
    for (int k0 = 0; k0 < ub; k0 += 8 * NT) {
        int32_t c[8], v = 0;
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const int k = k0 + threadIdx.x * 8 + e;
            c[e] = k < ub ? cnt[k] : 0;
            v += c[e];
        }
        int32_t total;
        int32_t run = carry + block_exclusive_scan<NT / 64>(v, wsum, &total);
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const int k = k0 + threadIdx.x * 8 + e;
            if (k < ub) {
                cnt[k] = run;
                if (ulo + k <= U) bucket[ulo + k] = b0 + run;
                if (ulo + k == U) bucket[U + 1] = b1;
            }
            run += c[e];
        }
        carry += total;
    }
    __syncthreads();
    for (int32_t eb = b0 + threadIdx.x; eb < b1; eb += kBinBatch * NT) {
        int2 pr[kBinBatch];
#pragma unroll
        for (int e = 0; e < kBinBatch; e++) pr[e] = eb + e * NT < b1 ? bp[eb + e * NT] : make_int2(0, 0);
#pragma unroll
        for (int e = 0; e < kBinBatch; e++) {
            if (eb + e * NT < b1) {
                const int32_t p = b0 + atomicAdd(&cnt[(pr[e].y < 0 ? U : pr[e].y) - ulo], 1);
                pairs[p] = pr[e];
            }
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void bpr_bin_sort_kernel(int32_t U, int shift, int nbins, const int32_t *__restrict__ bin_start,
                                                           const int2 *__restrict__ bp, int32_t *__restrict__ bucket,
                                                           int2 *__restrict__ pairs) {
    __shared__ int32_t cnt[1 << kMaxBinShift];
    __shared__ int32_t wsum[5];
    for (int b = blockIdx.x; b < nbins; b += gridDim.x)  // keys ulo .. ulo + ub - 1 (key U = the samples without a user, sorted last)
        bin_sort_body<256>(U, 1 << shift, b << shift, bin_start[b], bin_start[b + 1], bp, bucket, pairs, cnt, wsum);
}

// ---- equal positives of a run next to each other ------------------------------------------------
// The last step of launch_prepare_users (both forms).  The positive of a sample is drawn with replacement from the user's n_u
// feedbacks and a run holds ~N / U samples whatever n_u, so about half the (user, positive) pairs of an S-ml1m epoch repeat one of
// the same run (distinct share 0.49; C3 shapes 0.63): bpr_update_user_kernel sends ONE atomic row update for a stretch of samples
// with the same positive, and this pass makes the repeats such stretches.  One wave per run sorts the run's (i, j) pairs in LDS
// (bitonic, 64-bit keys) and writes them back in place: 8 bytes read and written per sample in whole lines, no global atomic, no
// lone store -- nothing of what the update kernel beside it is sensitive to (see the binned preparation above).
// The key's upper half is not i but a per-user BIJECTION of i: sorted by i itself every group would walk the item ids upwards at
// the same pace, all 6040 of them inside the same narrow band of rows at any moment -- the rows' atomic queues and the staleness of
// a hot row's gathers are what the replicas and the fold period exist to bound.  With the salted order a positive's place in its
// run is uniform, as it was in arrival order.  The lower half is j: the order inside a run is a function of the run's multiset.
// A sample without a negative (i = j = -1) gets the largest key and ends up last in its run; runs longer than kGroupCap samples
// (a chunk is max(4M, 32 U) samples: more than 1024 per user only below 4096 users) stay in arrival order -- the update kernel
// combines what is adjacent, whatever put it there.
constexpr int kGroupCap = 1024;  // samples of a run the pass sorts: 8 KB of LDS per wave
constexpr uint32_t kGroupMul = 0x9E3779B1u;
constexpr uint32_t mul_inverse_u32(uint32_t m) {  // of an odd m, modulo 2^32 (Newton: five steps double 3 correct bits to 96)
    uint32_t x = m;
    for (int k = 0; k < 5; k++) x *= 2u - m * x;
    return x;
}
constexpr uint32_t kGroupMulInv = mul_inverse_u32(kGroupMul);
static_assert(kGroupMul * kGroupMulInv == 1u, "inverse of the mixing multiplier");
__device__ __forceinline__ uint32_t group_salt(int32_t u) { return (uint32_t)u * 0x85EBCA6Bu + 0x7F4A7C15u; }
__device__ __forceinline__ uint64_t group_key(int32_t i, int32_t j, uint32_t salt) {
    if (j < 0) return ~0ull;
    uint32_t x = ((uint32_t)i ^ salt) * kGroupMul;
    x ^= x >> 16;
    return ((uint64_t)x << 32) | (uint32_t)j;
}
__device__ __forceinline__ int2 group_unkey(uint64_t k, uint32_t salt) {
    const int32_t j = (int32_t)(uint32_t)k;
    if (j < 0) return make_int2(-1, -1);
    uint32_t x = (uint32_t)(k >> 32);
    x ^= x >> 16;
    return make_int2((int32_t)((x * kGroupMulInv) ^ salt), j);
}

// one run of 3 .. kGroupCap samples, by the NT threads of a workgroup: sorted in key[], written back in place
template <int NT>
__device__ __forceinline__ void group_run(uint64_t *key, int32_t beg, int32_t len, uint32_t salt, int32_t *si, int32_t *sj) {
    const int lane = threadIdx.x;
    int P = 4;
    while (P < len) P <<= 1;
    for (int k = lane; k < P; k += NT) key[k] = k < len ? group_key(si[beg + k], sj[beg + k], salt) : ~0ull;
    __syncthreads();
    for (int kk = 2; kk <= P; kk <<= 1) {
        for (int jj = kk >> 1; jj > 0; jj >>= 1) {
            for (int t = lane; t < (P >> 1); t += NT) {
                const int lo = ((t & ~(jj - 1)) << 1) | (t & (jj - 1)), hi = lo | jj;
                const uint64_t a = key[lo], b = key[hi];
                if ((a > b) == ((lo & kk) == 0)) key[lo] = b, key[hi] = a;
            }
            __syncthreads();
        }
    }
    // (the padding keys equal the key of a sample without a negative and decode to the same (-1, -1): the first `len` keys
    // are the run's samples whichever of the equal keys they are)
    for (int k = lane; k < len; k += NT) {
        const int2 v = group_unkey(key[k], salt);
        si[beg + k] = v.x;
        sj[beg + k] = v.y;
    }
    __syncthreads();
}

__global__ __launch_bounds__(64) void bpr_group_positives_kernel(int32_t U, const int32_t *__restrict__ off, int32_t *__restrict__ si,
                                                                 int32_t *__restrict__ sj) {
    __shared__ uint64_t key[kGroupCap];
    for (int32_t u = blockIdx.x; u < U; u += gridDim.x) {
        const int32_t beg = off[u], len = off[u + 1] - beg;
        if (len < 3 || len > kGroupCap) continue;  // (two samples are adjacent anyway)
        group_run<64>(key, beg, len, group_salt(u), si, sj);
    }
}

// ---- the per-bin finish: sort, item draws and grouping of a bin in ONE LDS-resident pass -------------------------------------------
// After bpr_bin_scatter_kernel every sample of a bin sits in one contiguous window of bp[], and one workgroup owns the bin.  What
// bpr_bin_sort_kernel, bpr_sample_items_kernel and bpr_group_positives_kernel do to that window through global memory -- pairs read
// twice and written, read again, (i, j) written, read and written again: 56 bytes per sample, three launches -- this kernel does
// in LDS: the pairs are read once, counted per user, scanned (bucket[] as before) and placed by run in key[]; a thread per sorted
// position replays its sample's stream exactly as bpr_sample_items_kernel does and leaves group_key(i, j, salt(u)) in place of the
// pair; a wave per run sorts the runs of 3 .. kGroupCap samples (in place: the bitonic network whose merges all point upwards, so
// that positions >= len act as +inf without being there) and decodes them; the window's (i, j) go out once, in whole lines.
// 16 bytes per sample of global traffic, no global atomic (a workgroup's failed draws: one), no lone store.
// The rows the draws look into: the bin's users are consecutive, so their rows are ONE range uptr[ulo] .. uptr[ulo + users] of
// uidx_sorted / uidx.  Where that range has at most kFinStage entries the workgroup copies uidx_sorted's into LDS and row_contains
// runs there (S-ml1m: 16 users, 2,630 entries on average, 5,426 at most); at half of that or less uidx's too.  Longer ranges (C3
// shapes: 128 users, ~12,800 entries) are read from global memory as bpr_sample_items_kernel reads them.
// Capacities: kFinCap samples (48 KB of keys) + kFinStage row entries (24 KB) + two words per user of the bin = 76 KB of LDS, two
// workgroups per CU.  The host sends a chunk here only where n / nbins <= 3/4 kFinCap (launch_prepare_users); a bin that holds
// more all the same (users with feedback in a narrow id range) is finished by its workgroup: sorted through global memory
// (bin_sort_body), drawn a slice of kFinCap positions at a time, its runs grouped in global memory (group_run).
constexpr int kFinThreads = 512;
constexpr int kFinCap = 6144;                      // samples of a bin at most
constexpr int kFinPer = kFinCap / kFinThreads;     // pairs a thread holds in registers between the count and the placement
constexpr int kFinStage = 6144;                    // row entries staged at most
constexpr int kFinShift = 9, kFinUsers = 1 << kFinShift;  // user ids per bin at most (one thread each in the scan)
#ifndef GORSE_BPR_STAGE_ROWS
#define GORSE_BPR_STAGE_ROWS 1  // A/B: 0 = the rows always from global memory
#endif
static_assert(kFinUsers <= kFinThreads && kFinCap >= kGroupCap && kFinCap % kFinThreads == 0, "geometry of bpr_bin_finish_kernel");

__device__ __forceinline__ void wave_lds_sync() {  // LDS written by a wave's lanes, read by others of the SAME wave
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ascending sort of k[0 .. len), len <= kGroupCap, by one wave
__device__ __forceinline__ void wave_sort_run(uint64_t *k, int len, int lane) {
    int P = 4;
    while (P < len) P <<= 1;
    for (int kk = 2; kk <= P; kk <<= 1) {
        for (int jj = kk >> 1; jj > 0; jj >>= 1) {
            for (int t = lane; t < (P >> 1); t += 64) {
                const int lo = ((t & ~(jj - 1)) << 1) | (t & (jj - 1));
                const int hi = jj == (kk >> 1) ? lo ^ (kk - 1) : lo | jj;  // (a merge's first step mirrors: every step sorts upwards)
                if (hi < len) {
                    const uint64_t a = k[lo], b = k[hi];
                    if (a > b) k[lo] = b, k[hi] = a;
                }
            }
            wave_lds_sync();
        }
    }
}

// A uniform value as a per-lane one.  Philox's ten round keys are sums of the seed's halves: of a uniform seed the compiler keeps all
// twenty in scalar registers across the draw loops, which bpr_bin_finish_kernel does not have (it spilled sixteen); of a per-lane
// seed they are twenty vector adds per block of four draws, next to its forty multiplies.
__device__ __forceinline__ uint64_t lane_copy(uint64_t x) {
    uint32_t lo, hi;
    asm("v_mov_b32 %0, %1" : "=v"(lo) : "s"((uint32_t)x));
    asm("v_mov_b32 %0, %1" : "=v"(hi) : "s"((uint32_t)(x >> 32)));
    return ((uint64_t)hi << 32) | lo;
}

__global__ __launch_bounds__(kFinThreads) void bpr_bin_finish_kernel(int32_t U, int32_t I, int shift, const int32_t *__restrict__ bin_start,
                                                                     const int2 *__restrict__ bp, const int64_t *__restrict__ uptr,
                                                                     const int32_t *__restrict__ uidx,
                                                                     const int32_t *__restrict__ usorted, uint64_t seed, uint64_t epoch,
                                                                     int64_t sample_base, int32_t *__restrict__ bucket,
                                                                     int2 *__restrict__ pairs, int32_t *__restrict__ si,
                                                                     int32_t *__restrict__ sj, int32_t *__restrict__ fail_count,
                                                                     int group) {
    __shared__ uint64_t key[kFinCap];         // (sample id, user) by run, then the group key of the sample's (i, j), then (i, j)
    __shared__ int32_t cnt[kFinUsers + 1];    // per user of the bin: samples, then where its run begins, then where it ends
    __shared__ int32_t rowoff[kFinUsers + 1]; // where the user's row begins in the bin's range of rows
    __shared__ int32_t rows[kFinStage];       // uidx_sorted's entries of the range (and uidx's behind them)
    __shared__ int32_t wsum[kFinThreads / 64 + 1];
    __shared__ int32_t nfail;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int ub = 1 << shift;
    const int32_t ulo = (int32_t)blockIdx.x << shift;  // keys ulo .. ulo + ub - 1 (key U = the samples without a user, sorted last)
    const int32_t b0 = bin_start[blockIdx.x], b1 = bin_start[blockIdx.x + 1], m = b1 - b0;
    const bool big = m > kFinCap;  // (the whole workgroup) more samples than key[] holds: see below
    // 1. the users' rows
    if (tid == 0) nfail = 0;
    const int64_t rbase = uptr[ulo];  // (ulo <= U)
    for (int k = tid; k <= ub; k += kFinThreads) {
        const int64_t uu = (int64_t)ulo + k < U ? (int64_t)ulo + k : U;
        rowoff[k] = (int32_t)(uptr[uu] - rbase);
    }
    __syncthreads();
    const int32_t range = rowoff[ub];  // entries of the users' rows together
    const bool staged = GORSE_BPR_STAGE_ROWS && m > 0 && range <= kFinStage, staged_idx = staged && 2 * range <= kFinStage;
    if (staged)
        for (int k = tid; k < range; k += kFinThreads) {
            rows[k] = usorted[rbase + k];
            if (staged_idx) rows[range + k] = uidx[rbase + k];
        }
    // 2. the samples per user -> the run offsets -> the pairs by run; every counter ends up at its run's end
    if (big) {
        bin_sort_body<kFinThreads>(U, ub, ulo, b0, b1, bp, bucket, pairs, cnt, wsum);  // (by run in pairs[], through global memory)
    } else {
        if (tid < ub) cnt[tid] = 0;
        __syncthreads();
        int2 pr[kFinPer];  // the bin's pairs, read once
#pragma unroll
        for (int e = 0; e < kFinPer; e++) {
            const int p = tid + e * kFinThreads;
            pr[e] = p < m ? bp[b0 + p] : make_int2(0, 0);
            if (p < m) atomicAdd(&cnt[(pr[e].y < 0 ? U : pr[e].y) - ulo], 1);
        }
        __syncthreads();
        const int32_t c = tid < ub ? cnt[tid] : 0;
        const int32_t run = block_exclusive_scan<kFinThreads / 64>(c, wsum, nullptr);
        if (tid < ub) {
            cnt[tid] = run;
            if (ulo + tid <= U) bucket[ulo + tid] = b0 + run;
            if (ulo + tid == U) bucket[U + 1] = b1;
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < kFinPer; e++) {
            if (tid + e * kFinThreads < m) {
                const int32_t q = atomicAdd(&cnt[(pr[e].y < 0 ? U : pr[e].y) - ulo], 1);
                key[q] = ((uint64_t)(uint32_t)pr[e].y << 32) | (uint32_t)pr[e].x;
            }
        }
        __syncthreads();
    }
    // (a bin within the capacity: one round)
    for (int32_t s0 = 0; s0 < m; s0 += kFinCap) {
        const int32_t ms = m - s0 < kFinCap ? m - s0 : kFinCap;
        if (big) {
            for (int p = tid; p < ms; p += kFinThreads) {
                const int2 pr = pairs[b0 + s0 + p];
                key[p] = ((uint64_t)(uint32_t)pr.y << 32) | (uint32_t)pr.x;
            }
            __syncthreads();
        }
        // 3. the item draws, a thread per sorted position (bpr_sample_items_kernel); the key of (i, j) takes the pair's place
        for (int p = tid; p < ms; p += kFinThreads) {
            const int32_t sid = (int32_t)(uint32_t)key[p], u = (int32_t)(key[p] >> 32);
            uint64_t out = ~0ull;  // a sample without a negative: what group_key gives it, and (-1, -1)
            if (u >= 0) {
                const int32_t ro = rowoff[u - ulo], n_u = rowoff[u - ulo + 1] - ro;
                Philox g;
                // (lane_copy: without it this kernel spills scalar registers -- tests/test_bpr_bin_finish_cpu.py is what says so)
                g.init(lane_copy(seed), epoch, (uint64_t)(sample_base + sid));
                replay_user(g, U, u);
                const int32_t r = g.int31n(n_u);
                const int32_t pi = staged_idx ? rows[range + ro + r] : uidx[rbase + ro + r];
                const int32_t nj = staged ? draw_negative(g, I, rows + ro, n_u) : draw_negative(g, I, usorted + rbase + ro, n_u);
                if (nj < 0)
                    atomicAdd(&nfail, 1);
                else
                    out = big ? ((uint64_t)(uint32_t)nj << 32) | (uint32_t)pi : group_key(pi, nj, group_salt(u));
            }
            key[p] = out;
        }
        __syncthreads();
        // 4. a wave per run: equal positives next to each other (bpr_group_positives_kernel's order), then (i, j) in the key's place
        if (!big) {
            for (int k = wid; k < ub; k += kFinThreads / 64) {
                const int32_t beg = k ? cnt[k - 1] : 0, len = cnt[k] - beg;
                const uint32_t salt = group_salt(ulo + k);
                if (group && len >= 3 && len <= kGroupCap && ulo + k < U) wave_sort_run(key + beg, len, lane);
                for (int t = lane; t < len; t += 64) {
                    const int2 v = group_unkey(key[beg + t], salt);
                    key[beg + t] = ((uint64_t)(uint32_t)v.y << 32) | (uint32_t)v.x;
                }
            }
            __syncthreads();
        }
        // 5. the window, once
        for (int p = tid; p < ms; p += kFinThreads) {
            si[b0 + s0 + p] = (int32_t)(uint32_t)key[p];
            sj[b0 + s0 + p] = (int32_t)(key[p] >> 32);
        }
        __syncthreads();
    }
    if (tid == 0 && nfail > 0) atomicAdd(fail_count, nfail);
    // a bin over the capacity went through key[] a slice at a time, the slices' (i, j) are in global memory: its runs are grouped
    // there, as bpr_group_positives_kernel does it, one after the other by the whole workgroup
    if (big && group)
        for (int k = 0; k < ub && ulo + k < U; k++) {
            const int32_t beg = k ? cnt[k - 1] : 0, len = cnt[k] - beg;
            if (len >= 3 && len <= kGroupCap) group_run<kFinThreads>(key, b0 + beg, len, group_salt(ulo + k), si, sj);
        }
}

// ---- memory access flavours ------------------------------------------------------------------
template <int MODE>
__device__ __forceinline__ float load_row(const float *p) {
    if (MODE == MODE_EXACT)
        return *p;
    else  // agent-scope load: served by L2 (never stale for written-back data), bypasses the CU's L1
        return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// row[e] <- fma(t, lr, snapshot) in the flavour of MODE
template <int MODE>
__device__ __forceinline__ void apply(float *p, float snap, float t, float lr, bool fused) {
    if constexpr (MODE == MODE_ATOMIC) {
        (void)snap;
        (void)fused;
        __hip_atomic_fetch_add(p, t * lr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
        float r = fused ? fmaf(t, lr, snap) : t * lr + snap;
        if constexpr (MODE == MODE_EXACT)
            *p = r;
        else  // write-through (sc1) store: visible to the other XCDs' L2s, like a CPU store
            __hip_atomic_store(p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__device__ __forceinline__ float bpr_exp(float x, int exp_mode) {
    return exp_mode == 1 ? exp_restated(x) : (exp_mode == 2 ? __expf(x) : expf(x));
}

// one element of the three updates of model.go:473-488 (operation order of SURVEY.md A2)
template <int MODE>
__device__ __forceinline__ void update_elem(float *pu, float *qi, float *qj, int e, float p, float a, float b, float grad,
                                            float nreg, float lr, bool fused, bool same_item) {
    float t1 = p * grad;
    t1 = fused ? fmaf(a, nreg, t1) : a * nreg + t1;
    float t2 = p * (-grad);
    t2 = fused ? fmaf(b, nreg, t2) : b * nreg + t2;
    float t3 = a - b;
    t3 = t3 * grad;
    t3 = fused ? fmaf(p, nreg, t3) : p * nreg + t3;
    if constexpr (MODE == MODE_EXACT) {
        float qi_new = fused ? fmaf(t1, lr, a) : t1 * lr + a;
        qi[e] = qi_new;
        // i == j cannot come out of the sampler; a hand-made stream applies both updates in order
        float base = same_item ? qi_new : b;
        qj[e] = fused ? fmaf(t2, lr, base) : t2 * lr + base;
        pu[e] = fused ? fmaf(t3, lr, p) : t3 * lr + p;
    } else {
        apply<MODE>(qi + e, a, t1, lr, fused);
        apply<MODE>(qj + e, b, t2, lr, fused);
        apply<MODE>(pu + e, p, t3, lr, fused);
    }
}

// Hot-row replicas (GORSE_BPR_HOGWILD_ATOMIC only).  Device-scope atomics and L1-bypassing loads are
// served memory-side, line by line, in order: a row that a popularity-skewed epoch keeps hitting builds a
// deep atomic queue, and every gather of that row -- and the retirement of every wave that updated it --
// waits in it (measured: positive-item atomics redirected away from the rows being read = 2.0x, spread
// over 8 rows each = 2.7x on S-ml1m; profiles/r01_b_probe_rep.txt).  So the positive-item update of a HOT
// item (share of the training feedback >= 1/8192, chosen at create time) -- and, in the user-run schedule, the update of a
// hot item drawn as the NEGATIVE -- lands in one of the item's R_s private rows picked by the group id (R_s = 1 .. kHotReplicas by the
// item's expected update rate, gorse_mf_create / hot_rows.hpp), and FOLDER workgroups of the same launch drain the replicas into the
// real rows with one combined atomic per element and pass, one pass per fold period of the device's constant-rate clock.  Q stays the
// only source of truth for every reader; a hot row's update becomes visible one folder pass (a fold period) late, the same order as the
// latency of the atomics themselves.  Once every worker workgroup has finished, the folders make a last pass: the launch leaves every
// replica zero and Q complete, so nothing outside bpr.hip ever sees them.
// The ACCUMULATED tier (hot_rows.hpp acc_rows_layout; handles whose whole Q fits one XCD's L2): every WARM item has one accumulator
// row behind the replica rows, and its hot_slot word is that row's code -- to the workers it is a hot item with one replica, so on
// such a handle no worker atomic lands on a row that anybody gathers (atomics onto rows under agent-scope loads run at 241 G dwords/s
// on a table of that size, onto rows nobody reads at 311: profiles/r04_s_probe_atomics3.txt).  The tier's slots follow the hot ones in
// items / meta (n_hot .. n_hot + n_acc) and have folder workgroups of their own, kFolderBlocksAcc of them behind the hot tier's, which
// pass every kDefaultAccFoldEvery-th fold period; the hot tier's folders and their period are what they are without the tier.  In the last
// pass all folder workgroups share the rows of both tiers.  That is the ATOMIC fold: the per-sample kernel's, a handle's without the
// tier, a launch's with the store route open.  A user-run launch on a handle with the tier and the store route closed has no worker
// that writes Q and folds in the SOLE-WRITER form (below kFolderTimeout): loads and stores instead of the exchange and the add.
constexpr int kHotReplicas = GORSE_HOT_REPLICAS;
constexpr int kFolderBlocks = 32;
// the tier's folders: 2,780 rows x 64 elements at C2 are 178 K (slot, element) pairs, 22 per thread of 32 workgroups and pass -- on
// the hot tier's 8,192 threads (11 pairs each today) they would not fit the period
constexpr int kFolderBlocksAcc = 32;
// Fold periods between two passes of the tier's folders.  A warm item takes at most 1/8192 + 1/I of the updates (3.9e-4 at C2), the
// hottest item 1.5e-2 and is folded every period: at 4 a warm row's window holds 3.9e-4 x 4 / 1.5e-2 ~ 1/10 of the stale updates the
// hottest item's window holds, and at nFactors 16 about 50 where the 32 us window that diverged (kDefaultFoldPeriod below) held ~1800.
// Swept on C2 (profiles/bpr_acc_rows_sweep.txt): 2 / 4 / 8 -> 0.393 / 0.389 / 0.384 ms per epoch at nFactors 64, 0.202 / 0.202 / 0.201
// at 16; NDCG@10 after 30 epochs stays within 0.006 of the sequential oracle at 2 and 4 and leaves the +-0.01 bar at 8 (nFactors 8, 16).
constexpr int kDefaultAccFoldEvery = 4;
int g_acc_fold_every = kDefaultAccFoldEvery;  // gorse_hip_test_set_bpr_acc_fold_every
// Wall-clock ticks (100 MHz) from the start of one folder pass to the next: how late a hot row's update reaches Q.  Swept on C2
// (profiles/r07_hr_sweep_replica_unit.txt, replica unit 0.001): 8 / 16 / 32 us -> 0.545 / 0.544 / 0.538 ms per epoch at nFactors 64,
// 0.295 / 0.293 ms at 16 -- where 32 us DIVERGED (non-finite factors within 23 epochs, three handles of three): the hottest item takes
// ~1.5 % of the updates, and at the small widths' sample rate a 32 us window holds ~1800 of them computed from one stale row.  8 us
// keeps a factor of four from that; it costs nothing measurable at nFactors 64.
constexpr uint32_t kDefaultFoldPeriod = 800;
uint32_t g_fold_period = kDefaultFoldPeriod;  // gorse_hip_test_set_bpr_fold_period
// folders that have waited this long (10 s) for the workers stop waiting (a launch of the largest chunk takes ~0.13 s): a last pass
// while workers still run leaves some updates in the replicas, where the next launch's folders find them -- never a hung device
constexpr uint64_t kFolderTimeout = 1000000000ull;
uint64_t g_folder_timeout = kFolderTimeout;  // gorse_hip_test_set_bpr_folder_timeout
// The SOLE-WRITER fold.  On a handle with the accumulated tier every item has a row, so in a user-run launch without the store route
// no worker instruction writes Q: the folders are the only writers of the Q rows they fold, and their atomics -- an exchange per row
// and an add onto Q per pass, the add the only atomic of the launch that lands on rows the workers gather -- are not needed.  Such a
// launch (launch_update_users decides: HotRows::sole) folds with loads and stores instead.  At its start every folder thread copies
// the Q elements it owns into `base` (a table of (n_hot + n_acc) x d floats of the handle's, private to bpr.hip); a periodic pass
// LOADS the slot's rows and stores Q <- base + their sum -- nothing is zeroed, the rows grow for the length of the launch -- and the
// last pass exchanges the rows with zero and stores Q <- base + the sum of what it took.  The exchange stays there on purpose: it
// leaves every row zero without a race, and after a last pass made while workers still run (the timeout) whatever lands behind it
// stays in the row, where the next launch -- which starts from base = Q -- finds it.  What makes the stores safe is ownership: every
// (slot, element group) belongs to ONE thread for the whole launch, periodic and last pass alike (hot_rows.hpp fold_share), so no
// workgroup still in a periodic pass can overwrite another's final value.  Q = base + (the launch's updates of the row) is one of the
// associations a Hogwild launch produces anyway, and with one update per row the bits of the atomic form.  Every other launch -- a
// handle without the tier, the store route, the per-sample kernel -- keeps the atomic fold below.
#ifndef GORSE_BPR_FOLD_SOLE_WRITER
#define GORSE_BPR_FOLD_SOLE_WRITER 1  // A/B: 0 = every launch folds with atomics
#endif

struct HotRows {
    const int32_t *slot;   // I entries: class of an item -- hot_code(first replica row, log2 R_s) of a HOT item, hot_code(its row, 0)
                           // of an item of the accumulated tier, -1 warm, -2 cold
    const int32_t *items;  // n_hot + n_acc entries: item of a slot (the hot slots first)
    const int32_t *meta;   // n_hot + n_acc entries: hot_code of a slot
    float *rep;            // replica rows, then the tier's rows, of d floats: all zero outside an update launch
    int32_t *done;         // two sets of arrival stripes (worker workgroups that have finished) + the folders' pass count
    int n_hot;
    int d;
    int set;               // the set of stripes this launch counts in (launch parity: the launch zeroes the other one for the next)
    uint32_t period;       // wall-clock ticks between two folder passes
    int n_acc;             // slots of the accumulated tier (0: the handle has none)
    int acc_every;         // fold periods between two passes of the tier's folders
    float *base;           // n_hot + n_acc rows of d floats: Q's rows of the slots as the launch found them (the sole-writer fold)
    int sole;              // the launch folds as Q's sole writer (launch_update_users)
    uint64_t timeout;      // wall-clock ticks after which the folders stop waiting for the workers
};

// a group of the sole-writer fold (kFoldGroup = 2 floats, 8-byte aligned: d and the element are even): agent-scope load, store and
// exchange with zero, the flavours the gathers and the cold-store route use across XCDs; the exchange per element, so that it meets
// the workers' fp32 adds as the atomic fold's does
static_assert(kFoldGroup == 2 && kFolderThreads == kBlock, "the sole-writer fold moves float pairs, one per thread of an update workgroup");
__device__ __forceinline__ float2 load_pair(const float *p) {
    const unsigned long long x = __hip_atomic_load((const unsigned long long *)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return make_float2(__uint_as_float((unsigned)x), __uint_as_float((unsigned)(x >> 32)));
}
__device__ __forceinline__ void store_pair(float *p, float2 v) {
    __hip_atomic_store((unsigned long long *)p, (unsigned long long)__float_as_uint(v.x) | ((unsigned long long)__float_as_uint(v.y) << 32),
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ float2 drain_pair(float *p) {
    const float x = __hip_atomic_exchange(p, 0.0f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const float y = __hip_atomic_exchange(p + 1, 0.0f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return make_float2(x, y);
}

// the replica row that group `group` adds a hot item's update to (code: the item's hot_slot word)
__device__ __forceinline__ float *hot_row(const HotRows &hot, int32_t code, int64_t group) {
    return hot.rep + (hot_base(code) + (group & ((1 << hot_lg(code)) - 1))) * hot.d;
}

// The arrival counter of the worker workgroups, in kDoneStripes words 256 bytes apart: one 64-byte line serves 88 M atomics/s
// (scripts/probe_atomics4.hip), and the per-sample kernel's 4096 workgroups, which all finish within a few microseconds of each other,
// queued 46 us on a single word at the end of every launch (S-ml100k: a third of the kernel).
constexpr int kDoneStripes = GORSE_HOT_DONE_STRIPES, kDoneStride = GORSE_HOT_DONE_STRIDE;
constexpr int kFoldPassesWord = 2 * kDoneStripes * kDoneStride;  // hot.done[]: the last launch's folder passes (gorse_hip_test_bpr_fold_stats)
__device__ __forceinline__ int32_t *done_set(const HotRows &hot, int set) { return hot.done + set * kDoneStripes * kDoneStride; }
// The end of a worker workgroup (every thread calls it).  LAST: the launch's folders make the last pass themselves, once every worker
// is counted -- so the workgroup's atomics on the replicas are performed, and released at agent scope, before it is counted.  Without
// LAST (the per-sample kernel: bpr_fold_kernel follows its launch) the count only ends the folders' passes and needs no order; there a
// release in each of the up to 4096 short-lived workgroups cost more than the fold kernel it saves (S-ml100k: update kernel 52 -> 126
// us, and the sampler beside it 56 -> 124 us: each agent-scope release writes back the XCD's L2, which the sampler's stores fill;
// profiles/r07_hr_full_ab.txt, session A).
template <bool LAST>
__device__ __forceinline__ void worker_done(const HotRows &hot) {
    if constexpr (LAST) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        if constexpr (LAST) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __hip_atomic_fetch_add(done_set(hot, hot.set) + (blockIdx.x & (kDoneStripes - 1)) * kDoneStride, 1, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
    }
}
__device__ __forceinline__ bool workers_done(const HotRows &hot, int workers) {  // (called by whole waves)
    const int lane = threadIdx.x & 63;
    const int32_t *c = done_set(hot, hot.set);
    int v = lane < kDoneStripes ? __hip_atomic_load(c + lane * kDoneStride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v >= workers;
}

// one folder pass: (slot, element) pairs strided over the folder threads; each exchanges the slot's R_s rows and adds their sum once
// (slots [s0, s1): the hot tier's are [0, n_hot))
__device__ __forceinline__ void fold_pass(const HotRows &hot, float *Q, int s0, int s1, int64_t tid, int64_t nthreads) {
    const int d = hot.d;
    const int64_t work = (int64_t)(s1 - s0) * d;
    for (int64_t w = tid; w < work; w += nthreads) {
        const int64_t slot = s0 + w / d;
        const int e = (int)(w - (slot - s0) * d);
        const int32_t code = hot.meta[slot];
        const int nr = 1 << hot_lg(code);
        float *r0 = hot.rep + hot_base(code) * d + e;
        float v[kHotReplicas];
#pragma unroll
        for (int r = 0; r < kHotReplicas; r++)
            v[r] = r < nr ? __hip_atomic_exchange(r0 + (int64_t)r * d, 0.0f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0f;
        float sum = 0.0f;
#pragma unroll
        for (int r = 0; r < kHotReplicas; r++) sum += v[r];
        if (sum != 0.0f)
            __hip_atomic_fetch_add(Q + (int64_t)hot.items[slot] * d + e, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// one pass over slots [s0, s1) of the accumulated tier (one row each): kAccBatch exchanges of a thread are in flight before the first
// add that depends on one -- the tier's pass is a few times the hot tier's, and a chain of exchange -> add round trips per pair is
// what its last pass, at the end of the launch, cannot afford
constexpr int kAccBatch = 4;
__device__ __forceinline__ void fold_acc_pass(const HotRows &hot, float *Q, int s0, int s1, int tid, int nthreads) {
    const int d = hot.d;
    const int work = (s1 - s0) * d;  // (at most 4 MiB / 4 pairs: hot_rows.hpp kAccTableBytes)
    for (int wb = tid; wb < work; wb += kAccBatch * nthreads) {
        float v[kAccBatch];
        float *q[kAccBatch];
#pragma unroll
        for (int b = 0; b < kAccBatch; b++) {
            const int w = wb + b * nthreads;
            v[b] = 0.0f;
            q[b] = Q;
            if (w < work) {
                const int slot = s0 + w / d;
                const int e = w - (slot - s0) * d;
                q[b] = Q + (int64_t)hot.items[slot] * d + e;
                v[b] = __hip_atomic_exchange(hot.rep + hot_base(hot.meta[slot]) * d + e, 0.0f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
#pragma unroll
        for (int b = 0; b < kAccBatch; b++)
            if (v[b] != 0.0f) __hip_atomic_fetch_add(q[b], v[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// The sole-writer fold (above HotRows).  sh: this thread's share of its tier (hot_rows.hpp fold_share).
// launch start: base <- Q for the groups this thread owns -- nobody else writes these elements of Q during the launch
__device__ __forceinline__ void fold_sole_begin(const HotRows &hot, const float *Q, const FoldShare &sh) {
    const int d = hot.d, groups = fold_groups(sh, d);
    for (int g = sh.tid; g < groups; g += sh.nthreads) {
        const int slot = fold_group_slot(sh, g, d), e = fold_group_elem(g, d);
        *(float2 *)(hot.base + (int64_t)slot * d + e) = load_pair(Q + (int64_t)hot.items[slot] * d + e);
    }
}
// one pass over the groups this thread owns: Q <- base + the sum of the slot's rows (at most ROWS of them: kHotReplicas in the hot
// tier, 1 in the accumulated tier), the rows loaded in a periodic pass and exchanged with zero in the LAST.  BATCH groups a time, their
// rows kFoldRowsAtOnce a time: all those loads or exchanges are in flight before the first instruction that depends on one.  Two
// pairs in either tier: with more, the folders and not the workers set the register count of the nFactors 8 / 16 kernels (64 -> 72
// VGPRs at 4 pairs of the accumulated tier), which is the workers' occupancy on every handle.
constexpr int kFoldRowsAtOnce = 2;
template <bool LAST, int ROWS, int BATCH>
__device__ __forceinline__ void fold_sole_pass(const HotRows &hot, float *Q, const FoldShare &sh) {
    constexpr int RC = ROWS < kFoldRowsAtOnce ? ROWS : kFoldRowsAtOnce;
    const int d = hot.d, groups = fold_groups(sh, d);
    for (int gb = sh.tid; gb < groups; gb += BATCH * sh.nthreads) {
        float2 sum[BATCH];
        int at[BATCH];  // slot * d + element of the group, < 0 = none
#pragma unroll
        for (int b = 0; b < BATCH; b++) {
            const int g = gb + b * sh.nthreads;
            at[b] = g < groups ? fold_group_slot(sh, g, d) * d + fold_group_elem(g, d) : -1;
            sum[b] = make_float2(0.0f, 0.0f);
        }
#pragma unroll
        for (int rc = 0; rc < ROWS; rc += RC) {
            float2 v[BATCH][RC];
#pragma unroll
            for (int b = 0; b < BATCH; b++) {
#pragma unroll
                for (int r = 0; r < RC; r++) v[b][r] = make_float2(0.0f, 0.0f);
                if (at[b] >= 0) {
                    const int32_t code = hot.meta[at[b] / d];
                    const int nr = 1 << hot_lg(code);
                    float *r0 = hot.rep + hot_base(code) * d + at[b] % d;
#pragma unroll
                    for (int r = 0; r < RC; r++)
                        if (rc + r < nr) v[b][r] = LAST ? drain_pair(r0 + (int64_t)(rc + r) * d) : load_pair(r0 + (int64_t)(rc + r) * d);
                }
            }
#pragma unroll
            for (int b = 0; b < BATCH; b++)
#pragma unroll
                for (int r = 0; r < RC; r++) sum[b].x += v[b][r].x, sum[b].y += v[b][r].y;  // (row after row, as the atomic fold sums)
        }
#pragma unroll
        for (int b = 0; b < BATCH; b++)
            if (at[b] >= 0) {
                const float2 base = *(const float2 *)(hot.base + at[b]);
                // (a select, not a skipped store: an element nothing was added to keeps its bits, a -0.0 included)
                store_pair(Q + (int64_t)hot.items[at[b] / d] * d + at[b] % d,
                           make_float2(sum[b].x != 0.0f ? base.x + sum[b].x : base.x, sum[b].y != 0.0f ? base.y + sum[b].y : base.y));
            }
    }
}

// The folder workgroups (blockIdx.x < folders) of an update launch: the hot tier's kFolderBlocks first, then -- on a handle with the
// accumulated tier -- the tier's own.  Wave 0 polls the workers' arrival count at the grain of one load round trip and decides for the
// workgroup: a pass over its tier when its period has run out (the hot tier's: the fold period; the accumulated tier's: acc_every of
// them), and once every worker has finished, with LAST, the last pass (an agent-scope acquire behind the count the workers released
// into), in which all folder workgroups share the rows of both tiers.  So the end of the launch never waits for a folder's sleep, and
// with LAST no fold kernel follows the launch.  Both kinds wait in the same loop, under the same bound (kFolderTimeout).
// A launch in the sole-writer form (hot.sole, above HotRows) waits and decides in the same way and differs in what a pass does: every
// thread works on its own share of its own tier's slots in every pass, the last included -- each workgroup decides for itself when
// its last pass begins, so a row shared out differently in that pass could be stored final by one workgroup and stale by another.
template <bool LAST>
__device__ void run_folders(const HotRows &hot, float *Q, int folders) {
    __shared__ int go;
    const int workers = (int)gridDim.x - folders;
    const int hotf = folders < kFolderBlocks ? folders : kFolderBlocks;  // the hot tier's workgroups
    const bool acc = (int)blockIdx.x >= hotf;                            // this workgroup serves the accumulated tier
    const int n_all = hot.n_hot + hot.n_acc;
    const uint64_t period = acc ? (uint64_t)hot.period * (uint64_t)hot.acc_every : hot.period;
    if (blockIdx.x == 0 && threadIdx.x < kDoneStripes)  // the stripes the launch before this one counted in: zero for the next launch
        __hip_atomic_store(done_set(hot, hot.set ^ 1) + threadIdx.x * kDoneStride, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // the sole-writer form: this thread's share of its tier's slots, the same in every pass of the launch; base <- Q first
    bool sole = false;
    FoldShare sh{};
    if constexpr (LAST && GORSE_BPR_FOLD_SOLE_WRITER) {
        sole = hot.sole != 0;
        sh = fold_share((int)blockIdx.x, (int)threadIdx.x, hot.n_hot, hot.n_acc, folders, kFolderBlocks);
        if (sole) fold_sole_begin(hot, Q, sh);
    }
    const uint64_t t0 = wall_clock64();
    uint64_t next = t0 + period;
    int passes = 0;
    for (;;) {
        if (threadIdx.x < 64) {
            const bool all = workers_done(hot, workers);
            if (threadIdx.x == 0) {
                const uint64_t now = wall_clock64();
                int g = 0;
                if (all || now - t0 > hot.timeout) {
                    if constexpr (LAST) {
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    }
                    g = 2;
                } else if (now >= next) {
                    next = now + period;
                    g = 1;
                }
                go = g;
            }
        }
        __syncthreads();
        const int g = go;
        __syncthreads();
        if (g == 0) continue;
        if (g == 2 && !LAST) break;
        // a periodic pass (g == 1): this workgroup's tier among the workgroups of its kind; the last pass (g == 2): both tiers among all
        const bool last = g == 2;
        if (sole) {  // both passes over this thread's own share: hot tier one group a time, the other tier two
            if constexpr (LAST && GORSE_BPR_FOLD_SOLE_WRITER) {
                if (!acc) {
                    if (last)
                        fold_sole_pass<true, kHotReplicas, 1>(hot, Q, sh);
                    else
                        fold_sole_pass<false, kHotReplicas, 1>(hot, Q, sh);
                } else {
                    if (last)
                        fold_sole_pass<true, 1, 2>(hot, Q, sh);
                    else
                        fold_sole_pass<false, 1, 2>(hot, Q, sh);
                }
            }
        } else {
            const int first = last || !acc ? 0 : hotf, among = last ? folders : (acc ? folders - hotf : hotf);
            const int tid = ((int)blockIdx.x - first) * (int)blockDim.x + (int)threadIdx.x, nthreads = among * (int)blockDim.x;
            if (last || !acc) fold_pass(hot, Q, 0, hot.n_hot, tid, nthreads);
            if (last || acc) fold_acc_pass(hot, Q, hot.n_hot, n_all, tid, nthreads);
        }
        passes++;
        if (last) break;
    }
    // the pass counts of the launch (gorse_hip_test_bpr_fold_stats): the hot tier's first workgroup and the accumulated tier's first
    if (threadIdx.x == 0 && ((int)blockIdx.x == 0 || (int)blockIdx.x == hotf)) hot.done[kFoldPassesWord + (acc ? 1 : 0)] = passes;
}

template <int NC, int MODE>
__global__ __launch_bounds__(kBlock) void bpr_update_kernel(float *P, float *Q, const int32_t *__restrict__ us,
                                                            const int32_t *__restrict__ is,
                                                            const int32_t *__restrict__ js,
                                                            const int32_t *__restrict__ order, int64_t begin,
                                                            int64_t end, int d, float lr, float reg, int exp_mode,
                                                            double *loss, HotRows hot, int folders) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    if (MODE == MODE_ATOMIC && (int)blockIdx.x < folders) {
        run_folders<false>(hot, Q, folders);
        return;
    }
    const int lane = threadIdx.x & (kGroup - 1);
    const int gib = threadIdx.x / kGroup;
    const int64_t group = (int64_t)((int)blockIdx.x - folders) * kGroupsPerBlock + gib;
    const int64_t ngroups = (int64_t)((int)gridDim.x - folders) * kGroupsPerBlock;
    const VecShape vs(d);
    const float nreg = -reg;
    double my_loss = 0.0;
    for (int64_t s = begin + group; s < end; s += ngroups) {
        const int64_t t = order ? (int64_t)order[s] : s;
        const int u = us[t], i = is[t], j = js[t];
        if ((u | i | j) < 0) continue;
        float *pu = P + (int64_t)u * d, *qi = Q + (int64_t)i * d, *qj = Q + (int64_t)j * d;
        float *qiw = qi;  // where the positive item's update lands
        if (MODE == MODE_ATOMIC && folders > 0) {  // (a launch has folders where it has rows that take an item's updates: open_hot)
            const int32_t code = hot.slot[i];
            if (code >= 0) qiw = hot_row(hot, code, group);
        }
        if constexpr (NC > 0) {
            float p[NC], a[NC], b[NC];
#pragma unroll
            for (int c = 0; c < NC; c++) {
                p[c] = load_row<MODE>(pu + 16 * c + lane);
                a[c] = load_row<MODE>(qi + 16 * c + lane);
                b[c] = load_row<MODE>(qj + 16 * c + lane);
            }
            const float diff = dot512_regs<NC>(p, a) - dot512_regs<NC>(p, b);
            const float ex = bpr_exp(-diff, exp_mode);
            const float grad = ex / (1.0f + ex);
            if (loss && lane == 0) my_loss += (double)log1pf(ex);
#pragma unroll
            for (int c = 0; c < NC; c++)
                update_elem<MODE>(pu, qiw, qj, 16 * c + lane, p[c], a[c], b[c], grad, nreg, lr, true, i == j);
        } else {
            float *sp = smem + (size_t)gib * 3 * d, *sa = sp + d, *sb = sa + d;
            for (int e = lane; e < d; e += kGroup) {
                sp[e] = load_row<MODE>(pu + e);
                sa[e] = load_row<MODE>(qi + e);
                sb[e] = load_row<MODE>(qj + e);
            }
            __builtin_amdgcn_wave_barrier();
            const float diff = dot512_lds(sp, sa, vs, lane) - dot512_lds(sp, sb, vs, lane);
            const float ex = bpr_exp(-diff, exp_mode);
            const float grad = ex / (1.0f + ex);
            if (loss && lane == 0) my_loss += (double)log1pf(ex);
            for (int e = lane; e < d; e += kGroup)
                update_elem<MODE>(pu, qiw, qj, e, sp[e], sa[e], sb[e], grad, nreg, lr, !vs.unfused(e), i == j);
            __builtin_amdgcn_wave_barrier();
        }
    }
    if (loss && lane == 0 && my_loss != 0.0) atomicAdd(loss, my_loss);
    if (MODE == MODE_ATOMIC && folders > 0) worker_done<false>(hot);
}

// after a per-sample update launch: Q[item] += the sum of its replicas, replicas <- 0 (nothing else runs on the stream); the slots
// of both tiers
__global__ __launch_bounds__(256) void bpr_fold_kernel(HotRows hot, float *Q) {
    const int d = hot.d;
    const int64_t work = (int64_t)(hot.n_hot + hot.n_acc) * d;
    for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < work; w += (int64_t)gridDim.x * blockDim.x) {
        const int64_t slot = w / d;
        const int e = (int)(w - slot * d);
        const int32_t code = hot.meta[slot];
        float *r0 = hot.rep + hot_base(code) * d + e;
        float sum = 0.0f;
        for (int r = 0; r < (1 << hot_lg(code)); r++) {
            sum += r0[(int64_t)r * d];
            r0[(int64_t)r * d] = 0.0f;
        }
        if (sum != 0.0f) Q[(int64_t)hot.items[slot] * d + e] += sum;
    }
}

// ---- counting sort by user ---------------------------------------------------------------------
constexpr int kScanTile = 2048;  // elements per workgroup of the scan (256 threads x 8)

// first pass of the counting sort of whole triplets (launch_user_sort: gorse_bpr_apply_triplets, GORSE_TEST_BPR_STABLE_RANK):
// rank[s] = arrival rank of sample s among the samples of its key; keys < 0 (skipped samples) count under key K
__global__ __launch_bounds__(256) void bpr_rank_kernel(const int32_t *__restrict__ key, int64_t n, int32_t K,
                                                       int32_t *__restrict__ bucket, int32_t *__restrict__ rank) {
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n; s += (int64_t)gridDim.x * blockDim.x)
        rank[s] = atomicAdd(&bucket[key[s] < 0 ? K : key[s]], 1);
}

// exclusive scan of data[0..m) in place, three launches: tile sums, scan of the tile sums, tile rescans
__device__ __forceinline__ int32_t block_exclusive_scan_256(int32_t v, int32_t *lds, int32_t *total) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int32_t x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        int32_t y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) lds[wid] = x;
    __syncthreads();
    int32_t base = 0;
    for (int w = 0; w < wid; w++) base += lds[w];
    if (total) *total = lds[0] + lds[1] + lds[2] + lds[3];
    __syncthreads();
    return base + x - v;
}

__global__ __launch_bounds__(256) void scan_tile_sums_kernel(const int32_t *__restrict__ data, int64_t m,
                                                             int32_t *__restrict__ sums) {
    __shared__ int32_t lds[4];
    const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * 8;
    int32_t v = 0;
#pragma unroll
    for (int e = 0; e < 8; e++)
        if (base + e < m) v += data[base + e];
    int32_t total;
    (void)block_exclusive_scan_256(v, lds, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void scan_sums_kernel(int32_t *__restrict__ sums, int64_t nt) {
    __shared__ int32_t lds[4];
    int32_t carry = 0;
    for (int64_t t0 = 0; t0 < nt; t0 += 256) {
        const int64_t t = t0 + threadIdx.x;
        const int32_t v = t < nt ? sums[t] : 0;
        int32_t total;
        const int32_t ex = block_exclusive_scan_256(v, lds, &total);
        if (t < nt) sums[t] = carry + ex;
        carry += total;
    }
}

__global__ __launch_bounds__(256) void scan_apply_kernel(int32_t *__restrict__ data, int64_t m,
                                                         const int32_t *__restrict__ sums) {
    __shared__ int32_t lds[4];
    const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * 8;
    int32_t x[8], v = 0;
#pragma unroll
    for (int e = 0; e < 8; e++) {
        x[e] = base + e < m ? data[base + e] : 0;
        v += x[e];
    }
    int32_t run = sums[blockIdx.x] + block_exclusive_scan_256(v, lds, nullptr);
#pragma unroll
    for (int e = 0; e < 8; e++) {
        if (base + e < m) data[base + e] = run;
        run += x[e];
    }
}


// scatter by an arbitrary key array (one window): keys < 0 sort behind every real key
__global__ __launch_bounds__(256) void bpr_scatter_by_kernel(const int32_t *__restrict__ key, const int32_t *__restrict__ us,
                                                             const int32_t *__restrict__ is, const int32_t *__restrict__ js,
                                                             int64_t n, int32_t K, const int32_t *__restrict__ bucket,
                                                             const int32_t *__restrict__ rank, int32_t *__restrict__ su,
                                                             int32_t *__restrict__ si, int32_t *__restrict__ sj) {
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n; s += (int64_t)gridDim.x * blockDim.x) {
        const int32_t kk = key[s] < 0 ? K : key[s];
        const int64_t pos = (int64_t)bucket[kk] + rank[s];
        su[pos] = us[s];
        si[pos] = is[s];
        sj[pos] = js[s];
    }
}

// ---- user-run schedule ---------------------------------------------------------------------------
// The chunk's triplets are counting-sorted by USER (the order in which a Hogwild epoch applies its samples is free:
// parallel.go:44-68) and one 16-lane group walks ALL samples of one user: p_u is loaded once, updated in registers
// sample after sample -- exact sequential SGD on the user side, no lost or delayed update -- and stored once, so a
// third of the fp32 atomics (the unit this kernel is bound by: ~1 dword/clk per L2 channel) and a third of the
// gathers disappear.  q_i / q_j are gathered two samples (q_j with the store route: one) ahead of the arithmetic and updated
// with atomics as in bpr_update_kernel (hot items through the replicas).  Users are drawn uniformly (model.go:452-458), so
// the runs are Poisson(N / U)-sized: balanced without any work splitting.
// POSITIVE SERIES.  A series is a maximal stretch of consecutive valid samples of a run with the same positive i (the preparation
// puts a run's repeats of a positive next to each other: bpr_group_positives_kernel; the kernel combines whatever is adjacent).
// Its first sample computes from the gathered snapshot as every sample did before; after each sample the group's own copy of the
// row becomes mad(t1, lr, a), the next sample of the series computes from that copy -- the operands of the sequential code, not a
// snapshot two samples stale -- and its row is not gathered at all; t1 * lr adds up in registers and goes out as ONE atomic per
// element when the series ends: the next positive differs, the next sample is invalid, the run ends, or one of the two samples has
// the series' positive as its NEGATIVE (hand-made streams; i == j included): such a sample's negative-side update then never meets a
// row with a change pending, nothing is lost or counted twice.  A series of one sample issues exactly the atomic of t1 * lr it
// always did.  The sum goes out in the iteration of the series' LAST sample, so no change is pending across iterations outside a
// series, and inside one the previous sample's positive (im1) is the pending row: the own-history rule of the store route holds as
// it stands.  Bound on the delay: a change waits for at most kSeriesFlush = 8 samples of its group (the sum goes out every 8
// samples of a longer series, which keeps walking on its own copy) -- ~28 us at nFactors 64, ~14 us at 16 -- and it is ONE group's
// change to the row, each sample of it computed from a row that holds the group's earlier ones.  The fold-period sweep
// (kDefaultFoldPeriod) diverged when EVERY group's updates of a hot row, ~1800 of them, were computed from one stale row; here
// the other groups' updates keep arriving and only the series' own group reads past them, for the length of the series (<= the
// run; 2 samples on average at C2, ~9 for a user of 19 feedbacks).  tests/test_gpu_bpr_positive_series.py runs 30 epochs at
// nFactors 8 and 16.
// Item classes (hot.slot): >= 0 = the replica rows of a HOT item or the accumulator row of an item of the accumulated tier,
// kWarm = fp32 atomics straight onto the row, kCold = an item whose
// row is touched so rarely (expected touches per `cold window` samples < 1, gorse_mf_create) that the reference's own unlocked
// load / fma / store (model.go:473-488 under parallel.go:44-81) loses next to nothing: its update is ONE write-through store of
// fma(t, lr, row) instead of d atomic dwords.  NEG_STORE opens that route for the NEGATIVE item of a sample; the positive's update is
// always an atomic (by store it cost 0.003-0.005 of NDCG: see kDefaultStoreMode).
constexpr int kCold = -2;  // (-1 = "warm": fp32 atomics straight onto the row)
constexpr int kSeriesFlush = 8;  // samples of a positive series whose summed change goes out together (see POSITIVE SERIES below)
#ifndef GORSE_BPR_SERIES_SKIP_GATHERS
#define GORSE_BPR_SERIES_SKIP_GATHERS 1  // A/B: 0 = the positive's row is gathered for every sample, used or not
#endif

// D8: nFactors = 8 (the width of model_test.go:35-48): lanes 0..7 of the group own the eight elements -- the unfused 8-lane tail of
// the AVX512 kernels (floats_avx512.c:350-358, VecShape::unfused) -- and lanes 8..15 mirror them (the reduction needs the products
// replicated there); only lanes 0..7 write.
#ifndef GORSE_BPR_D8_PAIRS
#define GORSE_BPR_D8_PAIRS 1  // A/B: 0 = nFactors 8 with lanes 8..15 of a group mirroring lanes 0..7 (rounds 4-5)
#endif
template <int NC, bool NEG_STORE, bool D8 = false>
__global__ __launch_bounds__(kBlock) void bpr_update_user_kernel(float *P, float *Q, const int32_t *__restrict__ si,
                                                                 const int32_t *__restrict__ sj,
                                                                 const int32_t *__restrict__ off, int32_t U, int d,
                                                                 float lr, float reg, int exp_mode, double *loss,
                                                                 HotRows hot, int folders, int neg_replicas) {
    if ((int)blockIdx.x < folders) {
        run_folders<true>(hot, Q, folders);
        return;
    }
    // sample (i1, j1) continues the series of the sample (i0, j0) in front of it: the same positive, both samples valid, and neither
    // negative is that positive (hand-made streams: such a sample's negative-side update must meet a row without pending change)
    auto continues = [](int i0, int j0, int i1, int j1) { return i0 == i1 && (i0 | j0 | j1) >= 0 && i0 != j0 && i0 != j1; };
    const int glane = threadIdx.x & (kGroup - 1);
    const int lane = D8 ? (glane & 7) : glane;   // element owned inside a 16-float chunk
    // D8 (round 6): the two halves of a 16-lane group take a user run EACH (eight lanes own a row of eight: until round 5 lanes 8..15
    // mirrored lanes 0..7 and only wrote nothing) -- eight runs per wave instead of four
    constexpr int SUBS = D8 && GORSE_BPR_D8_PAIRS ? 2 : 1;
    const bool writer = !D8 || SUBS == 2 || glane < 8;
    auto mad = [](float x, float y, float z) { return D8 ? x * y + z : fmaf(x, y, z); };
    auto tree8 = [](float v) { return SUBS == 2 ? group_tree8_halves(v) : group_tree8(v); };
    const int gib = threadIdx.x / kGroup;
    const int64_t group = ((int64_t)((int)blockIdx.x - folders) * kGroupsPerBlock + gib) * SUBS + (SUBS == 2 ? glane >> 3 : 0);
    const int64_t ngroups = (int64_t)((int)gridDim.x - folders) * kGroupsPerBlock * SUBS;
    const float nreg = -reg;
    double my_loss = 0.0;
    // which class look-ups this launch needs (every path issues the same loads from a valid address: a look-up nobody needs
    // reads a word that is in cache anyway)
    const bool open = folders > 0;  // the launch has rows that take an item's updates, of either tier (open_hot)
    const bool look_i = open;
    const bool look_j = (open && neg_replicas) || NEG_STORE;
    const int32_t *slot_of = (look_i || look_j) ? hot.slot : si;
    // the items of this group's last two samples: a row one of them wrote is NOT in the snapshot of the current sample (gathered
    // two samples ago), so its update goes through an atomic whatever its class -- a store would overwrite the group's own work
    int im1 = -1, jm1 = -1, im2 = -1, jm2 = -1;
    for (int64_t u = group; u < U; u += ngroups) {
        const int beg = off[u], end = off[u + 1];
        if (beg >= end) continue;
        float *pu = P + u * d;
        // item rows are gathered G = 2 samples ahead of the arithmetic (ra[0] / rb[0]: this sample, ra[k]: sample s + k, the row of sample
        // s + G in flight), their indices IA = 3 ahead and the class of an item G ahead; positions past the run's end re-read the
        // last sample (result unused).  Nothing is used in the iteration that loads it: the counter the waits go by also counts the
        // atomics and returns in order, so a wait for a load issued after them is a wait for their acknowledgement from the memory
        // side.  What a load waits behind is therefore the atomics of min(G, IA - G) iterations ago: with few groups per SIMD
        // (C2: 6040 groups on 1024 SIMDs) that distance IS the time of an iteration.  (Deeper pipelines -- up to rows 6 and ids 9 ahead --
        // and a ring without register rotation were measured and were no faster: profiles/r04_s_probe_bpr_depth.txt.)
        constexpr int G = 2, IA = 3;  // (the own-history rule of the store route looks G = 2 samples back)
        // with the store route open for negatives their rows are gathered ONE sample ahead instead of two: what a store can
        // overwrite is what other groups added between the gather and the store, and that window halves
        constexpr int GB = NEG_STORE ? 1 : G;  // the negative's gather distance
        float p[NC], ra[G][NC], rb[GB][NC];
        const int last = end - 1;
        auto at = [&](int s) { return s <= last ? s : last; };
        auto cl = [](int x) { return x < 0 ? 0 : x; };  // a skipped sample (i = j = -1) gathers row 0, its results are not used
        auto idx_i = [&](int i_, int j_) { return look_i ? cl(i_) : (look_j ? cl(j_) : beg); };
        auto idx_j = [&](int i_, int j_) { return look_j ? cl(j_) : (look_i ? cl(i_) : beg); };
        int ii[IA], jj[IA], sli[G], slj[G];
#pragma unroll
        for (int k = 0; k < IA; k++) ii[k] = si[at(beg + k)], jj[k] = sj[at(beg + k)];
#pragma unroll
        for (int k = 0; k < G; k++) sli[k] = slot_of[idx_i(ii[k], jj[k])], slj[k] = slot_of[idx_j(ii[k], jj[k])];
        // the series in flight: `cur` the positive's row as this group has left it, `acc` its change not yet sent (of `pending`
        // samples), `cont` = the current sample continues the series of the one before
        float cur[NC], acc[NC];
        bool cont = false;
        int pending = 0;
#pragma unroll
        for (int c = 0; c < NC; c++) {
            p[c] = load_row<MODE_ATOMIC>(pu + 16 * c + lane);
#pragma unroll
            for (int k = 0; k < G; k++) ra[k][c] = load_row<MODE_ATOMIC>(Q + (int64_t)cl(ii[k]) * d + 16 * c + lane);
#pragma unroll
            for (int k = 0; k < GB; k++) rb[k][c] = load_row<MODE_ATOMIC>(Q + (int64_t)cl(jj[k]) * d + 16 * c + lane);
        }
        for (int s = beg; s < end; s++) {
            const int in_ = si[at(s + IA)], jn_ = sj[at(s + IA)];
            const int sli_n = slot_of[idx_i(ii[G], jj[G])];
            const int slj_n = slot_of[idx_j(ii[G], jj[G])];
            const int i = ii[0], j = jj[0], slot = sli[0], slotj = slj[0];
            float(&a)[NC] = ra[0];
            float(&b)[NC] = rb[0];
            float ran[NC], rbn[NC];
            // the positive's row of sample s + G: not gathered where that sample will continue a series (it computes from `cur`)
            const bool gather_i = !GORSE_BPR_SERIES_SKIP_GATHERS || !(s + G <= last && continues(ii[G - 1], jj[G - 1], ii[G], jj[G]));
#pragma unroll
            for (int c = 0; c < NC; c++) ran[c] = 0.0f;
            if (gather_i) {
#pragma unroll
                for (int c = 0; c < NC; c++) ran[c] = load_row<MODE_ATOMIC>(Q + (int64_t)cl(ii[G]) * d + 16 * c + lane);
            }
#pragma unroll
            for (int c = 0; c < NC; c++) rbn[c] = load_row<MODE_ATOMIC>(Q + (int64_t)cl(jj[GB]) * d + 16 * c + lane);
            if (cont) {
#pragma unroll
                for (int c = 0; c < NC; c++) a[c] = cur[c];
            }
            const bool more = s < last && continues(i, j, ii[1], jj[1]);  // the next sample continues this one's series
            const bool valid = j >= 0;  // j < 0: the sampler found no negative for this sample (bpr_sample_items_kernel)
            float *qi = Q + (int64_t)cl(i) * d, *qj = Q + (int64_t)cl(j) * d;
            if (open && slot >= 0) qi = hot_row(hot, slot, group);
            if (open && neg_replicas && slotj >= 0) qj = hot_row(hot, slotj, group);
            bool st_j = false;
            if constexpr (NEG_STORE) {
                const bool own_j = i == j || j == im1 || j == jm1 || j == im2 || j == jm2;
                st_j = slotj == kCold && !own_j;
            }
            const float diff = D8 ? tree8(p[0] * a[0]) - tree8(p[0] * b[0]) : dot512_regs<NC>(p, a) - dot512_regs<NC>(p, b);
            const float ex = bpr_exp(-diff, exp_mode);
            const float grad = ex / (1.0f + ex);
            if (loss && (SUBS == 2 ? (glane & 7) == 0 : glane == 0) && valid) my_loss += (double)log1pf(ex);
            float t1[NC], t2[NC];
#pragma unroll
            for (int c = 0; c < NC; c++) {
                t1[c] = mad(a[c], nreg, p[c] * grad);
                t2[c] = mad(b[c], nreg, p[c] * (-grad));
                const float t3 = mad(p[c], nreg, (a[c] - b[c]) * grad);
                p[c] = valid ? mad(t3, lr, p[c]) : p[c];
            }
            if (valid) {  // (every lane keeps the series: the lanes that mirror a row of eight need `cur` as the writers do)
#pragma unroll
                for (int c = 0; c < NC; c++) {
                    acc[c] = pending > 0 ? acc[c] + t1[c] * lr : t1[c] * lr;  // a series of one sends t1 * lr, as the kernel did without series
                    cur[c] = mad(t1[c], lr, a[c]);
                }
                if (!more || ++pending >= kSeriesFlush) {
                    pending = 0;
                    if (writer) {
#pragma unroll
                        for (int c = 0; c < NC; c++)
                            __hip_atomic_fetch_add(qi + 16 * c + lane, acc[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                }
            }
            cont = more;
            if (!valid || !writer) {
            } else if (st_j) {
#pragma unroll
                for (int c = 0; c < NC; c++)
                    __hip_atomic_store(qj + 16 * c + lane, mad(t2[c], lr, b[c]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } else {
#pragma unroll
                for (int c = 0; c < NC; c++)
                    __hip_atomic_fetch_add(qj + 16 * c + lane, t2[c] * lr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
#pragma unroll
            for (int c = 0; c < NC; c++) {
#pragma unroll
                for (int k = 0; k + 1 < G; k++) ra[k][c] = ra[k + 1][c];
                ra[G - 1][c] = ran[c];
#pragma unroll
                for (int k = 0; k + 1 < GB; k++) rb[k][c] = rb[k + 1][c];
                rb[GB - 1][c] = rbn[c];
            }
            im2 = im1, jm2 = jm1, im1 = i, jm1 = j;
#pragma unroll
            for (int k = 0; k + 1 < IA; k++) ii[k] = ii[k + 1], jj[k] = jj[k + 1];
            ii[IA - 1] = in_, jj[IA - 1] = jn_;
#pragma unroll
            for (int k = 0; k + 1 < G; k++) sli[k] = sli[k + 1], slj[k] = slj[k + 1];
            sli[G - 1] = sli_n, slj[G - 1] = slj_n;
        }
        if (writer) {
#pragma unroll
            for (int c = 0; c < NC; c++)  // the only writer of this row in the launch
                __hip_atomic_store(pu + 16 * c + lane, p[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (loss && (SUBS == 2 ? (glane & 7) == 0 : glane == 0) && my_loss != 0.0) atomicAdd(loss, my_loss);
    if (folders > 0) worker_done<true>(hot);
}

// the whole scan by ONE workgroup, tile after tile (a few thousand counters: two launches and two dependencies fewer)
__global__ __launch_bounds__(256) void scan_small_kernel(int32_t *__restrict__ data, int64_t m) {
    __shared__ int32_t lds[4];
    int32_t carry = 0;
    for (int64_t t0 = 0; t0 < m; t0 += kScanTile) {
        const int64_t base = t0 + (int64_t)threadIdx.x * 8;
        int32_t x[8], v = 0;
#pragma unroll
        for (int e = 0; e < 8; e++) {
            x[e] = base + e < m ? data[base + e] : 0;
            v += x[e];
        }
        int32_t total;
        int32_t run = carry + block_exclusive_scan_256(v, lds, &total);
#pragma unroll
        for (int e = 0; e < 8; e++) {
            if (base + e < m) data[base + e] = run;
            run += x[e];
        }
        carry += total;
    }
}

int32_t exclusive_scan_i32(int32_t *data, int64_t m, int32_t *tmp, hipStream_t st) {
    const int64_t nt = ceil_div(m, kScanTile);
    if (nt <= 16) {
        scan_small_kernel<<<dim3(1), dim3(256), 0, st>>>(data, m);
        GORSE_HIP_CHECK(hipGetLastError());
        return GORSE_OK;
    }
    scan_tile_sums_kernel<<<dim3((unsigned)nt), dim3(256), 0, st>>>(data, m, tmp);
    scan_sums_kernel<<<dim3(1), dim3(256), 0, st>>>(tmp, nt);
    scan_apply_kernel<<<dim3((unsigned)nt), dim3(256), 0, st>>>(data, m, tmp);
    GORSE_HIP_CHECK(hipGetLastError());
    return GORSE_OK;
}


// counting sort of the chunk's triplets by user: `sorted` receives su | si | sj, bucket[0..U] the run offsets
int32_t launch_user_sort(gorse_mf *h, const int32_t *trip, int32_t *sorted, int32_t *bucket, int32_t *rank, int64_t n, size_t cap,
                         hipStream_t st) {
    const int64_t m = h->U + 2;  // one counter per user + one for skipped samples (sorted last) + the end offset
    const int64_t blocks = std::min<int64_t>(ceil_div(n, 256), 256 * 8);
    GORSE_HIP_CHECK(hipMemsetAsync(bucket, 0, (size_t)m * sizeof(int32_t), st));
    // key = user, skipped samples (u < 0) get key U; GORSE_TEST_BPR_STABLE_RANK: one thread ranks the samples in stream order
    if (g_variant & GORSE_TEST_BPR_STABLE_RANK)
        bpr_rank_kernel<<<dim3(1), dim3(1), 0, st>>>(trip, n, (int32_t)h->U, bucket, rank);
    else
        bpr_rank_kernel<<<dim3((unsigned)blocks), dim3(256), 0, st>>>(trip, n, (int32_t)h->U, bucket, rank);
    GORSE_TRY(exclusive_scan_i32(bucket, m, h->scan_tmp2.p, st));
    bpr_scatter_by_kernel<<<dim3((unsigned)blocks), dim3(256), 0, st>>>(trip, trip, trip + cap, trip + 2 * cap, n,
                                                                       (int32_t)h->U, bucket, rank, sorted,
                                                                       sorted + cap, sorted + 2 * cap);
    GORSE_HIP_CHECK(hipGetLastError());
    return GORSE_OK;
}
int32_t ensure_user_sort(gorse_mf *h) {
    const int64_t m = h->U + 2;
    // the tile x bin matrix of the binned preparation: prep_bins gives a chunk at most max(512, cap / 65536) tiles and min(kMaxBins - 1, U + 1) bins
    const size_t mat = prep_matrix_words(h->U, (int64_t)h->trip_cap);
    if ((size_t)m <= h->ubucket[0].n && h->scan_tmp2.n >= (size_t)ceil_div(m, kScanTile) && h->urank[0].n >= 2 * h->trip_cap &&
        h->ubins.n >= (size_t)2 * kMaxBins && h->ubinmat.n >= mat)
        return GORSE_OK;
    GORSE_TRY(mf_sync_streams(h));
    if (h->ubins.n < (size_t)2 * kMaxBins) GORSE_TRY(h->ubins.alloc((size_t)2 * kMaxBins));
    if (h->ubinmat.n < mat) GORSE_TRY(h->ubinmat.alloc(mat));
    for (int b = 0; b < 2; b++) {
        GORSE_TRY(h->ubucket[b].alloc((size_t)m));
        // per buffer (the sampler of chunk c + 1 ranks while chunk c is applied); twice the chunk: the binned preparation's (sample id,
        // user) pairs in sorted order
        GORSE_TRY(h->urank[b].alloc(2 * h->trip_cap));
    }
    if (h->scan_tmp2.n < (size_t)ceil_div(m, kScanTile)) GORSE_TRY(h->scan_tmp2.alloc((size_t)ceil_div(m, kScanTile)));
    return GORSE_OK;
}
// user runs need enough users to fill the chip with one 16-lane group each (4096 groups = one wave per SIMD) and a
// register-resident factor width; otherwise the per-sample schedule is the faster one (S-ml100k: 943 users)
bool user_runs_supported(const gorse_mf *h) {
    return (h->d == 8 || h->d == 16 || h->d == 32 || h->d == 64 || h->d == 128) && (h->U >= 4096 || (g_variant & GORSE_TEST_BPR_USER_RUNS));
}

// which item updates may take the store route (gorse_hip_test_set_bpr_store_mode)
// Cold negatives by store: measured at C3 whole (profiles/r04_b_probe_bpr_stores_*.txt): update kernel 89 -> 60 ms per epoch, 4 % of the updates of cold rows
// overwritten, NDCG@10 0.6100 against 0.6096 with atomics only (sequential oracle 0.6126); the positive side stays atomic -- by store
// it costs 0.003-0.005 of NDCG for 6 % more speed
constexpr int kDefaultStoreMode = 1;
int g_store_mode = kDefaultStoreMode;  // 1 = NEG_STORE of bpr_update_user_kernel where the handle has cold items, 0 = atomics only

// the replica rows of a slot lie next to each other (r04_a: 4 KB apart or n_hot rows apart makes no difference); n_hot stays 0 (no
// replicas, no folders) until the launch opens them: open_hot
HotRows make_hot(const gorse_mf *h) {
    return HotRows{h->hot_slot.p, h->hot_items.p, h->hot_meta.p, h->hot_rep.p, h->hot_done.p, 0, h->d, 0, g_fold_period, 0, g_acc_fold_every,
                   h->hot_base.p, 0, g_folder_timeout};
}
bool has_hot(const gorse_mf *h) { return h->n_hot > 0 || h->n_acc > 0; }  // any row that takes an item's updates for it
// an update launch with folders: the replicas open, the launch's set of arrival stripes by launch parity (the set of the launch before
// is zeroed by this one's folders; gorse_mf_create zeroed both)
int open_hot(gorse_mf *h, HotRows &hot) {
    hot.n_hot = h->n_hot;
    hot.n_acc = h->n_acc;
    hot.set = (int)(h->hot_launches++ & 1);
    return kFolderBlocks + (h->n_acc > 0 ? kFolderBlocksAcc : 0);
}

// start / stop (may be null): events bound to the kernel's own dispatch (hipExtLaunchKernelGGL) -- its timestamps and its completion
// signal, no marker packet on the stream (epoch_impl)
int32_t launch_update_users(gorse_mf *h, const int32_t *sorted, const int32_t *bucket, size_t cap, float lr, float reg,
                            int exp_mode, double *loss, hipStream_t st, bool stores, hipEvent_t start = nullptr,
                            hipEvent_t stop = nullptr) {
    const int d = h->d;
    int64_t blocks = ceil_div(h->U, (int64_t)kGroupsPerBlock * (d == 8 && GORSE_BPR_D8_PAIRS ? 2 : 1));  // nFactors 8: two runs per group
    const int64_t capb = 256 * 16;
    if (blocks > capb) blocks = capb;
    HotRows hot = make_hot(h);
    const int folders = has_hot(h) ? open_hot(h, hot) : 0;
    blocks += folders;
    // the negative's slot look-up is one more gather per sample: where a draw has a fair chance of meeting a hot item (hot_rows.hpp;
    // gorse_mf_create counted the negatives into the replica counts by the same rule)
    // -- and always with the accumulated tier, where every item has a row
    const int neg_rep = hot.n_acc > 0 || (hot.n_hot > 0 && hot_neg_replicas(hot.n_hot, h->I)) ? 1 : 0;
    dim3 grid((unsigned)blocks), block(kBlock);
    // cold items by store only in GORSE_BPR_HOGWILD_STORES and where the handle has any (n_cold) -- the atomics-only instantiation otherwise
    const bool neg_store = stores && h->n_cold > 0 && g_store_mode == 1;
    // The sole-writer fold (above HotRows): with the tier neg_rep is 1 and every item's class word is >= 0, so without the store route
    // no worker instruction of this kernel addresses Q for writing -- the folders are the only writers of the rows they fold
    hot.sole = GORSE_BPR_FOLD_SOLE_WRITER && hot.n_acc > 0 && !neg_store && h->hot_base.p != nullptr ? 1 : 0;
    if (folders > 0) h->fold_sole_last = hot.sole;
#define LAUNCH2(NC, NEG_STORE)                                                                                         \
    hipExtLaunchKernelGGL((bpr_update_user_kernel<(NC == 0 ? 1 : NC), NEG_STORE, NC == 0>), grid, block, 0, st, start, stop, 0,     \
                          h->P.p, h->Q.p, sorted + cap, sorted + 2 * cap, bucket, (int32_t)h->U, d, lr, reg, exp_mode, loss, hot, \
                          folders, neg_rep)
#define LAUNCH(NC)                                                                                                     \
    do {                                                                                                               \
        if (neg_store)                                                                                                 \
            LAUNCH2(NC, true);                                                                                         \
        else                                                                                                           \
            LAUNCH2(NC, false);                                                                                        \
    } while (0)
    if (d == 8)
        LAUNCH(0);
    else if (d == 16)
        LAUNCH(1);
    else if (d == 32)
        LAUNCH(2);
    else if (d == 64)
        LAUNCH(4);
    else
        LAUNCH(8);
#undef LAUNCH2
#undef LAUNCH
    GORSE_HIP_CHECK(hipGetLastError());
    return GORSE_OK;
}

template <int MODE>
int32_t launch_update_mode(gorse_mf *h, const int32_t *us, const int32_t *is, const int32_t *js, const int32_t *order,
                           int64_t begin, int64_t end, float lr, float reg, int exp_mode, double *loss,
                           hipStream_t st, hipEvent_t start, hipEvent_t stop) {
    const int64_t n = end - begin;
    if (n <= 0) return GORSE_OK;
    const int d = h->d;
    int64_t blocks = ceil_div(n, kGroupsPerBlock);
    const int64_t cap = 256 * 16;  // 16 workgroups of 4 waves per CU: grid-stride beyond that
    if (blocks > cap) blocks = cap;
    HotRows hot = make_hot(h);
    const int folders = MODE == MODE_ATOMIC && has_hot(h) ? open_hot(h, hot) : 0;
    if (folders > 0) h->fold_sole_last = 0;  // (the per-sample kernel's fold is the atomic one, then bpr_fold_kernel)
    blocks += folders;
    dim3 grid((unsigned)blocks), block(kBlock);
#define LAUNCH(NC, SH)                                                                                              \
    hipExtLaunchKernelGGL((bpr_update_kernel<NC, MODE>), grid, block, SH, st, start, folders > 0 ? nullptr : stop, 0, h->P.p, \
                          h->Q.p, us, is, js, order, begin, end, d, lr, reg, exp_mode, loss, hot, folders)
    if (d == 16)
        LAUNCH(1, 0);
    else if (d == 32)
        LAUNCH(2, 0);
    else if (d == 64)
        LAUNCH(4, 0);
    else if (d == 128)
        LAUNCH(8, 0);
    else
        LAUNCH(0, (size_t)kGroupsPerBlock * 3 * d * sizeof(float));
#undef LAUNCH
    GORSE_HIP_CHECK(hipGetLastError());
    if (folders > 0) {  // (its folders make no last pass: worker_done); the launch's stop event is this kernel's
        const int64_t fb = std::min<int64_t>(ceil_div((int64_t)(hot.n_hot + hot.n_acc) * d, 256), 512);
        hipExtLaunchKernelGGL(bpr_fold_kernel, dim3((unsigned)fb), dim3(256), 0, st, nullptr, stop, 0, hot, h->Q.p);
        GORSE_HIP_CHECK(hipGetLastError());
    }
    return GORSE_OK;
}

int32_t launch_update(gorse_mf *h, int mode, const int32_t *us, const int32_t *is, const int32_t *js,
                      const int32_t *order, int64_t begin, int64_t end, float lr, float reg, int exp_mode, double *loss,
                      hipStream_t st, hipEvent_t start = nullptr, hipEvent_t stop = nullptr) {
    switch (mode) {
    case MODE_ATOMIC:
        return launch_update_mode<MODE_ATOMIC>(h, us, is, js, order, begin, end, lr, reg, exp_mode, loss, st, start, stop);
    case MODE_EXACT:
        return launch_update_mode<MODE_EXACT>(h, us, is, js, order, begin, end, lr, reg, exp_mode, loss, st, start, stop);
    case MODE_RACY:
        return launch_update_mode<MODE_RACY>(h, us, is, js, order, begin, end, lr, reg, exp_mode, loss, st, start, stop);
    }
    return fail(GORSE_ERR_INVALID, "unknown BPR mode %d", mode);
}

int32_t launch_sampler(gorse_mf *h, uint64_t seed, uint64_t epoch, int64_t base, int64_t n, int32_t *trip, size_t cap,
                       hipStream_t st, hipEvent_t start = nullptr, hipEvent_t stop = nullptr) {
    if (n <= 0) return GORSE_OK;
    int64_t blocks = std::min<int64_t>(ceil_div(n, 256), 256 * 8);
    hipExtLaunchKernelGGL(bpr_sample_kernel, dim3((unsigned)blocks), dim3(256), 0, st, start, stop, 0, (int32_t)h->U, (int32_t)h->I,
                          h->uptr.p, h->uidx.p, h->uidx_sorted.p, seed, epoch, base, n, trip, trip + cap, trip + 2 * cap,
                          h->fail_count.p);
    GORSE_HIP_CHECK(hipGetLastError());
    return GORSE_OK;
}

// The user-run schedule's preparation of one chunk (see bpr_sample_user_kernel): user draws + ranks, scan of the run counters,
// sample ids scattered to their sorted positions, item draws by run.  `trip` (3 x cap ints, otherwise the unsorted triplets)
// holds the keys and (sample id, user) pairs; `rank` (2 x cap) the ranks or the sorted pairs; `sorted` receives si at cap, sj at
// 2 cap; bucket[0..U + 1] the run offsets.
// (PrepBins / prep_bins: csrc/bpr_bins.hpp, shared with the CPU cover test)
constexpr size_t kItemsBatchFrom = (size_t)8 << 20;  // feedbacks of a handle beyond which the users' rows cannot all sit in the L2s
int32_t launch_prepare_users(gorse_mf *h, uint64_t seed, uint64_t epoch, int64_t base, int64_t n, int32_t *trip, int32_t *sorted,
                             int32_t *bucket, int32_t *rank, size_t cap, hipStream_t st) {
    if (n <= 0) return GORSE_OK;
    const int64_t m = h->U + 2;
    const int64_t blocks = std::min<int64_t>(ceil_div(n, 256), 256 * 8);
    const PrepBins pb = prep_bins(h->U, n);
    // the profile's spans of this chain are bound to their kernels (KernelProfile::events): a span of one kernel is that launch's start
    // and stop event, a span of several the start of its first and the stop of its last -- no marker packet on the preparation stream
    hipEvent_t ev_a = nullptr, ev_b = nullptr;
    // the item draws: four positions per thread where the users' rows cannot all sit in the L2s (see bpr_sample_items_batch_kernel)
    auto launch_items = [&](const int2 *pairs) {
        h->prof.events(GORSE_PROF_BPR_SAMPLE, &ev_a, &ev_b);
        if (h->uidx.n > kItemsBatchFrom)
            hipExtLaunchKernelGGL(bpr_sample_items_batch_kernel, dim3((unsigned)blocks), dim3(256), 0, st, ev_a, ev_b, 0, (int32_t)h->U,
                                  (int32_t)h->I, h->uptr.p, h->uidx.p, h->uidx_sorted.p, seed, epoch, base, n, pairs, sorted + cap,
                                  sorted + 2 * cap, h->fail_count.p);
        else
            hipExtLaunchKernelGGL(bpr_sample_items_kernel, dim3((unsigned)blocks), dim3(256), 0, st, ev_a, ev_b, 0, (int32_t)h->U,
                                  (int32_t)h->I, h->uptr.p, h->uidx.p, h->uidx_sorted.p, seed, epoch, base, n, pairs, sorted + cap,
                                  sorted + 2 * cap, h->fail_count.p);
    };
    // equal positives of a run next to each other (bpr_group_positives_kernel): one wave per run, in place
    auto launch_group = [&]() {
        if (g_variant & GORSE_TEST_BPR_ARRIVAL_ORDER) return;
        h->prof.events(GORSE_PROF_BPR_SORT, &ev_a, &ev_b);
        hipExtLaunchKernelGGL(bpr_group_positives_kernel, dim3((unsigned)std::min<int64_t>(h->U, 256 * 16)), dim3(64), 0, st, ev_a, ev_b, 0,
                              (int32_t)h->U, bucket, sorted + cap, sorted + 2 * cap);
    };
    if (pb.ok && !(g_variant & GORSE_TEST_BPR_NO_BINS)) {
        int32_t *key = trip;
        int2 *bp = reinterpret_cast<int2 *>(trip + cap), *pairs = reinterpret_cast<int2 *>(rank);  // (rank: 2 x cap words, ensure_user_sort)
        int32_t *bin_count = h->ubins.p, *bin_start = h->ubins.p + kMaxBins, *H = h->ubinmat.p;
        const unsigned tiles = (unsigned)ceil_div(n, pb.tile);
        if ((size_t)tiles * pb.nbins > h->ubinmat.n) return fail(GORSE_ERR_INVALID, "tile x bin matrix smaller than %u x %d", tiles, pb.nbins);
        // the finish of the bins in one LDS-resident pass (bpr_bin_finish_kernel) where a bin's expected samples are safely under
        // its capacity (the 10M-user set: ~27,500 per bin), a bin's users have a counter each, and the users' rows sit in the L2s:
        // where they do not (C3 shapes) the item draws are bpr_sample_items_batch_kernel's, four chains of look-ups per thread, which
        // the finish kernel does not have; GORSE_TEST_BPR_THREE_KERNELS: the three kernels whatever the shape
        const bool finish = !(g_variant & GORSE_TEST_BPR_THREE_KERNELS) && pb.shift <= kFinShift && n / pb.nbins <= kFinCap / 4 * 3 &&
                            h->uidx.n <= kItemsBatchFrom;
        h->prof.events(GORSE_PROF_BPR_SAMPLE, &ev_a, &ev_b);
        hipExtLaunchKernelGGL(bpr_bin_count_kernel, dim3(tiles), dim3(kBinThreads), 0, st, ev_a, ev_b, 0, (int32_t)h->U, h->uptr.p, seed,
                              epoch, base, n, pb.tile, pb.shift, pb.nbins, key, h->fail_count.p, H);
        // the sort's span: offsets, scatter and (without the finish) the bins' sort
        h->prof.events(GORSE_PROF_BPR_SORT, &ev_a, &ev_b);
        hipExtLaunchKernelGGL(bpr_bin_offsets_kernel, dim3((unsigned)ceil_div(pb.nbins, 64)), dim3(kOffWaves * 64), 0, st, ev_a, nullptr, 0,
                              H, (int)tiles, pb.nbins, bin_count);
        hipExtLaunchKernelGGL(bpr_bin_scatter_kernel, dim3(tiles), dim3(kBinThreads), 0, st, nullptr, finish ? ev_b : nullptr, 0,
                              (int32_t)h->U, key, n, pb.tile, pb.shift, pb.nbins, bin_count, H, bin_start, bp);
        if (finish) {
            h->prof.events(GORSE_PROF_BPR_SAMPLE, &ev_a, &ev_b);
            hipExtLaunchKernelGGL(bpr_bin_finish_kernel, dim3((unsigned)pb.nbins), dim3(kFinThreads), 0, st, ev_a, ev_b, 0, (int32_t)h->U,
                                  (int32_t)h->I, pb.shift, bin_start, bp, h->uptr.p, h->uidx.p, h->uidx_sorted.p, seed, epoch, base, bucket,
                                  pairs, sorted + cap, sorted + 2 * cap, h->fail_count.p, (g_variant & GORSE_TEST_BPR_ARRIVAL_ORDER) ? 0 : 1);
            GORSE_HIP_CHECK(hipGetLastError());
            return GORSE_OK;
        }
        hipExtLaunchKernelGGL(bpr_bin_sort_kernel, dim3((unsigned)pb.nbins), dim3(256), 0, st, nullptr, ev_b, 0, (int32_t)h->U, pb.shift,
                              pb.nbins, bin_start, bp, bucket, pairs);
        launch_items(pairs);
        launch_group();
        GORSE_HIP_CHECK(hipGetLastError());
        return GORSE_OK;
    }
    int32_t *key = trip;
    int2 *pairs = reinterpret_cast<int2 *>(trip + cap);
    int tok = h->prof.begin(GORSE_PROF_BPR_SAMPLE, st);
    GORSE_HIP_CHECK(hipMemsetAsync(bucket, 0, (size_t)m * sizeof(int32_t), st));
    bpr_sample_user_kernel<<<dim3((unsigned)blocks), dim3(256), 0, st>>>((int32_t)h->U, h->uptr.p, seed, epoch, base, n, key,
                                                                         h->fail_count.p, bucket, rank);
    h->prof.end(tok, st);
    tok = h->prof.begin(GORSE_PROF_BPR_SORT, st);
    GORSE_TRY(exclusive_scan_i32(bucket, m, h->scan_tmp2.p, st));
    bpr_scatter_ids_kernel<<<dim3((unsigned)blocks), dim3(256), 0, st>>>(key, rank, bucket, n, (int32_t)h->U, pairs);
    h->prof.end(tok, st);
    launch_items(pairs);
    launch_group();
    GORSE_HIP_CHECK(hipGetLastError());
    return GORSE_OK;
}

// Samples per chunk.  The user-run schedule loads p_u once per RUN (a user's samples inside one chunk), so a chunk should hold
// a few dozen samples per user: 4M samples serve the S-ml1m and C3-shard shapes (<= 125K users); the full C3 set (1M users)
// takes 32M, the 10M-user set 128M -- 64 bytes of triplet / pair / sort buffers per sample of capacity, 8.2 GB of the 288 at most.
int64_t g_chunk_override = 0;  // probe: gorse_hip_test_set_bpr_chunk
int64_t chunk_capacity(const gorse_mf *h) {
    if (g_chunk_override > 0) return g_chunk_override;
    const int64_t lo = (int64_t)1 << 22, hi = (int64_t)1 << 27;
    return std::min(std::max(lo, 32 * h->U), hi);
}

int32_t ensure_trip(gorse_mf *h, int64_t want) {
    size_t cap = (size_t)std::min<int64_t>(std::max<int64_t>(want, 1), chunk_capacity(h));
    cap = (cap + 1) & ~(size_t)1;  // even: trip + cap is read as (sample id, user) pairs of 8 bytes
    if (cap <= h->trip_cap) return GORSE_OK;
    GORSE_TRY(mf_sync_streams(h));
    for (int b = 0; b < 2; b++) GORSE_TRY(h->trip[b].alloc(cap * 3));
    for (int b = 0; b < 2; b++) GORSE_TRY(h->sorted[b].alloc(cap * 3));
    h->trip_cap = cap;
    return GORSE_OK;
}

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
        GORSE_TRY(launch_update(h, MODE_EXACT, d_us, d_is, d_js, h->order.p, level_ptr[l], level_ptr[l + 1], lr, reg,
                                exp_mode, d_loss, h->stream));
    }
    GORSE_HIP_CHECK(hipStreamSynchronize(h->stream));  // `order` (host vector) was copied asynchronously
    return GORSE_OK;
}

// Hogwild schedule: 1 = user runs (bpr_update_user_kernel), 0 = per-sample groups (bpr_update_kernel).  The
// environment variable GORSE_BPR_SCHEDULE = "users" | "samples" overrides the compiled default (read once);
// GORSE_TEST_BPR_USER_RUNS / _PER_SAMPLE of gorse_hip_test_set_variant override both.
int g_user_runs = 1;
bool user_runs_default() {
    static const int v = [] {
        const char *e = getenv("GORSE_BPR_SCHEDULE");
        if (e && !strcmp(e, "users")) return 1;
        if (e && !strcmp(e, "samples")) return 0;
        return g_user_runs;
    }();
    return v != 0;
}
bool user_runs_enabled() {
    return (g_variant & GORSE_TEST_BPR_USER_RUNS) ? true : ((g_variant & GORSE_TEST_BPR_PER_SAMPLE) ? false : user_runs_default());
}
int g_exp_mode_exact = 0;  // exp flavour of the sequential schedule; tests flip it to 1 for bit parity

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
    GORSE_TRY(ensure_trip(h, n_samples));
    double *d_loss = loss_out ? h->loss.p : nullptr;
    // Epoch pacing: the (begin, end) pair gorse_mf_epoch_throttle / _times read (csrc/mf.hip).  Between two update kernels the update
    // stream carries the wait on the chunk's preparation and nothing else: the epoch's end, the chunk's "consumed" event and the
    // profile's span are the launch's own events (ev_consumed, mf_internal.hpp).  An epoch that does not begin where the one before it
    // ended takes its begin from its first update launch (ep_begin) -- unless something else of the epoch comes first on the stream (the
    // loss memset, the sequential schedule's sampler, the sort of GORSE_TEST_BPR_STABLE_RANK) or the profile needs that launch's start
    // event: then the begin is recorded where the stream reaches the epoch, as the only marker packet of the epoch.
    const bool uruns = (mode == MODE_ATOMIC || mode == MODE_STORES) && user_runs_enabled() && user_runs_supported(h);
    const bool stable_rank = uruns && (g_variant & GORSE_TEST_BPR_STABLE_RANK);  // the sort on the update stream, by one thread
    hipEvent_t ep_begin = nullptr, ep_end = nullptr;
    GORSE_TRY(mf_epoch_begin(h, chained, d_loss || mode == MODE_EXACT || stable_rank || h->prof.on, &ep_begin));
    if (d_loss) GORSE_HIP_CHECK(hipMemsetAsync(d_loss, 0, sizeof(double), h->stream));
    const int64_t cap = (int64_t)h->trip_cap;
    if (mode == MODE_EXACT) {
        std::vector<int32_t> host((size_t)cap * 3);
        for (int64_t s0 = 0; s0 < n_samples; s0 += cap) {
            const int64_t m = std::min(cap, n_samples - s0);
            int32_t *tb = h->trip[0].p;
            GORSE_TRY(launch_sampler(h, seed, epoch, base + s0, m, tb, (size_t)cap, h->stream));
            GORSE_HIP_CHECK(hipMemcpyAsync(host.data(), tb, (size_t)cap * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
            GORSE_HIP_CHECK(hipStreamSynchronize(h->stream));
            GORSE_TRY(run_sequential(h, tb, tb + cap, tb + 2 * cap, host.data(), host.data() + cap, host.data() + 2 * cap, m,
                                     lr, reg, g_exp_mode_exact, cancel, d_loss));
        }
    } else {
        // two-stream pipeline: stream2 samples (and item-sorts) chunk c+1 while stream applies chunk c; the
        // buffer parity runs on across calls so that back-to-back enqueued epochs overlap as well
        if (uruns) GORSE_TRY(ensure_user_sort(h));
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
                GORSE_TRY(launch_prepare_users(h, seed, epoch, base + s0, m, tb, h->sorted[b].p, h->ubucket[b].p, h->urank[b].p,
                                               (size_t)cap, prep));
            } else {
                hipEvent_t sa = nullptr, sb = nullptr;
                h->prof.events(GORSE_PROF_BPR_SAMPLE, &sa, &sb);
                GORSE_TRY(launch_sampler(h, seed, epoch, base + s0, m, tb, (size_t)cap, prep, sa, sb));
            }
            GORSE_HIP_CHECK(hipEventRecord(h->ev_sampled[b], prep));
            GORSE_HIP_CHECK(hipStreamWaitEvent(h->stream, h->ev_sampled[b], 0));
            if (stable_rank) {  // the triplets ranked by one thread and scattered, on the update stream
                const int tok = h->prof.begin(GORSE_PROF_BPR_SORT, h->stream);
                GORSE_TRY(launch_user_sort(h, tb, h->sorted[b].p, h->ubucket[b].p, h->urank[b].p, m, (size_t)cap, h->stream));
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
                GORSE_TRY(launch_update_users(h, h->sorted[b].p, h->ubucket[b].p, (size_t)cap, lr, reg, g_exp_mode_exact, d_loss, h->stream,
                                              mode == MODE_STORES, start, stop));
            else  // (the per-sample schedule has no store route: mode 3 is mode 0 there)
                GORSE_TRY(launch_update(h, mode == MODE_STORES ? MODE_ATOMIC : mode, tb, tb + cap, tb + 2 * cap, nullptr, 0, m, lr, reg, 0, d_loss,
                                        h->stream, start, stop));
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

extern "C" void gorse_hip_test_set_exact_exp(int32_t mode) { g_exp_mode_exact = mode; }

extern "C" int32_t gorse_mf_bpr_schedule(gorse_mf *h, int32_t *user_runs) {
    if (!h || !user_runs) return fail(GORSE_ERR_INVALID, "NULL argument");
    *user_runs = (user_runs_enabled() && user_runs_supported(h)) ? 1 : 0;
    return GORSE_OK;
}
extern "C" void gorse_hip_test_set_variant(int32_t v) {
    g_variant = v & (GORSE_TEST_BPR_USER_RUNS | GORSE_TEST_BPR_PER_SAMPLE | GORSE_TEST_BPR_STABLE_RANK | GORSE_TEST_BPR_THREE_KERNELS |
                     GORSE_TEST_BPR_ARRIVAL_ORDER | GORSE_TEST_BPR_NO_BINS);
}
extern "C" void gorse_hip_test_set_bpr_chunk(int64_t samples) { g_chunk_override = samples; }
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
    g_store_mode = store_mode < 0 ? kDefaultStoreMode : (store_mode & 1);
}
extern "C" void gorse_hip_test_set_bpr_fold_period(int32_t ticks) { g_fold_period = ticks > 0 ? (uint32_t)ticks : kDefaultFoldPeriod; }
extern "C" void gorse_hip_test_set_bpr_acc_fold_every(int32_t periods) { g_acc_fold_every = periods > 0 ? periods : kDefaultAccFoldEvery; }
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
extern "C" void gorse_hip_test_set_bpr_folder_timeout(int64_t ticks) { g_folder_timeout = ticks > 0 ? (uint64_t)ticks : kFolderTimeout; }
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
    GORSE_TRY(ensure_trip(h, n));
    GORSE_TRY(mf_sync_streams(h));
    const int64_t cap = (int64_t)h->trip_cap;
    for (int64_t s0 = 0; s0 < n; s0 += cap) {
        const int64_t m = std::min(cap, n - s0);
        int32_t *tb = h->trip[0].p;
        GORSE_TRY(launch_sampler(h, seed, epoch, sample_base + s0, m, tb, (size_t)cap, h->stream));
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
    GORSE_TRY(ensure_trip(h, n));
    if (n < 0 || n > (int64_t)h->trip_cap) return fail(GORSE_ERR_INVALID, "n outside one chunk (%zu samples)", h->trip_cap);
    if (!user_runs_supported(h)) return fail(GORSE_ERR_INVALID, "this handle does not run the user-run schedule");
    GORSE_TRY(ensure_user_sort(h));
    GORSE_TRY(mf_sync_streams(h));
    const size_t cap = h->trip_cap;
    GORSE_TRY(launch_prepare_users(h, seed, epoch, sample_base, n, h->trip[0].p, h->sorted[0].p, h->ubucket[0].p, h->urank[0].p, cap,
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
    GORSE_TRY(ensure_trip(h, n));
    GORSE_TRY(mf_sync_streams(h));
    const int64_t cap = (int64_t)h->trip_cap;
    for (int64_t s0 = 0; s0 < n; s0 += cap) {
        const int64_t m = std::min(cap, n - s0);
        int32_t *tb = h->trip[0].p;
        GORSE_HIP_CHECK(hipMemcpyAsync(tb, u + s0, (size_t)m * 4, hipMemcpyHostToDevice, h->stream));
        GORSE_HIP_CHECK(hipMemcpyAsync(tb + cap, i + s0, (size_t)m * 4, hipMemcpyHostToDevice, h->stream));
        GORSE_HIP_CHECK(hipMemcpyAsync(tb + 2 * cap, j + s0, (size_t)m * 4, hipMemcpyHostToDevice, h->stream));
        if (mode == MODE_EXACT) {
            GORSE_TRY(run_sequential(h, tb, tb + cap, tb + 2 * cap, u + s0, i + s0, j + s0, m, lr, reg, g_exp_mode_exact,
                                     nullptr, nullptr));
        } else if ((mode == MODE_ATOMIC || mode == MODE_STORES) && user_runs_enabled() && user_runs_supported(h)) {
            GORSE_TRY(ensure_user_sort(h));
            GORSE_TRY(launch_user_sort(h, tb, h->sorted[0].p, h->ubucket[0].p, h->urank[0].p, m, (size_t)cap, h->stream));
            GORSE_TRY(launch_update_users(h, h->sorted[0].p, h->ubucket[0].p, (size_t)cap, lr, reg, g_exp_mode_exact, nullptr,
                                          h->stream, mode == MODE_STORES));
            GORSE_HIP_CHECK(hipStreamSynchronize(h->stream));
        } else {
            GORSE_TRY(launch_update(h, mode == MODE_STORES ? MODE_ATOMIC : mode, tb, tb + cap, tb + 2 * cap, nullptr, 0, m, lr, reg, 0, nullptr, h->stream));
            GORSE_HIP_CHECK(hipStreamSynchronize(h->stream));
        }
    }
    return GORSE_OK;
}
