// bpr_prepare.hip -- sampling and chunk preparation of the BPR step on gfx950.  Reference: model/cf/model.go:449-468.
//
// The sample stream itself -- which draws make sample s, in which order -- is stated once, in bpr_stream.hpp; every sampling and
// preparation kernel below composes its functions.
// Kernels per chunk of samples (the user-run schedule; bpr_launch_prepare_users runs the preparation AHEAD on its own stream, by user
// bins where the shape has them: see "the preparation by user BINS" below -- the form without bins is):
//   bpr_sample_user_kernel : model.go:452-458 -- sample s draws its USER from the counter-based Philox stream of sample s and
//                            takes its rank in that user's run.
//   scan + bpr_scatter_ids : counting sort of the chunk's SAMPLE IDS by user (the order in which a Hogwild epoch applies its
//                            samples is free: parallel.go:44-68).
//   bpr_sample_items_kernel: model.go:459-468 -- one thread per sorted position replays its sample's stream and draws the
//                            positive and the negative; (i, j) are written in sorted order.
// Other schedules:
//   bpr_sample_kernel      : model.go:449-468 -- one thread per sample draws the whole triplet (the same stream): the
//                            per-sample and sequential schedules, gorse_bpr_sample_triplets.
//   bpr_rank / bpr_scatter_by : counting sort of whole triplets by user (bpr_launch_user_sort: gorse_bpr_apply_triplets,
//                            GORSE_TEST_BPR_STABLE_RANK).
// Which route a chunk takes, the flat kernels' grid and the scan's form are bpr_plan.hpp's rules (bpr_prep_route, bpr_flat_grid,
// bpr_scan_one_workgroup); the bins' geometry is bpr_bins.hpp's.
#include "bpr_internal.hpp"
#include <utility>

using namespace gorse;

namespace {

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
// (kFinCap, kFinStage, kFinShift: bpr_plan.hpp, where the rule that sends a chunk here reads them)
constexpr int kFinThreads = 512;
constexpr int kFinPer = kFinCap / kFinThreads;     // pairs a thread holds in registers between the count and the placement
constexpr int kFinUsers = 1 << kFinShift;          // user ids per bin at most (one thread each in the scan)
#ifndef GORSE_BPR_STAGE_ROWS
// make ab AB=no_stage AB_SRC=bpr_prepare AB_FLAGS=-DGORSE_BPR_STAGE_ROWS=0
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

// ---- counting sort by user ---------------------------------------------------------------------
// (kScanTile: bpr_plan.hpp)

// first pass of the counting sort of whole triplets (launch_user_sort: gorse_bpr_apply_triplets, GORSE_TEST_BPR_STABLE_RANK):
// rank[s] = arrival rank of sample s among the samples of its key; keys < 0 (skipped samples) count under key K
__global__ __launch_bounds__(256) void bpr_rank_kernel(const int32_t *__restrict__ key, int64_t n, int32_t K,
                                                       int32_t *__restrict__ bucket, int32_t *__restrict__ rank) {
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n; s += (int64_t)gridDim.x * blockDim.x)
        rank[s] = atomicAdd(&bucket[key[s] < 0 ? K : key[s]], 1);
}

// exclusive scan of data[0..m) in place, three launches: tile sums, scan of the tile sums, tile rescans (the block-wide scan of the
// 256 threads is block_exclusive_scan<4> above)
__global__ __launch_bounds__(256) void scan_tile_sums_kernel(const int32_t *__restrict__ data, int64_t m,
                                                             int32_t *__restrict__ sums) {
    __shared__ int32_t lds[4];
    const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * 8;
    int32_t v = 0;
#pragma unroll
    for (int e = 0; e < 8; e++)
        if (base + e < m) v += data[base + e];
    int32_t total;
    (void)block_exclusive_scan<4>(v, lds, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void scan_sums_kernel(int32_t *__restrict__ sums, int64_t nt) {
    __shared__ int32_t lds[4];
    int32_t carry = 0;
    for (int64_t t0 = 0; t0 < nt; t0 += 256) {
        const int64_t t = t0 + threadIdx.x;
        const int32_t v = t < nt ? sums[t] : 0;
        int32_t total;
        const int32_t ex = block_exclusive_scan<4>(v, lds, &total);
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
    int32_t run = sums[blockIdx.x] + block_exclusive_scan<4>(v, lds, nullptr);
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
        int32_t run = carry + block_exclusive_scan<4>(v, lds, &total);
#pragma unroll
        for (int e = 0; e < 8; e++) {
            if (base + e < m) data[base + e] = run;
            run += x[e];
        }
        carry += total;
    }
}

int32_t exclusive_scan_i32(int32_t *data, int64_t m, int32_t *tmp, hipStream_t st) {
    if (bpr_scan_one_workgroup(m)) {
        scan_small_kernel<<<dim3(1), dim3(256), 0, st>>>(data, m);
        GORSE_HIP_CHECK(hipGetLastError());
        return GORSE_OK;
    }
    const int64_t nt = bpr_scan_tiles(m);
    scan_tile_sums_kernel<<<dim3((unsigned)nt), dim3(256), 0, st>>>(data, m, tmp);
    scan_sums_kernel<<<dim3(1), dim3(256), 0, st>>>(tmp, nt);
    scan_apply_kernel<<<dim3((unsigned)nt), dim3(256), 0, st>>>(data, m, tmp);
    GORSE_HIP_CHECK(hipGetLastError());
    return GORSE_OK;
}

}  // namespace

// counting sort of the chunk's triplets by user: `sorted` receives su | si | sj, bucket[0..U] the run offsets
int32_t gorse::bpr_launch_user_sort(gorse_mf *h, const int32_t *trip, int32_t *sorted, int32_t *bucket, int32_t *rank, int64_t n, size_t cap,
                                    hipStream_t st) {
    const int64_t m = h->U + 2;  // one counter per user + one for skipped samples (sorted last) + the end offset
    const int64_t blocks = bpr_flat_grid(n);
    GORSE_HIP_CHECK(hipMemsetAsync(bucket, 0, (size_t)m * sizeof(int32_t), st));
    // key = user, skipped samples (u < 0) get key U; GORSE_TEST_BPR_STABLE_RANK: one thread ranks the samples in stream order
    if (g_bpr.variant & GORSE_TEST_BPR_STABLE_RANK)
        bpr_rank_kernel<<<dim3(1), dim3(1), 0, st>>>(trip, n, (int32_t)h->U, bucket, rank);
    else
        bpr_rank_kernel<<<dim3((unsigned)blocks), dim3(kFlatThreads), 0, st>>>(trip, n, (int32_t)h->U, bucket, rank);
    GORSE_TRY(exclusive_scan_i32(bucket, m, h->scan_tmp2.p, st));
    bpr_scatter_by_kernel<<<dim3((unsigned)blocks), dim3(kFlatThreads), 0, st>>>(trip, trip, trip + cap, trip + 2 * cap, n,
                                                                                (int32_t)h->U, bucket, rank, sorted,
                                                                                sorted + cap, sorted + 2 * cap);
    GORSE_HIP_CHECK(hipGetLastError());
    return GORSE_OK;
}
int32_t gorse::bpr_ensure_user_sort(gorse_mf *h) {
    const int64_t m = h->U + 2;
    // the tile x bin matrix of the binned preparation: prep_bins gives a chunk at most max(512, cap / 65536) tiles and min(kMaxBins - 1, U + 1) bins
    const size_t mat = prep_matrix_words(h->U, (int64_t)h->trip_cap);
    if ((size_t)m <= h->ubucket[0].n && h->scan_tmp2.n >= (size_t)bpr_scan_tiles(m) && h->urank[0].n >= 2 * h->trip_cap &&
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
    if (h->scan_tmp2.n < (size_t)bpr_scan_tiles(m)) GORSE_TRY(h->scan_tmp2.alloc((size_t)bpr_scan_tiles(m)));
    return GORSE_OK;
}

int32_t gorse::bpr_launch_sampler(gorse_mf *h, uint64_t seed, uint64_t epoch, int64_t base, int64_t n, int32_t *trip, size_t cap,
                                  hipStream_t st, hipEvent_t start, hipEvent_t stop) {
    if (n <= 0) return GORSE_OK;
    int64_t blocks = bpr_flat_grid(n);
    hipExtLaunchKernelGGL(bpr_sample_kernel, dim3((unsigned)blocks), dim3(kFlatThreads), 0, st, start, stop, 0, (int32_t)h->U, (int32_t)h->I,
                          h->uptr.p, h->uidx.p, h->uidx_sorted.p, seed, epoch, base, n, trip, trip + cap, trip + 2 * cap,
                          h->fail_count.p);
    GORSE_HIP_CHECK(hipGetLastError());
    return GORSE_OK;
}

// The user-run schedule's preparation of one chunk (see bpr_sample_user_kernel): user draws + ranks, scan of the run counters,
// sample ids scattered to their sorted positions, item draws by run.  `trip` (3 x cap ints, otherwise the unsorted triplets)
// holds the keys and (sample id, user) pairs; `rank` (2 x cap) the ranks or the sorted pairs; `sorted` receives si at cap, sj at
// 2 cap; bucket[0..U + 1] the run offsets.
// (PrepBins / prep_bins: csrc/bpr_bins.hpp, shared with the CPU cover test; which route a chunk takes: bpr_plan.hpp bpr_prep_route)
int32_t gorse::bpr_launch_prepare_users(gorse_mf *h, uint64_t seed, uint64_t epoch, int64_t base, int64_t n, int32_t *trip, int32_t *sorted,
                                        int32_t *bucket, int32_t *rank, size_t cap, hipStream_t st) {
    if (n <= 0) return GORSE_OK;
    const int64_t m = h->U + 2;
    const int64_t blocks = bpr_flat_grid(n);
    const BprPrepRoute route = bpr_prep_route(h->U, n, h->uidx.n, g_bpr.variant);
    const PrepBins &pb = route.pb;
    // the profile's spans of this chain are bound to their kernels (KernelProfile::events): a span of one kernel is that launch's start
    // and stop event, a span of several the start of its first and the stop of its last -- no marker packet on the preparation stream
    hipEvent_t ev_a = nullptr, ev_b = nullptr;
    // the item draws: four positions per thread where the users' rows cannot all sit in the L2s (see bpr_sample_items_batch_kernel)
    auto launch_items = [&](const int2 *pairs) {
        h->prof.events(GORSE_PROF_BPR_SAMPLE, &ev_a, &ev_b);
        if (route.batch_items)
            hipExtLaunchKernelGGL(bpr_sample_items_batch_kernel, dim3((unsigned)blocks), dim3(kFlatThreads), 0, st, ev_a, ev_b, 0, (int32_t)h->U,
                                  (int32_t)h->I, h->uptr.p, h->uidx.p, h->uidx_sorted.p, seed, epoch, base, n, pairs, sorted + cap,
                                  sorted + 2 * cap, h->fail_count.p);
        else
            hipExtLaunchKernelGGL(bpr_sample_items_kernel, dim3((unsigned)blocks), dim3(kFlatThreads), 0, st, ev_a, ev_b, 0, (int32_t)h->U,
                                  (int32_t)h->I, h->uptr.p, h->uidx.p, h->uidx_sorted.p, seed, epoch, base, n, pairs, sorted + cap,
                                  sorted + 2 * cap, h->fail_count.p);
    };
    // equal positives of a run next to each other (bpr_group_positives_kernel): one wave per run, in place
    auto launch_group = [&]() {
        if (g_bpr.variant & GORSE_TEST_BPR_ARRIVAL_ORDER) return;
        h->prof.events(GORSE_PROF_BPR_SORT, &ev_a, &ev_b);
        hipExtLaunchKernelGGL(bpr_group_positives_kernel, dim3((unsigned)std::min<int64_t>(h->U, 256 * 16)), dim3(64), 0, st, ev_a, ev_b, 0,
                              (int32_t)h->U, bucket, sorted + cap, sorted + 2 * cap);
    };
    if (route.binned) {
        int32_t *key = trip;
        int2 *bp = reinterpret_cast<int2 *>(trip + cap), *pairs = reinterpret_cast<int2 *>(rank);  // (rank: 2 x cap words, ensure_user_sort)
        int32_t *bin_count = h->ubins.p, *bin_start = h->ubins.p + kMaxBins, *H = h->ubinmat.p;
        const unsigned tiles = (unsigned)ceil_div(n, pb.tile);
        if ((size_t)tiles * pb.nbins > h->ubinmat.n) return fail(GORSE_ERR_INVALID, "tile x bin matrix smaller than %u x %d", tiles, pb.nbins);
        const bool finish = route.finish;  // the bins in one LDS-resident pass (bpr_bin_finish_kernel), else the three kernels
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
                                  pairs, sorted + cap, sorted + 2 * cap, h->fail_count.p, (g_bpr.variant & GORSE_TEST_BPR_ARRIVAL_ORDER) ? 0 : 1);
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
    bpr_sample_user_kernel<<<dim3((unsigned)blocks), dim3(kFlatThreads), 0, st>>>((int32_t)h->U, h->uptr.p, seed, epoch, base, n, key,
                                                                                  h->fail_count.p, bucket, rank);
    h->prof.end(tok, st);
    tok = h->prof.begin(GORSE_PROF_BPR_SORT, st);
    GORSE_TRY(exclusive_scan_i32(bucket, m, h->scan_tmp2.p, st));
    bpr_scatter_ids_kernel<<<dim3((unsigned)blocks), dim3(kFlatThreads), 0, st>>>(key, rank, bucket, n, (int32_t)h->U, pairs);
    h->prof.end(tok, st);
    launch_items(pairs);
    launch_group();
    GORSE_HIP_CHECK(hipGetLastError());
    return GORSE_OK;
}

int32_t gorse::bpr_ensure_trip(gorse_mf *h, int64_t want) {
    const size_t cap = bpr_trip_capacity(want, bpr_chunk_capacity(h->U, g_bpr.chunk_override));
    if (cap <= h->trip_cap) return GORSE_OK;
    GORSE_TRY(mf_sync_streams(h));
    for (int b = 0; b < 2; b++) GORSE_TRY(h->trip[b].alloc(cap * 3));
    for (int b = 0; b < 2; b++) GORSE_TRY(h->sorted[b].alloc(cap * 3));
    h->trip_cap = cap;
    return GORSE_OK;
}
