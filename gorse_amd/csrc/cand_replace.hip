// cand_replace.hip -- replacement on a finished candidate chain: addReplacementCandidates and applyReplacementDecay
// (worker/pipeline.go:573-643) for every query of a pass at once.  The users' history rows go up once (one word per feedback:
// item * 2 + read, cand_replace_plan.hpp), and per call only the grown row pointer (8 bytes per query) comes back.
//   repl_sort_kernel        one workgroup per history row: the words sorted ascending, in LDS up to 4096 entries, in place in global
//                           memory beyond.  An item's entries are then adjacent, its positive one (if any) in front.
//   repl_mark_kernel        one wave per query walks the sorted row in chunks of 64: an entry is the row's when it is the first of its
//                           item and keep[item] != 0; such an entry is searched in the query's finished candidates (unsorted, may
//                           repeat, bounded by the pass's capacity: every lane walks them).  A flag per entry (dropped / already a
//                           candidate / to append), the replacement row's length and the grown candidate row's length per query.
//   nbr_scan_*              (csr_scan.hpp) both lengths become row pointers
//   repl_write_kernel       one wave per query: the old candidates first in their order, then the flagged entries with score bits
//                           +0.0 and stage 255; the replacement row (item, kind) by the same walk
//   repl_decay_sort_kernel  gorse_fm_rank_cand_decayed, one workgroup per list: every candidate's kind by a binary search in the query's
//                           replacement row, one double multiply, and for lists of up to 4096 entries a sort in LDS by
//                           (decay_key(final), rank_key(score), position) -- unique per entry, so the network's instability cannot show
// The grown rows are built beside the finished ones and swapped in at the end: a failure leaves the pass as it was.
#include "cand_internal.hpp"
#include "csr_scan.hpp"

using namespace gorse;

namespace {

constexpr int kReplWaves = 4;      // queries per workgroup of the wave-per-query kernels
constexpr int kReplThreads = 256;  // the workgroup-per-row kernels
constexpr int kSortLds = 4096;     // entries of the longest row or list sorted in LDS
constexpr int64_t kWaveGrid = 1024, kRowGrid = 4096;  // workgroups at most: 4096 queries in flight, the loops stride beyond

enum : uint8_t { kDropped = 0, kPresent = 1, kAbsent = 2 };

// what a list entry sorts by: the decayed double's key, then the ranker's order
struct SortKey {
    uint64_t hi, lo;
};
__device__ __forceinline__ bool above(const SortKey &a, const SortKey &b) { return a.hi > b.hi || (a.hi == b.hi && a.lo > b.lo); }
__device__ __forceinline__ bool above(uint32_t a, uint32_t b) { return a > b; }

// A bitonic network whose comparators all point the same way (the first step of a merge compares i with its mirror image), so
// entries past n count as +infinity by doing nothing: no padding is stored.  Ends behind a barrier (n > 1).
template <typename K>
__device__ __forceinline__ void repl_sort_network(K *a, int64_t n) {
    int64_t P = 1;
    while (P < n) P <<= 1;
    for (int64_t k = 2; k <= P; k <<= 1) {
        for (int64_t j = k >> 1; j > 0; j >>= 1) {
            for (int64_t i = threadIdx.x; i < P / 2; i += kReplThreads) {
                int64_t lo, hi;
                if (j == (k >> 1)) {
                    const int64_t blk = i / j, off = i - blk * j;
                    lo = blk * k + off;
                    hi = blk * k + k - 1 - off;
                } else {
                    lo = ((i & ~(j - 1)) << 1) | (i & (j - 1));
                    hi = lo | j;
                }
                if (hi < n) {
                    const K x = a[lo], y = a[hi];
                    if (above(x, y)) {
                        a[lo] = y;
                        a[hi] = x;
                    }
                }
            }
            __syncthreads();
        }
    }
}

// every history row's words sorted ascending in place; one workgroup per row
__global__ __launch_bounds__(kReplThreads) void repl_sort_kernel(int64_t nq, const int64_t *__restrict__ hptr, uint32_t *words) {
    __shared__ uint32_t sh[kSortLds];
    for (int64_t t = blockIdx.x; t < nq; t += gridDim.x) {
        const int64_t p0 = hptr[t], n = hptr[t + 1] - p0;
        if (n < 2) continue;  // the whole workgroup
        if (n <= kSortLds) {
            __syncthreads();  // the previous row's words are written back
            for (int i = threadIdx.x; i < n; i += kReplThreads) sh[i] = words[p0 + i];
            __syncthreads();
            repl_sort_network(sh, n);
            for (int i = threadIdx.x; i < n; i += kReplThreads) words[p0 + i] = sh[i];
        } else {
            repl_sort_network(words + p0, n);
        }
    }
}

struct MarkArgs {
    int64_t nq;
    const int64_t *hptr;     // the history rows, sorted
    const uint32_t *words;
    const uint8_t *keep;     // null: every item is kept
    const int64_t *fptr;     // the finished candidates
    const int32_t *f_item;
    uint8_t *flag;           // per history entry
    long long *rlen, *glen;  // nq entries each and a 0 behind them
    unsigned long long *kinds;  // [0] += positive entries of the replacement rows, [1] += read ones
};

__global__ __launch_bounds__(kReplWaves * 64) void repl_mark_kernel(const MarkArgs A) {
    const int lane = threadIdx.x & 63;
    const int64_t nw = (int64_t)gridDim.x * kReplWaves;
    unsigned long long positive = 0, read = 0;  // the same in every lane
    for (int64_t t = (int64_t)blockIdx.x * kReplWaves + (threadIdx.x >> 6); t < A.nq; t += nw) {
        const int64_t h0 = A.hptr[t], hn = A.hptr[t + 1] - h0;
        const int64_t f0 = A.fptr[t], fn = A.fptr[t + 1] - f0;
        int64_t rows = 0, absent = 0;
        for (int64_t e0 = 0; e0 < hn; e0 += 64) {
            const int64_t e = e0 + lane;
            uint32_t w = 0;
            bool kept = false;
            if (e < hn) {
                w = A.words[h0 + e];
                const bool first = e == 0 || (A.words[h0 + e - 1] >> 1) != (w >> 1);
                kept = first && !(A.keep && A.keep[w >> 1] == 0);
            }
            const int32_t item = (int32_t)(w >> 1);
            bool present = false;
            if (__any(kept))
                for (int64_t i = 0; i < fn; i++) present = present || A.f_item[f0 + i] == item;
            if (e < hn) A.flag[h0 + e] = !kept ? kDropped : present ? kPresent : kAbsent;
            rows += __popcll(__ballot(kept));
            absent += __popcll(__ballot(kept && !present));
            const int nread = __popcll(__ballot(kept && (w & 1u)));
            read += nread;
            positive += __popcll(__ballot(kept)) - nread;
        }
        if (lane == 0) {
            A.rlen[t] = rows;
            A.glen[t] = fn + absent;
            if (t == A.nq - 1) A.rlen[A.nq] = A.glen[A.nq] = 0;
        }
    }
    if (lane == 0) {
        if (positive) atomicAdd(A.kinds, positive);
        if (read) atomicAdd(A.kinds + 1, read);
    }
}

struct WriteArgs {
    int64_t nq;
    const int64_t *hptr;
    const uint32_t *words;
    const uint8_t *flag;
    const int64_t *fptr;  // the finished candidates
    const int32_t *f_item;
    const unsigned long long *f_score;
    const uint8_t *f_stage;
    const int64_t *gptr;  // the grown candidates
    int32_t *g_item;
    unsigned long long *g_score;
    uint8_t *g_stage;
    const int64_t *rptr;  // the replacement rows
    int32_t *r_item;
    uint8_t *r_kind;
};

__global__ __launch_bounds__(kReplWaves * 64) void repl_write_kernel(const WriteArgs A) {
    const int lane = threadIdx.x & 63;
    const int64_t nw = (int64_t)gridDim.x * kReplWaves;
    const unsigned long long below = ((unsigned long long)1 << lane) - 1;
    for (int64_t t = (int64_t)blockIdx.x * kReplWaves + (threadIdx.x >> 6); t < A.nq; t += nw) {
        const int64_t h0 = A.hptr[t], hn = A.hptr[t + 1] - h0;
        const int64_t f0 = A.fptr[t], fn = A.fptr[t + 1] - f0;
        const int64_t g0 = A.gptr[t], r0 = A.rptr[t];
        for (int64_t i = lane; i < fn; i += 64) {
            A.g_item[g0 + i] = A.f_item[f0 + i];
            A.g_score[g0 + i] = A.f_score[f0 + i];
            A.g_stage[g0 + i] = A.f_stage[f0 + i];
        }
        int64_t rows = 0, absent = 0;
        for (int64_t e0 = 0; e0 < hn; e0 += 64) {
            const int64_t e = e0 + lane;
            uint32_t w = 0;
            uint8_t f = kDropped;
            if (e < hn) {
                w = A.words[h0 + e];
                f = A.flag[h0 + e];
            }
            const unsigned long long kb = __ballot(f != kDropped), ab = __ballot(f == kAbsent);
            if (f != kDropped) {
                const int64_t d = r0 + rows + __popcll(kb & below);
                A.r_item[d] = (int32_t)(w >> 1);
                A.r_kind[d] = (w & 1u) ? GORSE_CAND_KIND_READ : GORSE_CAND_KIND_POSITIVE;
            }
            if (f == kAbsent) {
                const int64_t d = g0 + fn + absent + __popcll(ab & below);
                A.g_item[d] = (int32_t)(w >> 1);
                A.g_score[d] = 0;
                A.g_stage[d] = GORSE_CAND_STAGE_REPLACEMENT;
            }
            rows += __popcll(kb);
            absent += __popcll(ab);
        }
    }
}

struct DecayArgs {
    int64_t nq;
    const int64_t *fptr;
    const int32_t *f_item;
    const float *scores;
    const int64_t *rptr;  // null: no replacement rows, nothing is decayed
    const int32_t *r_item;
    const uint8_t *r_kind;
    double positive_decay, read_decay;
    int32_t cap;  // lists longer than this are left to the host
    double *fin;
    int32_t *order;
};

__global__ __launch_bounds__(kReplThreads) void repl_decay_sort_kernel(const DecayArgs A) {
    __shared__ SortKey sh[kSortLds];
    for (int64_t t = blockIdx.x; t < A.nq; t += gridDim.x) {
        const int64_t base = A.fptr[t], n = A.fptr[t + 1] - base;
        const int64_t r0 = A.rptr ? A.rptr[t] : 0, rn = A.rptr ? A.rptr[t + 1] - r0 : 0;
        const bool sorted = n <= A.cap;  // the whole workgroup
        __syncthreads();                 // the previous list's keys are read
        for (int64_t i = threadIdx.x; i < n; i += kReplThreads) {
            const int32_t item = A.f_item[base + i];
            const float s = A.scores[base + i];
            int64_t lo = 0, hi = rn;
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (A.r_item[r0 + mid] < item) lo = mid + 1;
                else hi = mid;
            }
            double v = (double)s;
            if (lo < rn && A.r_item[r0 + lo] == item) v = v * (A.r_kind[r0 + lo] == GORSE_CAND_KIND_POSITIVE ? A.positive_decay : A.read_decay);
            A.fin[base + i] = v;
            if (sorted) {
                SortKey k;
                k.hi = cand::decay_key((uint64_t)__double_as_longlong(v));
                k.lo = ((uint64_t)fm::rank_key(__float_as_uint(s)) << 32) | (uint32_t)i;
                sh[i] = k;
            }
        }
        if (!sorted) continue;
        __syncthreads();
        repl_sort_network(sh, n);
        for (int64_t i = threadIdx.x; i < n; i += kReplThreads) A.order[base + i] = (int32_t)(uint32_t)sh[i].lo;
    }
}

unsigned wave_grid(int64_t rows) { return (unsigned)std::max<int64_t>(1, std::min(ceil_div(rows, kReplWaves), kWaveGrid)); }
unsigned row_grid(int64_t rows) { return (unsigned)std::max<int64_t>(1, std::min(rows, kRowGrid)); }

template <typename T>
void exchange(DevBuf<T> &a, DevBuf<T> &b) {
    std::swap(a.p, b.p);
    std::swap(a.n, b.n);
}

float elapsed(hipEvent_t a, hipEvent_t b) {
    float ms = 0.0f;
    return hipEventElapsedTime(&ms, a, b) == hipSuccess ? ms : 0.0f;
}

}  // namespace

extern "C" int32_t gorse_cand_add_replacement(gorse_cand *c, const int64_t *hist_indptr, const int32_t *hist_items, const uint8_t *hist_kind,
                                              const uint8_t *keep) {
    const char *who = "gorse_cand_add_replacement";
    if (!c) return fail(GORSE_ERR_INVALID, "%s: handle is NULL", who);
    std::string msg;
    int32_t rc = cand::validate_replacement_pass(c->pass, &msg);
    if (rc == GORSE_OK) rc = cand::validate_history(c->pass.n_queries, hist_indptr, hist_items, hist_kind, c->n_items, &msg);
    if (rc != GORSE_OK) return fail(rc, "%s: %s", who, msg.c_str());
    GORSE_TRY(c->use());
    const int64_t nq = c->pass.n_queries, total = hist_indptr[nq], old_total = c->f_ptr_h.back();
    hipStream_t st = c->stream;

    // everything is built in buffers of the call's own and changes hands at the end
    DevBuf<int64_t> hptr, rptr, gptr;
    DevBuf<uint32_t> words;
    DevBuf<uint8_t> flag, g_stage, r_kind;
    DevBuf<int32_t> g_item, r_item;
    DevBuf<unsigned long long> g_score, kinds;
    std::vector<int64_t> gptr_h((size_t)nq + 1, 0);
    int64_t r_total = 0;
    unsigned long long kinds_h[2] = {0, 0};
    double ms = 0.0;
    GORSE_TRY(rptr.ensure((size_t)nq + 1));
    GORSE_TRY(gptr.ensure((size_t)nq + 1));
    if (nq > 0) {
        std::vector<uint32_t> words_h((size_t)total);
        for (int64_t e = 0; e < total; e++) words_h[(size_t)e] = cand::history_word(hist_items[e], hist_kind[e]);
        GORSE_TRY(hptr.ensure((size_t)nq + 1));
        GORSE_TRY(words.ensure((size_t)total));
        GORSE_TRY(flag.ensure((size_t)total));
        GORSE_TRY(kinds.ensure(2));
        const uint8_t *d_keep = nullptr;
        if (keep) {
            GORSE_TRY(c->keep.ensure((size_t)c->n_items));
            GORSE_HIP_CHECK(hipMemcpyAsync(c->keep.p, keep, (size_t)c->n_items, hipMemcpyHostToDevice, st));
            d_keep = c->keep.p;
        }
        GORSE_HIP_CHECK(hipMemcpyAsync(hptr.p, hist_indptr, (size_t)(nq + 1) * 8, hipMemcpyHostToDevice, st));
        if (total > 0) GORSE_HIP_CHECK(hipMemcpyAsync(words.p, words_h.data(), (size_t)total * 4, hipMemcpyHostToDevice, st));
        GORSE_HIP_CHECK(hipMemsetAsync(kinds.p, 0, 16, st));
        GORSE_HIP_CHECK(hipEventRecord(c->ev[0], st));
        if (total > 0) repl_sort_kernel<<<dim3(row_grid(nq)), dim3(kReplThreads), 0, st>>>(nq, hptr.p, words.p);
        const MarkArgs M{nq, hptr.p, words.p, d_keep, c->f_ptr.p, c->f_item.p, flag.p, (long long *)rptr.p, (long long *)gptr.p, kinds.p};
        repl_mark_kernel<<<dim3(wave_grid(nq)), dim3(kReplWaves * 64), 0, st>>>(M);
        GORSE_HIP_CHECK(hipGetLastError());
        GORSE_TRY(csr_exclusive_scan((long long *)rptr.p, nq + 1, c->sums, st));
        GORSE_TRY(csr_exclusive_scan((long long *)gptr.p, nq + 1, c->sums, st));
        GORSE_HIP_CHECK(hipEventRecord(c->ev[1], st));
        GORSE_HIP_CHECK(hipMemcpyAsync(gptr_h.data(), gptr.p, (size_t)(nq + 1) * 8, hipMemcpyDeviceToHost, st));
        GORSE_HIP_CHECK(hipMemcpyAsync(&r_total, rptr.p + nq, 8, hipMemcpyDeviceToHost, st));
        GORSE_HIP_CHECK(hipMemcpyAsync(kinds_h, kinds.p, 16, hipMemcpyDeviceToHost, st));
        GORSE_HIP_CHECK(hipStreamSynchronize(st));
        const int64_t g_total = gptr_h[(size_t)nq];
        GORSE_TRY(g_item.ensure((size_t)g_total));
        GORSE_TRY(g_score.ensure((size_t)g_total));
        GORSE_TRY(g_stage.ensure((size_t)g_total));
        GORSE_TRY(r_item.ensure((size_t)r_total));
        GORSE_TRY(r_kind.ensure((size_t)r_total));  // the last thing that can run out of memory
        GORSE_HIP_CHECK(hipEventRecord(c->ev[2], st));
        const WriteArgs W{nq,     hptr.p,   words.p,   flag.p,    c->f_ptr.p, c->f_item.p, c->f_score.p, c->f_stage.p,
                          gptr.p, g_item.p, g_score.p, g_stage.p, rptr.p,     r_item.p,    r_kind.p};
        repl_write_kernel<<<dim3(wave_grid(nq)), dim3(kReplWaves * 64), 0, st>>>(W);
        GORSE_HIP_CHECK(hipGetLastError());
        GORSE_HIP_CHECK(hipEventRecord(c->ev[3], st));
        GORSE_HIP_CHECK(hipStreamSynchronize(st));
        ms = (double)elapsed(c->ev[0], c->ev[1]) + (double)elapsed(c->ev[2], c->ev[3]);
    } else {
        GORSE_HIP_CHECK(hipMemsetAsync(rptr.p, 0, 8, st));
        GORSE_HIP_CHECK(hipMemsetAsync(gptr.p, 0, 8, st));
        GORSE_HIP_CHECK(hipStreamSynchronize(st));
    }
    exchange(c->f_ptr, gptr);
    exchange(c->f_item, g_item);
    exchange(c->f_score, g_score);
    exchange(c->f_stage, g_stage);
    exchange(c->r_ptr, rptr);
    exchange(c->r_item, r_item);
    exchange(c->r_kind, r_kind);
    c->f_ptr_h.swap(gptr_h);
    c->r_total = r_total;
    c->r_added = c->f_ptr_h.back() - old_total;
    c->r_positive = (int64_t)kinds_h[0], c->r_read = (int64_t)kinds_h[1];
    c->r_ms = ms;
    c->pass.replaced = true;
    return GORSE_OK;
}

extern "C" int32_t gorse_cand_get_replacement(gorse_cand *c, int64_t *indptr_out, int32_t *items_out, uint8_t *kind_out) {
    if (!c) return fail(GORSE_ERR_INVALID, "handle is NULL");
    if (!c->pass.begun || !c->pass.finished) return fail(GORSE_ERR_INVALID, "gorse_cand_get_replacement: no finished pass (gorse_cand_finish)");
    const int64_t nq = c->pass.n_queries;
    if (!c->pass.replaced) {  // no replacement stage: every row is empty
        if (indptr_out) std::fill(indptr_out, indptr_out + nq + 1, (int64_t)0);
        return GORSE_OK;
    }
    GORSE_TRY(c->use());
    if (indptr_out) GORSE_HIP_CHECK(hipMemcpyAsync(indptr_out, c->r_ptr.p, (size_t)(nq + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    if (c->r_total > 0) {
        if (items_out) GORSE_HIP_CHECK(hipMemcpyAsync(items_out, c->r_item.p, (size_t)c->r_total * 4, hipMemcpyDeviceToHost, c->stream));
        if (kind_out) GORSE_HIP_CHECK(hipMemcpyAsync(kind_out, c->r_kind.p, (size_t)c->r_total, hipMemcpyDeviceToHost, c->stream));
    }
    GORSE_HIP_CHECK(hipStreamSynchronize(c->stream));
    return GORSE_OK;
}

extern "C" int32_t gorse_cand_replacement_stats(gorse_cand *c, int64_t *n_added, int64_t *n_positive, int64_t *n_read, double *device_ms) {
    if (!c) return fail(GORSE_ERR_INVALID, "handle is NULL");
    const bool on = c->pass.begun && c->pass.replaced;
    if (n_added) *n_added = on ? c->r_added : 0;
    if (n_positive) *n_positive = on ? c->r_positive : 0;
    if (n_read) *n_read = on ? c->r_read : 0;
    if (device_ms) *device_ms = on ? c->r_ms : 0.0;
    return GORSE_OK;
}

int32_t gorse::cand_decay_sort(const gorse_cand *c, hipStream_t st, const float *scores, double positive_decay, double read_decay,
                               int32_t cap, double *fin, int32_t *order) {
    const int64_t nq = c->pass.n_queries;
    const bool rows = c->pass.replaced && c->r_total > 0;
    const DecayArgs D{nq,           c->f_ptr.p, c->f_item.p, scores, rows ? c->r_ptr.p : nullptr, c->r_item.p, c->r_kind.p, positive_decay,
                      read_decay, std::min<int32_t>(cap, kSortLds), fin, order};
    repl_decay_sort_kernel<<<dim3(row_grid(nq)), dim3(kReplThreads), 0, st>>>(D);
    GORSE_HIP_CHECK(hipGetLastError());
    return GORSE_OK;
}
