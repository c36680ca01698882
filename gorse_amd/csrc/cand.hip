// cand.hip -- gorse_cand, the candidate chain: RecommendSequential (logics/recommend.go:135-156) with limit = 0 for many users at
// once, as the worker's offline pass runs it (worker/pipeline.go:124-306).  The exclusion rows and the candidate rows stay on the
// device for the whole pass; the stages that exist as device calls (gorse_mf_recommend, gorse_nbr_recommend) read their seen rows
// from the chain and leave their result rows on the device, the list recommenders are a filter, and per stage only the new row
// pointer (8 bytes per query) comes back.
//
// The current exclusion rows are a compact CSR with ascending rows -- the form rec_fast_kernel / rec_candidates_kernel
// (recommend.hip) and nbr_walk_kernel (nbr_recommend.hip) read -- rebuilt after every stage into the other of two buffers:
//   cand_sort_kernel      begin: every base row sorted ascending, in LDS up to 4096 entries, in place in global memory beyond
//   cand_filter_kernel    one wave per query walks the stage's list in chunks of 64 (one shared list, a CSR of lists, or result rows
//                         of stride k): a lane's entry is kept when its item is not in the current row (binary search) and keep[item]
//                         != 0; ballot + prefix count keep the order; the walk stops at k.  Kept entries go to a staging area of
//                         stride k, the new row length (old + kept) to the row pointer under construction.
//   nbr_scan_*            (csr_scan.hpp) the lengths become the new row pointer
//   cand_append_kernel    the staged entries behind the query's candidates, with the stage number
//   cand_merge_kernel     one workgroup per query: the <= 256 new items sorted in LDS; old element i goes to i + (new items below
//                         it), new element of rank r to r + (old items not above it) -- a stable merge, old first
//   cand_compact_kernel   finish: the candidate rows filtered by keep into a CSR (a counting pass, the scan, a writing pass)
// The filter runs before anything of the chain is written, and the merge's buffer is sized from the scanned pointer before the
// append: a failure up to there leaves the chain as it was.
#include "cand_internal.hpp"
#include "csr_scan.hpp"
#include "mf_internal.hpp"
#include "nbr_internal.hpp"

using namespace gorse;

namespace {

constexpr int kCandWaves = 4;     // queries per workgroup of the wave-per-query kernels
constexpr int kMergeThreads = 256;
constexpr int kSortLds = 4096;    // entries of the longest row sorted in LDS
constexpr int64_t kMaxGrid = (int64_t)1 << 20;

struct FilterArgs {
    const int32_t *items;               // shared: the list; lists: the CSR's items; rows: n_queries rows of `stride` entries
    const unsigned long long *score64;  // the scores' bits ...
    const float *score32;               // ... or floats to widen (gorse_mf_recommend's rows)
    const int64_t *lptr;                // lists: the CSR's row pointer
    const int32_t *cnt;                 // rows: the entries of row t
    int64_t n_list;                     // shared: the list's length; rows: the stride
    const int64_t *xptr;                // the current exclusion rows
    const int32_t *xitems;
    int32_t check;                      // 0: the stage excluded by itself (gorse_nbr_recommend's walk)
    const uint8_t *keep;                // null: every item is kept
    int64_t nq;
    int32_t k;
    int32_t *st_item;
    unsigned long long *st_score;
    int32_t *st_cnt;
    long long *newlen;                  // old row length + kept, nq entries, and a 0 behind them
};

// is v in the ascending row x[0 .. n)
__device__ __forceinline__ bool cand_in_row(const int32_t *__restrict__ x, int64_t n, int32_t v) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (x[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && x[lo] == v;
}

__global__ __launch_bounds__(kCandWaves * 64) void cand_filter_kernel(const FilterArgs A) {
    const int lane = threadIdx.x & 63;
    const int64_t nw = (int64_t)gridDim.x * kCandWaves;
    for (int64_t t = (int64_t)blockIdx.x * kCandWaves + (threadIdx.x >> 6); t < A.nq; t += nw) {
        int64_t o = 0, c = A.n_list;
        if (A.lptr) {
            o = A.lptr[t];
            c = A.lptr[t + 1] - o;
        } else if (A.cnt) {
            o = t * A.n_list;
            c = min((int64_t)max(A.cnt[t], 0), A.n_list);
        }
        const int64_t x0 = A.xptr[t], xn = A.xptr[t + 1] - x0;
        int kept = 0;  // the same in every lane
        for (int64_t e0 = 0; e0 < c && kept < A.k; e0 += 64) {
            const int64_t e = e0 + lane;
            int32_t j = -1;
            bool keep = false;
            if (e < c) {
                j = A.items[o + e];
                keep = j >= 0 && !(A.check && cand_in_row(A.xitems + x0, xn, j)) && !(A.keep && A.keep[j] == 0);
            }
            const unsigned long long b = __ballot(keep);
            const int pos = kept + __popcll(b & (((unsigned long long)1 << lane) - 1));
            if (keep && pos < A.k) {
                A.st_item[t * A.k + pos] = j;
                A.st_score[t * A.k + pos] = A.score64 ? A.score64[o + e]
                                                      : (unsigned long long)__double_as_longlong((double)A.score32[o + e]);
            }
            kept += __popcll(b);
        }
        if (lane == 0) {
            kept = min(kept, A.k);
            A.st_cnt[t] = kept;
            A.newlen[t] = xn + kept;
            if (t == A.nq - 1) A.newlen[A.nq] = 0;
        }
    }
}

// the staged entries of every query behind its candidates; one wave per query
__global__ __launch_bounds__(kCandWaves * 64) void cand_append_kernel(int64_t nq, int32_t k, int32_t capacity, int32_t stage,
                                                                      const int32_t *__restrict__ st_item,
                                                                      const unsigned long long *__restrict__ st_score,
                                                                      const int32_t *__restrict__ st_cnt, int32_t *__restrict__ c_item,
                                                                      unsigned long long *__restrict__ c_score, uint8_t *__restrict__ c_stage,
                                                                      int32_t *c_cnt) {
    const int lane = threadIdx.x & 63;
    const int64_t nw = (int64_t)gridDim.x * kCandWaves;
    for (int64_t t = (int64_t)blockIdx.x * kCandWaves + (threadIdx.x >> 6); t < nq; t += nw) {
        const int m = st_cnt[t], have = c_cnt[t];
        const int room = max(min(m, capacity - have), 0);  // (always m: the stages' k add up to the capacity at most)
        for (int e = lane; e < room; e += 64) {
            const int64_t d = t * capacity + have + e;
            c_item[d] = st_item[t * k + e];
            c_score[d] = st_score[t * k + e];
            c_stage[d] = (uint8_t)stage;
        }
        if (lane == 0) c_cnt[t] = have + room;  // (every lane has read it: one wave, in order)
    }
}

// out row t = old row t merged with the query's staged items, ascending, repeats kept; one workgroup per query
__global__ __launch_bounds__(kMergeThreads) void cand_merge_kernel(int64_t nq, int32_t k, const int64_t *__restrict__ optr,
                                                                   const int32_t *__restrict__ old, const int64_t *__restrict__ nptr,
                                                                   const int32_t *__restrict__ st_item, const int32_t *__restrict__ st_cnt,
                                                                   int32_t *__restrict__ out) {
    __shared__ int32_t raw[GORSE_CAND_MAX_K], srt[GORSE_CAND_MAX_K];
    const int tid = threadIdx.x;
    for (int64_t t = blockIdx.x; t < nq; t += gridDim.x) {
        const int m = min(st_cnt[t], GORSE_CAND_MAX_K);
        const int64_t o0 = optr[t], on = optr[t + 1] - o0, d0 = nptr[t];
        __syncthreads();  // the previous query's srt is read
        for (int e = tid; e < m; e += kMergeThreads) raw[e] = st_item[t * k + e];
        __syncthreads();
        for (int e = tid; e < m; e += kMergeThreads) {
            const int32_t v = raw[e];
            int rank = 0;
            for (int x = 0; x < m; x++) rank += (raw[x] < v || (raw[x] == v && x < e)) ? 1 : 0;
            srt[rank] = v;
        }
        __syncthreads();
        for (int64_t i = tid; i < on; i += kMergeThreads) {
            const int32_t v = old[o0 + i];
            int lo = 0, hi = m;  // the new items below v
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (srt[mid] < v) lo = mid + 1;
                else hi = mid;
            }
            out[d0 + i + lo] = v;
        }
        for (int e = tid; e < m; e += kMergeThreads) {
            const int32_t v = srt[e];
            int64_t lo = 0, hi = on;  // the old items not above v: equal ones stay in front
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (old[o0 + mid] <= v) lo = mid + 1;
                else hi = mid;
            }
            out[d0 + e + lo] = v;
        }
    }
}

// A bitonic network whose comparators all point the same way (the first step of a merge compares i with its mirror image), so
// entries past n count as +infinity by doing nothing: no padding is stored.  Ends behind a barrier.
template <int T>
__device__ __forceinline__ void cand_sort_network(int32_t *a, int64_t n) {
    int64_t P = 1;
    while (P < n) P <<= 1;
    for (int64_t k = 2; k <= P; k <<= 1) {
        for (int64_t j = k >> 1; j > 0; j >>= 1) {
            for (int64_t i = threadIdx.x; i < P / 2; i += T) {
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
                    const int32_t x = a[lo], y = a[hi];
                    if (x > y) {
                        a[lo] = y;
                        a[hi] = x;
                    }
                }
            }
            __syncthreads();
        }
    }
}

// every row of a CSR sorted ascending in place; one workgroup per row
__global__ __launch_bounds__(kMergeThreads) void cand_sort_kernel(int64_t nq, const int64_t *__restrict__ ptr, int32_t *items) {
    __shared__ int32_t sh[kSortLds];
    for (int64_t t = blockIdx.x; t < nq; t += gridDim.x) {
        const int64_t p0 = ptr[t], n = ptr[t + 1] - p0;
        if (n < 2) continue;  // the whole workgroup
        if (n <= kSortLds) {
            __syncthreads();
            for (int i = threadIdx.x; i < n; i += kMergeThreads) sh[i] = items[p0 + i];
            __syncthreads();
            cand_sort_network<kMergeThreads>(sh, n);
            for (int i = threadIdx.x; i < n; i += kMergeThreads) items[p0 + i] = sh[i];
        } else {
            cand_sort_network<kMergeThreads>(items + p0, n);
        }
    }
}

// finish: the candidate rows filtered by keep into a CSR.  write == 0: cnt64[t] = the survivors of row t (and a 0 behind the last);
// write != 0: the survivors in order to row fptr[t].  One wave per query.
__global__ __launch_bounds__(kCandWaves * 64) void cand_compact_kernel(int64_t nq, int32_t capacity, int32_t write,
                                                                       const int32_t *__restrict__ c_item,
                                                                       const unsigned long long *__restrict__ c_score,
                                                                       const uint8_t *__restrict__ c_stage, const int32_t *__restrict__ c_cnt,
                                                                       const uint8_t *__restrict__ keep, long long *cnt64,
                                                                       const int64_t *__restrict__ fptr, int32_t *__restrict__ f_item,
                                                                       unsigned long long *__restrict__ f_score, uint8_t *__restrict__ f_stage) {
    const int lane = threadIdx.x & 63;
    const int64_t nw = (int64_t)gridDim.x * kCandWaves;
    for (int64_t t = (int64_t)blockIdx.x * kCandWaves + (threadIdx.x >> 6); t < nq; t += nw) {
        const int c = min(max(c_cnt[t], 0), capacity);
        const int64_t d0 = write ? fptr[t] : 0;
        int kept = 0;
        for (int e0 = 0; e0 < c; e0 += 64) {
            const int e = e0 + lane;
            int32_t j = -1;
            if (e < c) j = c_item[t * capacity + e];
            const bool ok = j >= 0 && !(keep && keep[j] == 0);
            const unsigned long long b = __ballot(ok);
            if (write && ok) {
                const int64_t d = d0 + kept + __popcll(b & (((unsigned long long)1 << lane) - 1));
                f_item[d] = j;
                f_score[d] = c_score[t * capacity + e];
                f_stage[d] = c_stage[t * capacity + e];
            }
            kept += __popcll(b);
        }
        if (!write && lane == 0) {
            cnt64[t] = kept;
            if (t == nq - 1) cnt64[nq] = 0;
        }
    }
}

unsigned wave_grid(int64_t rows) { return (unsigned)std::max<int64_t>(1, std::min(ceil_div(rows, kCandWaves), kMaxGrid)); }
unsigned block_grid(int64_t rows) { return (unsigned)std::max<int64_t>(1, std::min(rows, kMaxGrid)); }

int32_t upload_keep(gorse_cand *c, const uint8_t *keep, const uint8_t **d_keep) {
    *d_keep = nullptr;
    if (!keep) return GORSE_OK;
    GORSE_TRY(c->keep.ensure((size_t)c->n_items));
    GORSE_HIP_CHECK(hipMemcpyAsync(c->keep.p, keep, (size_t)c->n_items, hipMemcpyHostToDevice, c->stream));
    *d_keep = c->keep.p;
    return GORSE_OK;
}

float elapsed(hipEvent_t a, hipEvent_t b) {
    float ms = 0.0f;
    return hipEventElapsedTime(&ms, a, b) == hipSuccess ? ms : 0.0f;
}

// One stage from its lists on the device (A.items .. A.n_list, A.check set by the caller): filter, scan, append, merge.  Everything
// the caller validates has been validated; stage_ms = the device time of the stage's own search.
int32_t run_stage(gorse_cand *c, FilterArgs A, int32_t k, const uint8_t *keep, double stage_ms) {
    const int64_t nq = c->pass.n_queries;
    const int other = 1 - c->cur;
    hipStream_t st = c->stream;
    double chain_ms = 0.0;
    if (nq > 0) {
        GORSE_TRY(c->st_item.ensure((size_t)nq * k));
        GORSE_TRY(c->st_score.ensure((size_t)nq * k));
        GORSE_TRY(c->st_cnt.ensure((size_t)nq));
        GORSE_TRY(upload_keep(c, keep, &A.keep));
        A.xptr = c->cur_ptr[c->cur].p, A.xitems = c->cur_items[c->cur].p;
        A.nq = nq, A.k = k;
        A.st_item = c->st_item.p, A.st_score = c->st_score.p, A.st_cnt = c->st_cnt.p;
        A.newlen = (long long *)c->cur_ptr[other].p;
        GORSE_HIP_CHECK(hipEventRecord(c->ev[0], st));
        cand_filter_kernel<<<dim3(wave_grid(nq)), dim3(kCandWaves * 64), 0, st>>>(A);
        GORSE_HIP_CHECK(hipGetLastError());
        GORSE_TRY(csr_exclusive_scan((long long *)c->cur_ptr[other].p, nq + 1, c->sums, st));
        GORSE_HIP_CHECK(hipEventRecord(c->ev[1], st));
        std::vector<int64_t> nptr((size_t)nq + 1);
        GORSE_HIP_CHECK(hipMemcpyAsync(nptr.data(), c->cur_ptr[other].p, (size_t)(nq + 1) * 8, hipMemcpyDeviceToHost, st));
        GORSE_HIP_CHECK(hipStreamSynchronize(st));
        GORSE_TRY(c->cur_items[other].ensure((size_t)nptr[(size_t)nq]));  // the last thing that can fail before the chain changes
        GORSE_HIP_CHECK(hipEventRecord(c->ev[2], st));
        cand_append_kernel<<<dim3(wave_grid(nq)), dim3(kCandWaves * 64), 0, st>>>(nq, k, c->pass.capacity, c->pass.n_stages, c->st_item.p,
                                                                                c->st_score.p, c->st_cnt.p, c->c_item.p, c->c_score.p,
                                                                                c->c_stage.p, c->c_cnt.p);
        cand_merge_kernel<<<dim3(block_grid(nq)), dim3(kMergeThreads), 0, st>>>(nq, k, c->cur_ptr[c->cur].p, c->cur_items[c->cur].p,
                                                                               c->cur_ptr[other].p, c->st_item.p, c->st_cnt.p,
                                                                               c->cur_items[other].p);
        GORSE_HIP_CHECK(hipGetLastError());
        GORSE_HIP_CHECK(hipEventRecord(c->ev[3], st));
        GORSE_HIP_CHECK(hipStreamSynchronize(st));
        chain_ms = (double)elapsed(c->ev[0], c->ev[1]) + (double)elapsed(c->ev[2], c->ev[3]);
        c->n_candidates += nptr[(size_t)nq] - c->cur_ptr_h[(size_t)nq];  // every kept entry went into its row
        c->cur_ptr_h.swap(nptr);
        c->cur = other;
    }
    c->pass.n_stages += 1;
    c->pass.sum_k += k;
    c->stage_ms.push_back(stage_ms);
    c->chain_ms.push_back(chain_ms);
    return GORSE_OK;
}

int32_t check_stage(gorse_cand *c, const char *who, int32_t k) {
    if (!c) return fail(GORSE_ERR_INVALID, "%s: handle is NULL", who);
    std::string msg;
    const int32_t rc = cand::validate_stage(c->pass, k, &msg);
    if (rc != GORSE_OK) return fail(rc, "%s: %s", who, msg.c_str());
    return GORSE_OK;
}

}  // namespace

extern "C" int32_t gorse_cand_create(gorse_cand **out, int32_t device, int64_t n_items) {
    if (!out) return fail(GORSE_ERR_INVALID, "handle pointer is NULL");
    *out = nullptr;
    if (n_items < 1 || n_items > INT32_MAX) return fail(GORSE_ERR_INVALID, "n_items = %lld outside 1 .. 2^31 - 1", (long long)n_items);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(GORSE_ERR_NO_DEVICE, "no HIP device visible (libgorse_hip needs an MI355X / gfx950)");
    if (device < 0 || device >= ndev) return fail(GORSE_ERR_INVALID, "device %d out of range [0,%d)", device, ndev);
    gorse_cand *c = new (std::nothrow) gorse_cand();
    if (!c) return fail(GORSE_ERR_NOMEM, "out of host memory");
    c->device = device;
    c->n_items = n_items;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    for (auto &ev : c->ev)
        if (e == hipSuccess) e = hipEventCreate(&ev);
    if (e != hipSuccess) {
        (void)gorse_cand_destroy(c);
        return fail(GORSE_ERR_HIP, "gorse_cand_create: %s", hipGetErrorString(e));
    }
    *out = c;
    return GORSE_OK;
}

extern "C" int32_t gorse_cand_destroy(gorse_cand *c) {
    if (!c) return GORSE_OK;
    (void)hipSetDevice(c->device);
    if (c->stream) {
        (void)hipStreamSynchronize(c->stream);
        (void)hipStreamDestroy(c->stream);
    }
    for (auto ev : c->ev)
        if (ev) (void)hipEventDestroy(ev);
    delete c;
    return GORSE_OK;
}

extern "C" int32_t gorse_cand_begin(gorse_cand *c, int64_t n_queries, const int64_t *excl_indptr, const int32_t *excl_items,
                                    int32_t capacity) {
    if (!c) return fail(GORSE_ERR_INVALID, "handle is NULL");
    std::string msg;
    const int32_t rc = cand::validate_begin(n_queries, excl_indptr, excl_items, capacity, c->n_items, &msg);
    if (rc != GORSE_OK) return fail(rc, "gorse_cand_begin: %s", msg.c_str());
    GORSE_TRY(c->use());
    const int64_t nq = n_queries, total = excl_indptr ? excl_indptr[nq] : 0;
    c->pass = cand::Pass();  // from here on a failure (memory, the runtime) leaves the chain without a pass
    std::vector<int64_t> ptr((size_t)nq + 1, 0);
    if (excl_indptr) ptr.assign(excl_indptr, excl_indptr + nq + 1);
    GORSE_TRY(c->base_ptr.ensure((size_t)nq + 1));
    GORSE_TRY(c->base_items.ensure((size_t)total));
    GORSE_TRY(c->cur_ptr[0].ensure((size_t)nq + 1));
    GORSE_TRY(c->cur_ptr[1].ensure((size_t)nq + 1));
    GORSE_TRY(c->cur_items[0].ensure((size_t)total));
    GORSE_TRY(c->c_item.ensure((size_t)nq * capacity));
    GORSE_TRY(c->c_score.ensure((size_t)nq * capacity));
    GORSE_TRY(c->c_stage.ensure((size_t)nq * capacity));
    GORSE_TRY(c->c_cnt.ensure((size_t)nq));
    hipStream_t st = c->stream;
    GORSE_HIP_CHECK(hipMemcpyAsync(c->base_ptr.p, ptr.data(), (size_t)(nq + 1) * 8, hipMemcpyHostToDevice, st));
    if (total > 0) {
        GORSE_HIP_CHECK(hipMemcpyAsync(c->base_items.p, excl_items, (size_t)total * 4, hipMemcpyHostToDevice, st));
        cand_sort_kernel<<<dim3(block_grid(nq)), dim3(kMergeThreads), 0, st>>>(nq, c->base_ptr.p, c->base_items.p);
        GORSE_HIP_CHECK(hipGetLastError());
        GORSE_HIP_CHECK(hipMemcpyAsync(c->cur_items[0].p, c->base_items.p, (size_t)total * 4, hipMemcpyDeviceToDevice, st));
    }
    GORSE_HIP_CHECK(hipMemcpyAsync(c->cur_ptr[0].p, c->base_ptr.p, (size_t)(nq + 1) * 8, hipMemcpyDeviceToDevice, st));
    if (nq > 0) GORSE_HIP_CHECK(hipMemsetAsync(c->c_cnt.p, 0, (size_t)nq * 4, st));
    GORSE_HIP_CHECK(hipStreamSynchronize(st));
    c->cur = 0;
    c->base_total = total;
    c->cur_ptr_h.swap(ptr);
    c->n_candidates = 0;
    c->f_ptr_h.clear();
    c->stage_ms.clear(), c->chain_ms.clear();
    c->pass.begun = true;
    c->pass.n_queries = nq, c->pass.capacity = capacity;
    return GORSE_OK;
}

extern "C" int32_t gorse_cand_add_mf(gorse_cand *c, gorse_mf *mf, const int32_t *users, int32_t k, const uint8_t *item_ok,
                                     const uint8_t *keep) {
    const char *who = "gorse_cand_add_mf";
    GORSE_TRY(check_stage(c, who, k));
    if (!mf) return fail(GORSE_ERR_INVALID, "%s: the model handle is NULL", who);
    if (mf->device != c->device) return fail(GORSE_ERR_INVALID, "%s: the model is on device %d, the chain on device %d", who, mf->device, c->device);
    if (mf->I != c->n_items)
        return fail(GORSE_ERR_INVALID, "%s: the model has %lld items, the chain %lld", who, (long long)mf->I, (long long)c->n_items);
    const int64_t nq = c->pass.n_queries;
    GORSE_TRY(mf_recommend_check(mf, nq, users, k));
    GORSE_TRY(c->use());
    GORSE_TRY(c->mf_items.ensure((size_t)nq * k));
    GORSE_TRY(c->mf_scores.ensure((size_t)nq * k));
    GORSE_TRY(c->mf_cnt.ensure((size_t)nq));
    // the search runs under the BASE rows (pipeline.go:200 takes the exclude set before RecommendSequential has added anything) ...
    MfDeviceRows rows{c->mf_items.p, c->mf_scores.p, c->mf_cnt.p};
    GORSE_TRY(mf_recommend_core(mf, nq, users, k, item_ok, c->base_total > 0 ? c->base_ptr.p : nullptr, c->base_items.p, nullptr, nullptr,
                                nullptr, &rows));
    GORSE_TRY(c->use());
    // ... and the filter applies the current ones
    FilterArgs A{};
    A.items = c->mf_items.p, A.score32 = c->mf_scores.p, A.cnt = c->mf_cnt.p, A.n_list = k, A.check = 1;
    return run_stage(c, A, k, keep, mf->rec_ms);
}

extern "C" int32_t gorse_cand_add_nbr(gorse_cand *c, gorse_nbr *nbr, const int32_t *rows, int32_t k, const uint8_t *keep) {
    const char *who = "gorse_cand_add_nbr";
    GORSE_TRY(check_stage(c, who, k));
    if (!nbr) return fail(GORSE_ERR_INVALID, "%s: the neighbourhood handle is NULL", who);
    if (nbr->device != c->device)
        return fail(GORSE_ERR_INVALID, "%s: the tables are on device %d, the chain on device %d", who, nbr->device, c->device);
    if (nbr->n_items != c->n_items)
        return fail(GORSE_ERR_INVALID, "%s: the tables have %lld items, the chain %lld", who, (long long)nbr->n_items, (long long)c->n_items);
    const int64_t nq = c->pass.n_queries;
    GORSE_TRY(nbr_recommend_check(nbr, who, nq, rows, k, nullptr, nullptr));
    // the walk excludes by the current rows itself, as recommendItemToItem does
    const bool has_seen = nq > 0 && c->cur_ptr_h[(size_t)nq] > 0;
    NbrDeviceRows R;
    GORSE_TRY(nbr_recommend_core(nbr, nq, rows, k, has_seen ? c->cur_ptr_h.data() : nullptr, c->cur_ptr[c->cur].p, c->cur_items[c->cur].p, &R));
    GORSE_TRY(c->use());
    FilterArgs A{};
    A.items = R.items, A.score64 = R.sums, A.cnt = R.cnt, A.n_list = k, A.check = 0;
    return run_stage(c, A, k, keep, nbr->ms);
}

extern "C" int32_t gorse_cand_add_shared(gorse_cand *c, int64_t n_list, const int32_t *items, const double *scores, int32_t k,
                                         const uint8_t *keep) {
    const char *who = "gorse_cand_add_shared";
    GORSE_TRY(check_stage(c, who, k));
    std::string msg;
    const int32_t rc = cand::validate_shared(n_list, items, scores, c->n_items, &msg);
    if (rc != GORSE_OK) return fail(rc, "%s: %s", who, msg.c_str());
    GORSE_TRY(c->use());
    GORSE_TRY(c->l_items.ensure((size_t)n_list));
    GORSE_TRY(c->l_scores.ensure((size_t)n_list));
    if (n_list > 0) {
        GORSE_HIP_CHECK(hipMemcpyAsync(c->l_items.p, items, (size_t)n_list * 4, hipMemcpyHostToDevice, c->stream));
        GORSE_HIP_CHECK(hipMemcpyAsync(c->l_scores.p, scores, (size_t)n_list * 8, hipMemcpyHostToDevice, c->stream));
    }
    FilterArgs A{};
    A.items = c->l_items.p, A.score64 = c->l_scores.p, A.n_list = n_list, A.check = 1;
    return run_stage(c, A, k, keep, 0.0);
}

extern "C" int32_t gorse_cand_add_lists(gorse_cand *c, const int64_t *indptr, const int32_t *items, const double *scores, int32_t k,
                                        const uint8_t *keep) {
    const char *who = "gorse_cand_add_lists";
    GORSE_TRY(check_stage(c, who, k));
    const int64_t nq = c->pass.n_queries;
    std::string msg;
    const int32_t rc = cand::validate_lists(nq, indptr, items, scores, c->n_items, &msg);
    if (rc != GORSE_OK) return fail(rc, "%s: %s", who, msg.c_str());
    GORSE_TRY(c->use());
    const int64_t n = indptr[nq];
    GORSE_TRY(c->l_ptr.ensure((size_t)nq + 1));
    GORSE_TRY(c->l_items.ensure((size_t)n));
    GORSE_TRY(c->l_scores.ensure((size_t)n));
    GORSE_HIP_CHECK(hipMemcpyAsync(c->l_ptr.p, indptr, (size_t)(nq + 1) * 8, hipMemcpyHostToDevice, c->stream));
    if (n > 0) {
        GORSE_HIP_CHECK(hipMemcpyAsync(c->l_items.p, items, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
        GORSE_HIP_CHECK(hipMemcpyAsync(c->l_scores.p, scores, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    }
    FilterArgs A{};
    A.items = c->l_items.p, A.score64 = c->l_scores.p, A.lptr = c->l_ptr.p, A.check = 1;
    return run_stage(c, A, k, keep, 0.0);
}

extern "C" int32_t gorse_cand_finish(gorse_cand *c, const uint8_t *keep) {
    if (!c) return fail(GORSE_ERR_INVALID, "handle is NULL");
    if (!c->pass.begun) return fail(GORSE_ERR_INVALID, "gorse_cand_finish: no pass begun (gorse_cand_begin)");
    if (c->pass.finished) return fail(GORSE_ERR_INVALID, "gorse_cand_finish: the pass is finished already");
    GORSE_TRY(c->use());
    const int64_t nq = c->pass.n_queries;
    hipStream_t st = c->stream;
    std::vector<int64_t> fptr((size_t)nq + 1, 0);
    GORSE_TRY(c->f_ptr.ensure((size_t)nq + 1));
    if (nq > 0) {
        const uint8_t *d_keep = nullptr;
        GORSE_TRY(upload_keep(c, keep, &d_keep));
        const dim3 grid(wave_grid(nq)), block(kCandWaves * 64);
        cand_compact_kernel<<<grid, block, 0, st>>>(nq, c->pass.capacity, 0, c->c_item.p, c->c_score.p, c->c_stage.p, c->c_cnt.p, d_keep,
                                                    (long long *)c->f_ptr.p, nullptr, nullptr, nullptr, nullptr);
        GORSE_HIP_CHECK(hipGetLastError());
        GORSE_TRY(csr_exclusive_scan((long long *)c->f_ptr.p, nq + 1, c->sums, st));
        GORSE_HIP_CHECK(hipMemcpyAsync(fptr.data(), c->f_ptr.p, (size_t)(nq + 1) * 8, hipMemcpyDeviceToHost, st));
        GORSE_HIP_CHECK(hipStreamSynchronize(st));
        const int64_t total = fptr[(size_t)nq];
        GORSE_TRY(c->f_item.ensure((size_t)total));
        GORSE_TRY(c->f_score.ensure((size_t)total));
        GORSE_TRY(c->f_stage.ensure((size_t)total));
        cand_compact_kernel<<<grid, block, 0, st>>>(nq, c->pass.capacity, 1, c->c_item.p, c->c_score.p, c->c_stage.p, c->c_cnt.p, d_keep,
                                                    nullptr, c->f_ptr.p, c->f_item.p, c->f_score.p, c->f_stage.p);
        GORSE_HIP_CHECK(hipGetLastError());
        GORSE_HIP_CHECK(hipStreamSynchronize(st));
    } else {
        GORSE_HIP_CHECK(hipMemsetAsync(c->f_ptr.p, 0, 8, st));
        GORSE_HIP_CHECK(hipStreamSynchronize(st));
    }
    c->f_ptr_h.swap(fptr);
    c->pass.finished = true;
    return GORSE_OK;
}

extern "C" int32_t gorse_cand_info(gorse_cand *c, int64_t *n_queries, int32_t *n_stages, int64_t *n_candidates, int64_t *n_excluded) {
    if (!c) return fail(GORSE_ERR_INVALID, "handle is NULL");
    const bool on = c->pass.begun;
    if (n_queries) *n_queries = on ? c->pass.n_queries : 0;
    if (n_stages) *n_stages = on ? c->pass.n_stages : 0;
    if (n_candidates) *n_candidates = !on ? 0 : c->pass.finished ? c->f_ptr_h.back() : c->n_candidates;
    if (n_excluded) *n_excluded = on ? c->cur_ptr_h.back() : 0;
    return GORSE_OK;
}

extern "C" int32_t gorse_cand_get(gorse_cand *c, int64_t *indptr_out, int32_t *items_out, double *scores_out, uint8_t *stage_out) {
    if (!c) return fail(GORSE_ERR_INVALID, "handle is NULL");
    if (!c->pass.begun || !c->pass.finished) return fail(GORSE_ERR_INVALID, "gorse_cand_get: no finished pass (gorse_cand_finish)");
    GORSE_TRY(c->use());
    const int64_t total = c->f_ptr_h.back();
    if (indptr_out) std::copy(c->f_ptr_h.begin(), c->f_ptr_h.end(), indptr_out);
    if (total > 0) {
        if (items_out) GORSE_HIP_CHECK(hipMemcpyAsync(items_out, c->f_item.p, (size_t)total * 4, hipMemcpyDeviceToHost, c->stream));
        if (scores_out) GORSE_HIP_CHECK(hipMemcpyAsync(scores_out, c->f_score.p, (size_t)total * 8, hipMemcpyDeviceToHost, c->stream));
        if (stage_out) GORSE_HIP_CHECK(hipMemcpyAsync(stage_out, c->f_stage.p, (size_t)total, hipMemcpyDeviceToHost, c->stream));
    }
    GORSE_HIP_CHECK(hipStreamSynchronize(c->stream));
    return GORSE_OK;
}

extern "C" int32_t gorse_cand_get_exclusion(gorse_cand *c, int64_t *indptr_out, int32_t *items_out) {
    if (!c) return fail(GORSE_ERR_INVALID, "handle is NULL");
    if (!c->pass.begun) return fail(GORSE_ERR_INVALID, "gorse_cand_get_exclusion: no pass begun (gorse_cand_begin)");
    GORSE_TRY(c->use());
    const int64_t total = c->cur_ptr_h.back();
    if (indptr_out) std::copy(c->cur_ptr_h.begin(), c->cur_ptr_h.end(), indptr_out);
    if (items_out && total > 0)
        GORSE_HIP_CHECK(hipMemcpyAsync(items_out, c->cur_items[c->cur].p, (size_t)total * 4, hipMemcpyDeviceToHost, c->stream));
    GORSE_HIP_CHECK(hipStreamSynchronize(c->stream));
    return GORSE_OK;
}

extern "C" int32_t gorse_cand_stats(gorse_cand *c, int32_t stage, double *stage_ms, double *chain_ms) {
    if (!c) return fail(GORSE_ERR_INVALID, "handle is NULL");
    if (!c->pass.begun || stage < 0 || stage >= c->pass.n_stages)
        return fail(GORSE_ERR_INVALID, "gorse_cand_stats: stage %d outside the pass's %d stages", stage, c->pass.begun ? c->pass.n_stages : 0);
    if (stage_ms) *stage_ms = c->stage_ms[(size_t)stage];
    if (chain_ms) *chain_ms = c->chain_ms[(size_t)stage];
    return GORSE_OK;
}
