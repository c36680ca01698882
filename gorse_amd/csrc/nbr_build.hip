// nbr_build.hip -- neighbour tables of gorse_nbr built on the device from a similarity search's device-resident results:
// gorse_nbr_set_table_from_topk / _from_sparse, and the read-back of either kind of table (gorse_nbr_get_table / _table_info).
//
// The searches (topk.hip / topk_mfma.hip and its units / sparse.hip) leave a block of result lists on the device: per query k = n + 1 (index,
// distance or score) pairs in rank order and a count.  QueryItemToItem / QueryUserToUser (item_to_item.go:72-86, user_to_user.go:
// 63-80) make a neighbour list of such a list by one ordered walk: skip the row itself, skip scores <= 0 for the Dot kinds, stop
// after n.  Here one wave walks one list -- order kept by ballot and prefix count -- into a staging area of stride n; the kept
// counts become the int64 row pointer by an exclusive scan; a compaction moves the pairs into exactly sized arrays.  Indices and
// weights never cross to the host: only the row pointer (the walk's planner needs it there), one "non-finite weight" flag, the
// largest kept index and, for a hop-1 table, the per-row bounds nbr::row_bounds forms on the host for a host-built table.
#include <cmath>

#include "csr_scan.hpp"
#include "nbr_internal.hpp"
#include "nbr_plan.hpp"
#include "sparse_host.hpp"
#include "topk_internal.hpp"

using namespace gorse;

namespace {

constexpr int kRuleWaves = 4;                      // result rows per workgroup of the row kernels (one wave each)
constexpr int64_t kMaxGrid = (int64_t)1 << 20;

struct RuleArgs {
    const int32_t *idx;   // the block's result lists, stride k
    const float *val;     // distances (negate) or scores
    const int32_t *cnt;
    const int64_t *self;  // per query: the stored row it is (the entry the rule skips)
    const int64_t *dst;   // per query: its row of the table
    int64_t m;            // queries
    int64_t base;         // by_self: the list of query q is row self[q] - base of the block (a covering range was searched); else row q
    int32_t by_self, k, n, negate, positive_only;
    int32_t *st_idx;      // staging, stride n
    float *st_w;
    long long *counts;    // per table row (the row pointer before its scan)
    int32_t *flags;       // [0] |= 1: a kept weight is not finite; [1] = max of the kept indices
};

// One wave per list.  Lane l looks at entries l, l + 64, ..: the ballot of "kept" and the count of kept lanes below give every kept
// entry its place, so the list's order survives.
__global__ __launch_bounds__(kRuleWaves * 64) void nbr_rule_kernel(const RuleArgs A) {
    const int lane = threadIdx.x & 63;
    const int64_t nw = (int64_t)gridDim.x * kRuleWaves;
    int bad = 0;
    int32_t mx = -1;
    for (int64_t q = (int64_t)blockIdx.x * kRuleWaves + (threadIdx.x >> 6); q < A.m; q += nw) {
        const int64_t s = A.self[q], r = A.dst[q];
        const int64_t row = A.by_self ? s - A.base : q;
        const int32_t *li = A.idx + row * A.k;
        const float *lv = A.val + row * A.k;
        const int c = min(max(A.cnt[row], 0), A.k);
        int kept = 0;  // the same in every lane
        for (int e0 = 0; e0 < c && kept < A.n; e0 += 64) {
            const int e = e0 + lane;
            int32_t j = -1;
            float raw = 0.0f;
            if (e < c) {
                j = li[e];
                raw = A.negate ? -lv[e] : lv[e];
            }
            const bool keep = j >= 0 && (int64_t)j != s && !(A.positive_only && raw <= 0.0f);  // a NaN is not <= 0
            const unsigned long long b = __ballot(keep);
            const int pos = kept + __popcll(b & (((unsigned long long)1 << lane) - 1));
            if (keep && pos < A.n) {
                A.st_idx[r * A.n + pos] = j;
                A.st_w[r * A.n + pos] = raw;
                if ((__float_as_uint(raw) & 0x7f800000u) == 0x7f800000u) bad = 1;
                mx = max(mx, j);
            }
            kept += __popcll(b);
        }
        if (lane == 0) A.counts[r] = min(kept, A.n);
    }
    for (int m = 32; m >= 1; m >>= 1) {
        mx = max(mx, __shfl_xor(mx, m, 64));
        bad |= __shfl_xor(bad, m, 64);
    }
    if (lane == 0) {
        if (bad) atomicOr(A.flags, 1);
        if (mx >= 0) atomicMax(A.flags + 1, mx);
    }
}

// staging (stride n) -> the table's exactly sized arrays; one wave per row
__global__ __launch_bounds__(kRuleWaves * 64) void nbr_compact_kernel(const long long *__restrict__ ptr, int64_t n_rows, int n,
                                                                      const int32_t *__restrict__ st_idx, const float *__restrict__ st_w,
                                                                      int32_t *__restrict__ out_idx, float *__restrict__ out_w) {
    const int lane = threadIdx.x & 63;
    const int64_t nw = (int64_t)gridDim.x * kRuleWaves;
    for (int64_t r = (int64_t)blockIdx.x * kRuleWaves + (threadIdx.x >> 6); r < n_rows; r += nw) {
        const long long p0 = ptr[r];
        const int c = (int)min((long long)n, ptr[r + 1] - p0);
        for (int e = lane; e < c; e += 64) {
            out_idx[p0 + e] = st_idx[r * n + e];
            out_w[p0 + e] = st_w[r * n + e];
        }
    }
}

// nbr::row_bounds on the device: src_sum[r] = the sum over hop-1 row r's entries of the hop-2 row lengths; one wave per row.
// (gorse_nbr_recommend has held the table's largest index against the hop-2 rows before this runs.)
__global__ __launch_bounds__(kRuleWaves * 64) void nbr_bound_kernel(const long long *__restrict__ ptr1, const int32_t *__restrict__ idx1,
                                                                    int64_t n_rows1, const long long *__restrict__ ptr2,
                                                                    long long *__restrict__ src_sum) {
    const int lane = threadIdx.x & 63;
    const int64_t nw = (int64_t)gridDim.x * kRuleWaves;
    for (int64_t r = (int64_t)blockIdx.x * kRuleWaves + (threadIdx.x >> 6); r < n_rows1; r += nw) {
        long long s = 0;
        for (long long p = ptr1[r] + lane; p < ptr1[r + 1]; p += 64) {
            const int32_t j = idx1[p];
            s += ptr2[j + 1] - ptr2[j];
        }
        for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
        if (lane == 0) src_sum[r] = s;
    }
}

unsigned row_grid(int64_t rows) { return (unsigned)std::max<int64_t>(1, std::min(ceil_div(rows, kRuleWaves), kMaxGrid)); }

// What one build holds until the table is whole: nothing of the handle changes before finish() swaps it in.
struct Build {
    gorse_nbr *h = nullptr;
    int32_t which = 0, n = 0, positive_only = 0, transform = 0;
    double scale = 1.0;
    int64_t n_rows = 0;
    std::vector<int64_t> rows, src;  // the valid sources: table row, stored row
    DevBuf<int64_t> d_rows, d_src;
    DevBuf<int32_t> st_idx, flags;
    DevBuf<float> st_w;
    DevBuf<int64_t> ptr;  // the kept counts, then the row pointer
    DevBuf<long long> sums;

    int32_t begin() {
        GORSE_TRY(h->use());
        const size_t nv = rows.size();
        GORSE_TRY(d_rows.alloc(nv));
        GORSE_TRY(d_src.alloc(nv));
        GORSE_TRY(st_idx.alloc((size_t)n_rows * n));
        GORSE_TRY(st_w.alloc((size_t)n_rows * n));
        GORSE_TRY(ptr.alloc((size_t)n_rows + 1));
        GORSE_TRY(flags.alloc(2));
        GORSE_HIP_CHECK(hipStreamSynchronize(h->stream));
        if (nv > 0) {
            GORSE_HIP_CHECK(hipMemcpy(d_rows.p, rows.data(), nv * 8, hipMemcpyHostToDevice));
            GORSE_HIP_CHECK(hipMemcpy(d_src.p, src.data(), nv * 8, hipMemcpyHostToDevice));
        }
        GORSE_HIP_CHECK(hipMemsetAsync(ptr.p, 0, ((size_t)n_rows + 1) * 8, h->stream));
        GORSE_HIP_CHECK(hipMemsetAsync(flags.p, 0, 4, h->stream));
        GORSE_HIP_CHECK(hipMemsetAsync(flags.p + 1, 0xff, 4, h->stream));
        GORSE_HIP_CHECK(hipStreamSynchronize(h->stream));  // the rule kernels run on the index's stream
        return GORSE_OK;
    }
    // the rule over the queries [q0, q0 + m) of the valid sources, whose lists lie in (idx, val, cnt)
    int32_t rule(int64_t q0, int64_t m, const int32_t *idx, const float *val, const int32_t *cnt, bool negate, bool by_self, int64_t base,
                 hipStream_t stream) {
        RuleArgs A{};
        A.idx = idx, A.val = val, A.cnt = cnt;
        A.self = d_src.p + q0, A.dst = d_rows.p + q0;
        A.m = m, A.base = base, A.by_self = by_self, A.k = n + 1, A.n = n, A.negate = negate, A.positive_only = positive_only;
        A.st_idx = st_idx.p, A.st_w = st_w.p, A.counts = (long long *)ptr.p, A.flags = flags.p;
        nbr_rule_kernel<<<dim3(row_grid(m)), dim3(kRuleWaves * 64), 0, stream>>>(A);
        GORSE_HIP_CHECK(hipGetLastError());
        return GORSE_OK;
    }
    // `index_stream` holds the rule kernels: the handle's stream waits for them by an event, then scans, compacts and swaps in
    int32_t finish(hipStream_t index_stream, const char *who) {
        hipStream_t st = h->stream;
        hipEvent_t ev = nullptr;
        GORSE_HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        hipError_t e = hipEventRecord(ev, index_stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(st, ev, 0);
        (void)hipEventDestroy(ev);  // (released once the wait has passed)
        if (e != hipSuccess) return fail(GORSE_ERR_HIP, "%s: ordering the two streams: %s", who, hipGetErrorString(e));
        const int64_t ns = n_rows + 1;
        GORSE_TRY(csr_exclusive_scan((long long *)ptr.p, ns, sums, st));
        int32_t fl[2] = {0, -1};
        std::vector<int64_t> ptr_host((size_t)ns);
        GORSE_HIP_CHECK(hipMemcpyAsync(fl, flags.p, 8, hipMemcpyDeviceToHost, st));
        GORSE_HIP_CHECK(hipMemcpyAsync(ptr_host.data(), ptr.p, (size_t)ns * 8, hipMemcpyDeviceToHost, st));
        GORSE_HIP_CHECK(hipStreamSynchronize(st));
        if (fl[0]) return fail(GORSE_ERR_INVALID, "%s: a kept raw weight is not finite", who);
        const int64_t nnz = ptr_host[(size_t)n_rows];
        DevBuf<int32_t> d_idx;
        DevBuf<float> d_w;
        GORSE_TRY(d_idx.alloc((size_t)nnz));
        GORSE_TRY(d_w.alloc((size_t)nnz));
        nbr_compact_kernel<<<dim3(row_grid(n_rows)), dim3(kRuleWaves * 64), 0, st>>>((const long long *)ptr.p, n_rows, n, st_idx.p, st_w.p, d_idx.p, d_w.p);
        GORSE_HIP_CHECK(hipGetLastError());
        GORSE_HIP_CHECK(hipStreamSynchronize(st));
        NbrTable &T = h->tab[which];
        T.set = true, T.weighted = true, T.on_device_only = true;
        T.n_rows = n_rows, T.nnz = nnz, T.max_index = fl[1];
        T.transform = transform, T.scale = scale;
        T.ptr.swap(ptr_host);
        std::vector<int32_t>().swap(T.idx);
        static_assert(sizeof(long long) == sizeof(int64_t), "the row pointer is scanned as long long");
        std::swap(T.d_ptr.p, ptr.p), std::swap(T.d_ptr.n, ptr.n);
        std::swap(T.d_idx.p, d_idx.p), std::swap(T.d_idx.n, d_idx.n);
        std::swap(T.d_w.p, d_w.p), std::swap(T.d_w.n, d_w.n);
        h->bounds_valid = false;
        return GORSE_OK;
    }
};

int32_t build_setup(Build &B, const char *who, gorse_nbr *h, int32_t which, int64_t index_n, int index_device, int64_t n_rows,
                    const int64_t *sources, int32_t n, int32_t positive_only, int32_t transform, double scale) {
    std::string msg;
    const int32_t rc = nbr::validate_from_search(which, n_rows, sources, n, transform, scale, index_n, h->n_items, &B.rows, &B.src, &msg);
    if (rc != GORSE_OK) return fail(rc, "%s: %s", who, msg.c_str());
    if (index_device != h->device)
        return fail(GORSE_ERR_INVALID, "%s: the index is on device %d, the handle on device %d", who, index_device, h->device);
    B.h = h, B.which = which, B.n = n, B.positive_only = positive_only != 0, B.transform = transform, B.scale = scale, B.n_rows = n_rows;
    return B.begin();
}

struct RuleConsumer final : TopkBlockConsumer {
    Build *B = nullptr;
    int32_t block(int64_t q0, int64_t m, const int32_t *idx, const float *dist, const int32_t *cnt, hipStream_t stream) override {
        return B->rule(q0, m, idx, dist, cnt, /*negate=*/true, /*by_self=*/false, 0, stream);
    }
};

}  // namespace

namespace gorse {

int32_t nbr_device_row_bounds(gorse_nbr *h, std::vector<int64_t> *src_sum) {
    NbrTable &T1 = h->tab[GORSE_NBR_HOP1], &T2 = h->tab[GORSE_NBR_HOP2];
    src_sum->assign((size_t)T1.n_rows, 0);
    if (T1.n_rows == 0) return GORSE_OK;
    DevBuf<long long> d_sum;
    GORSE_TRY(d_sum.alloc((size_t)T1.n_rows));
    nbr_bound_kernel<<<dim3(row_grid(T1.n_rows)), dim3(kRuleWaves * 64), 0, h->stream>>>(
        (const long long *)T1.d_ptr.p, T1.d_idx.p, T1.n_rows, (const long long *)T2.d_ptr.p, d_sum.p);
    GORSE_HIP_CHECK(hipGetLastError());
    GORSE_HIP_CHECK(hipMemcpyAsync(src_sum->data(), d_sum.p, (size_t)T1.n_rows * 8, hipMemcpyDeviceToHost, h->stream));
    GORSE_HIP_CHECK(hipStreamSynchronize(h->stream));
    return GORSE_OK;
}

}  // namespace gorse

extern "C" int32_t gorse_nbr_set_table_from_topk(gorse_nbr *h, int32_t which, gorse_topk *index, int64_t n_rows, const int64_t *sources,
                                                 int32_t n, int32_t positive_only, int32_t transform, double scale) {
    const char *who = "gorse_nbr_set_table_from_topk";
    if (!h || !index) return fail(GORSE_ERR_INVALID, "%s: handle is NULL", who);
    Build B;
    GORSE_TRY(build_setup(B, who, h, which, index->N, index->device, n_rows, sources, n, positive_only, transform, scale));
    if (!B.src.empty()) {
        RuleConsumer C;
        C.B = &B;
        GORSE_TRY(topk_search_stored(index, B.src.data(), (int64_t)B.src.size(), n + 1, &C));
        GORSE_TRY(h->use());
    }
    return B.finish(index->stream, who);
}

extern "C" int32_t gorse_nbr_set_table_from_sparse(gorse_nbr *h, int32_t which, gorse_sparse *index, int64_t n_rows, const int64_t *sources,
                                                   int32_t n, int32_t positive_only, int32_t transform, double scale) {
    const char *who = "gorse_nbr_set_table_from_sparse";
    if (!h || !index) return fail(GORSE_ERR_INVALID, "%s: handle is NULL", who);
    Build B;
    GORSE_TRY(build_setup(B, who, h, which, sparse::index_rows(index), sparse::index_device(index), n_rows, sources, n, positive_only,
                          transform, scale));
    hipStream_t index_stream = h->stream;
    if (!B.src.empty()) {
        // the stored rows from the smallest to the largest source asked for are searched; the rule reads the lists of the rows asked for
        const int64_t lo = *std::min_element(B.src.begin(), B.src.end()), hi = *std::max_element(B.src.begin(), B.src.end());
        sparse::StoredRowsResult R;
        GORSE_TRY(sparse::search_stored_rows(index, lo, hi + 1, n + 1, &R));
        GORSE_TRY(h->use());
        index_stream = (hipStream_t)R.stream;
        GORSE_TRY(B.rule(0, (int64_t)B.src.size(), R.idx, R.score, R.cnt, /*negate=*/false, /*by_self=*/true, lo, index_stream));
    }
    return B.finish(index_stream, who);
}

extern "C" int32_t gorse_nbr_table_info(gorse_nbr *h, int32_t which, int64_t *n_rows, int64_t *nnz, int32_t *weighted) {
    if (!h) return fail(GORSE_ERR_INVALID, "handle is NULL");
    if (which != GORSE_NBR_HOP1 && which != GORSE_NBR_HOP2) return fail(GORSE_ERR_INVALID, "gorse_nbr_table_info: which = %d is neither hop", which);
    const NbrTable &T = h->tab[which];
    if (!T.set) return fail(GORSE_ERR_INVALID, "gorse_nbr_table_info: the hop-%d table is not set", which + 1);
    if (n_rows) *n_rows = T.n_rows;
    if (nnz) *nnz = T.nnz;
    if (weighted) *weighted = T.weighted ? 1 : 0;
    return GORSE_OK;
}

extern "C" int32_t gorse_nbr_get_table(gorse_nbr *h, int32_t which, int64_t *indptr, int32_t *indices, float *weights) {
    if (!h) return fail(GORSE_ERR_INVALID, "handle is NULL");
    if (which != GORSE_NBR_HOP1 && which != GORSE_NBR_HOP2) return fail(GORSE_ERR_INVALID, "gorse_nbr_get_table: which = %d is neither hop", which);
    const NbrTable &T = h->tab[which];
    if (!T.set) return fail(GORSE_ERR_INVALID, "gorse_nbr_get_table: the hop-%d table is not set", which + 1);
    if (weights && !T.weighted) return fail(GORSE_ERR_INVALID, "gorse_nbr_get_table: the hop-%d table has no weights", which + 1);
    GORSE_TRY(h->use());
    if (indptr) std::copy(T.ptr.begin(), T.ptr.end(), indptr);
    if (indices && T.nnz > 0) GORSE_HIP_CHECK(hipMemcpyAsync(indices, T.d_idx.p, (size_t)T.nnz * 4, hipMemcpyDeviceToHost, h->stream));
    if (weights && T.nnz > 0) GORSE_HIP_CHECK(hipMemcpyAsync(weights, T.d_w.p, (size_t)T.nnz * 4, hipMemcpyDeviceToHost, h->stream));
    GORSE_HIP_CHECK(hipStreamSynchronize(h->stream));
    return GORSE_OK;
}
