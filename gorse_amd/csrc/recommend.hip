// recommend.hip -- gorse_mf_recommend: every user's k best UNSEEN items straight from the resident model.
// Reference: worker/pipeline.go:403-448 (updateCollaborativeRecommend) asks for CacheSize + |excludeSet| neighbours of the user's
// factor and drops the seen ones; here the exclusion happens on the device, behind the score's comparison with the user's running
// threshold, so nothing is over-fetched.  The result row is what gorse_mf_rank returns for the list of admissible unseen items in
// ascending order (heap.TopKFilter(k), common/heap/filter.go:23-59).
//
// Fast path (rec_fast_kernel + rec_finish_kernel).  A workgroup owns 16 queries (one per 16-lane group) and one SLICE of the items;
// it walks the slice in tiles of Q staged in LDS.  A group scores one item at a time in the reference's AVX512 order (cf_device.hpp)
// and compares the score with its threshold; only a score that passes is tested against item_ok, the user's sorted training row and
// the sorted seen row (binary searches), and appended to the group's buffer in global memory.  A full buffer is compacted to its
// kk = k + 1 best, sorted, and the threshold becomes the kk-th best.
//   Invariant: a score is dropped only when kk buffered candidates are >= it, so the kk best candidate SCORES of a slice always
//   survive, as a sorted sequence of values; the finish kernel merges the slices' lists and keeps the kk best of all.
//   Tie rule: a query whose kk best scores hold an equal pair (-0 == +0), or that met a NaN candidate score, is left to the literal
//   path; for every other query the k best items are uniquely ordered by score and that order IS the heap's.
// Literal path: the query's candidate list is materialised on the device in ascending order (rec_candidates_kernel) and handed to
// mf_rank_device, in chunks of bounded size; its scores come from mf_score_device.
#include <algorithm>
#include <cmath>

#include "mf_internal.hpp"

using namespace gorse;

namespace {

constexpr int kRecMaxK = 256;          // the fast path serves k <= this; beyond it every query is literal
constexpr int kRecMaxSlices = 8;       // item slices per query block at most
constexpr int kRecTileFloats = 8192;   // floats of Q per LDS tile (32 KB)
constexpr int kRecMaxTileItems = 1024;
constexpr int64_t kRecLiteralChunk = (int64_t)1 << 22;  // candidates materialised per literal launch at most (one query at least)
constexpr size_t kRecScratchBytes = (size_t)256 << 20;  // the fast path's buffers per launch

int g_rec_slices = 0;              // test hook: > 0 forces the slice count
int g_rec_buffer = 0;              // test hook: > 0 forces the buffer size (raised to k + 2 where smaller)
int64_t g_rec_literal_chunk = 0;   // test hook: > 0 replaces kRecLiteralChunk

struct RecArgs {
    const float *P, *Q;
    const int32_t *users;  // null: query t is user t
    const int64_t *uptr;
    const int32_t *uidx_sorted;
    const int64_t *sptr;  // null: no seen rows
    const int32_t *seen;  // every row sorted ascending
    const uint8_t *item_ok;
    int64_t q0, nq;  // the launch's queries are [q0, q0 + nq)
    int32_t I, d, k, kk, cap, slices, slice_len, tile_items;
    float *buf_s;     // nq * slices * 2 * cap: two halves per (query, slice), a compaction moves from one to the other
    int32_t *buf_i;
    float *out_s;     // nq * slices * kk: the slice's kk best, sorted by score descending
    int32_t *out_i;
    int32_t *out_cnt;   // nq * slices
    int32_t *nan_flag;  // nq
};

__device__ __forceinline__ bool rec_candidate(const uint8_t *__restrict__ item_ok, const int32_t *trow, int64_t tn, const int32_t *srow,
                                              int64_t sn, int32_t item) {
    return item_ok[item] != 0 && !row_contains(trow, tn, item) && !(sn > 0 && row_contains(srow, sn, item));
}

// One 16-lane group: the kk best of cnt buffered entries to dst, sorted by score descending (equal scores in buffer order).  Every
// entry is ranked by counting the entries ahead of it.  Returns the kk-th best score (-inf when there are fewer).  No NaN is buffered.
__device__ __forceinline__ float rec_compact(const float *ss, const int32_t *si, int cnt, float *ds, int32_t *di, int kk, int lane) {
    float kth = -INFINITY;
    for (int e = lane; e < cnt; e += kGroup) {
        const float s = ss[e];
        int rank = 0;
        for (int j = 0; j < cnt; j++) {
            const float o = ss[j];
            rank += (o > s || (o == s && j < e)) ? 1 : 0;
        }
        if (rank < kk) {
            ds[rank] = s;
            di[rank] = si[e];
            if (rank == kk - 1) kth = s;
        }
    }
    for (int m = 8; m >= 1; m >>= 1) kth = fmaxf(kth, __shfl_xor(kth, m, kGroup));
    return kth;
}

// NC > 0: d == 16 * NC, the user's row in registers; NC == 0: any d, the user's row in LDS behind the tile
template <int NC>
__global__ __launch_bounds__(kBlock) void rec_fast_kernel(const RecArgs A) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *tile = smem;
    const int lane = threadIdx.x & (kGroup - 1);
    const int gib = threadIdx.x / kGroup;
    const int d = A.d;
    const int64_t tq = (int64_t)blockIdx.x * kGroupsPerBlock + gib;
    const int sl = blockIdx.y;
    const int i0 = sl * A.slice_len;
    const int i1 = min(A.I, i0 + A.slice_len);
    int u = -1;
    if (tq < A.nq) u = A.users ? A.users[A.q0 + tq] : (int)(A.q0 + tq);
    const bool active = u >= 0;
    const VecShape vs(d);
    float a[NC > 0 ? NC : 1];
    float *urow = nullptr;
    if constexpr (NC > 0) {
#pragma unroll
        for (int c = 0; c < NC; c++) a[c] = active ? A.P[(int64_t)u * d + 16 * c + lane] : 0.0f;
    } else {
        urow = smem + (size_t)A.tile_items * d + (size_t)gib * d;
        if (active)
            for (int e = lane; e < d; e += kGroup) urow[e] = A.P[(int64_t)u * d + e];
    }
    const int32_t *trow = nullptr, *srow = nullptr;
    int64_t tn = 0, sn = 0;
    if (active) {
        trow = A.uidx_sorted + A.uptr[u];
        tn = A.uptr[u + 1] - A.uptr[u];
        if (A.sptr) {
            srow = A.seen + A.sptr[A.q0 + tq];
            sn = A.sptr[A.q0 + tq + 1] - A.sptr[A.q0 + tq];
        }
    }
    const int cap = A.cap, kk = A.kk;
    const int64_t slot = (tq < A.nq ? tq : 0) * A.slices + sl;
    float *bs = A.buf_s + slot * 2 * cap;
    int32_t *bi = A.buf_i + slot * 2 * cap;
    int half = 0, cnt = 0;
    float thr = __int_as_float(0x7fc00000);  // NaN: !(s <= thr) holds for every s until the first compaction
    for (int t0 = i0; t0 < i1; t0 += A.tile_items) {
        const int nt = min(A.tile_items, i1 - t0);
        __syncthreads();
        {   // the tile's rows are contiguous in Q
            const float *src = A.Q + (int64_t)t0 * d;
            const int nf = nt * d;
            if ((d & 3) == 0) {
                const float4 *s4 = (const float4 *)src;
                float4 *t4 = (float4 *)tile;
                for (int e = threadIdx.x; e < nf / 4; e += kBlock) t4[e] = s4[e];
            } else {
                for (int e = threadIdx.x; e < nf; e += kBlock) tile[e] = src[e];
            }
        }
        __syncthreads();
        if (!active) continue;
        for (int r = 0; r < nt; r++) {
            const float *qrow = tile + (size_t)r * d;
            float s;
            if constexpr (NC > 0) {
                float b[NC];
#pragma unroll
                for (int c = 0; c < NC; c++) b[c] = qrow[16 * c + lane];
                s = dot512_regs<NC>(a, b);
            } else {
                s = dot512_lds(urow, qrow, vs, lane);
            }
            if (!(s <= thr)) {  // (group-uniform: every lane of the group holds the same total)
                const int item = t0 + r;
                if (rec_candidate(A.item_ok, trow, tn, srow, sn, item)) {
                    if (s != s) {
                        if (lane == 0) atomicOr(&A.nan_flag[tq], 1);
                    } else {
                        float *cs = bs + half * cap;
                        int32_t *ci = bi + half * cap;
                        if (lane == 0) {
                            cs[cnt] = s;
                            ci[cnt] = item;
                        }
                        cnt++;
                        if (cnt == cap) {
                            __threadfence_block();
                            thr = rec_compact(cs, ci, cnt, bs + (half ^ 1) * cap, bi + (half ^ 1) * cap, kk, lane);
                            __threadfence_block();
                            half ^= 1;
                            cnt = kk;
                        }
                    }
                }
            }
        }
    }
    if (tq < A.nq) {
        int n = 0;
        if (active && cnt > 0) {
            __threadfence_block();
            (void)rec_compact(bs + half * cap, bi + half * cap, cnt, A.out_s + slot * kk, A.out_i + slot * kk, kk, lane);
            n = min(cnt, kk);
        }
        if (lane == 0) A.out_cnt[slot] = n;
    }
}

// One workgroup per query: the slices' lists merged, the kk best ranked, the tie rule applied.  lit[t] = 1: left to the literal path.
__global__ __launch_bounds__(kBlock) void rec_finish_kernel(const RecArgs A, int32_t *__restrict__ res_items, float *__restrict__ res_scores,
                                                            int32_t *__restrict__ res_cnt, int32_t *__restrict__ lit) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int kk = A.kk, k = A.k, maxn = A.slices * kk;
    float *es = smem;
    int32_t *ei = (int32_t *)(smem + maxn);
    float *ts = smem + 2 * (size_t)maxn;
    int32_t *ti = (int32_t *)(ts + kk);
    __shared__ int s_tie;
    const int64_t tq = blockIdx.x;
    const int tid = threadIdx.x;
    int n = 0;
    for (int sl = 0; sl < A.slices; sl++) {
        const int64_t slot = tq * A.slices + sl;
        const int c = A.out_cnt[slot];
        for (int e = tid; e < c; e += kBlock) {
            es[n + e] = A.out_s[slot * kk + e];
            ei[n + e] = A.out_i[slot * kk + e];
        }
        n += c;
    }
    if (tid == 0) s_tie = A.nan_flag[tq];
    __syncthreads();
    const int m = min(n, kk);
    for (int e = tid; e < n; e += kBlock) {
        const float s = es[e];
        int rank = 0;
        for (int j = 0; j < n; j++) {
            const float o = es[j];
            rank += (o > s || (o == s && j < e)) ? 1 : 0;
        }
        if (rank < m) {
            ts[rank] = s;
            ti[rank] = ei[e];
        }
    }
    __syncthreads();
    for (int r = tid; r + 1 < m; r += kBlock)
        if (ts[r] == ts[r + 1]) atomicOr(&s_tie, 1);
    __syncthreads();
    const int tie = s_tie;
    const int cntk = tie ? 0 : min(n, k);
    if (tid == 0) {
        lit[tq] = tie;
        res_cnt[tq] = cntk;
    }
    for (int r = tid; r < k; r += kBlock) {
        res_items[tq * k + r] = r < cntk ? ti[r] : -1;
        res_scores[tq * k + r] = r < cntk ? ts[r] : 0.0f;
    }
}

// Literal path: the candidates of query q in ascending order.  cand == null: only their number, to cnt_out; otherwise the list, to
// cand[cptr[q] ..).  One workgroup per query, 256 items per step, kept in order by a ballot scan.
__global__ __launch_bounds__(kBlock) void rec_candidates_kernel(const int32_t *__restrict__ lit_user, const int64_t *__restrict__ lit_query,
                                                                const int64_t *__restrict__ uptr, const int32_t *__restrict__ uidx_sorted,
                                                                const int64_t *__restrict__ sptr, const int32_t *__restrict__ seen,
                                                                const uint8_t *__restrict__ item_ok, int32_t I,
                                                                const int64_t *__restrict__ cptr, int32_t *__restrict__ cand,
                                                                int32_t *__restrict__ cnt_out) {
    __shared__ int wsum[kBlock / 64];
    const int64_t q = blockIdx.x;
    const int u = lit_user[q];
    const int tid = threadIdx.x, w = tid / 64, l = tid % 64;
    const int32_t *trow = uidx_sorted + uptr[u], *srow = nullptr;
    const int64_t tn = uptr[u + 1] - uptr[u];
    int64_t sn = 0;
    if (sptr) {
        const int64_t t = lit_query[q];
        srow = seen + sptr[t];
        sn = sptr[t + 1] - sptr[t];
    }
    const int64_t out0 = cand ? cptr[q] : 0;
    int base = 0;
    for (int i0 = 0; i0 < I; i0 += kBlock) {
        const int item = i0 + tid;
        const bool c = item < I && rec_candidate(item_ok, trow, tn, srow, sn, item);
        const unsigned long long b = __ballot(c);
        const int pre = __popcll(b & ((1ull << l) - 1ull));
        if (l == 0) wsum[w] = __popcll(b);
        __syncthreads();
        int off = 0, tot = 0;
        for (int x = 0; x < kBlock / 64; x++) {
            if (x < w) off += wsum[x];
            tot += wsum[x];
        }
        if (c && cand) cand[out0 + base + off + pre] = item;
        base += tot;
        __syncthreads();
    }
    if (!cand && tid == 0) cnt_out[q] = base;
}

// device time of what runs between begin() and end() on one stream, added up
struct RecTimer {
    hipEvent_t a = nullptr, b = nullptr;
    double ms = 0.0;
    ~RecTimer() {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
    }
    int32_t init() {
        GORSE_HIP_CHECK(hipEventCreate(&a));
        GORSE_HIP_CHECK(hipEventCreate(&b));
        return GORSE_OK;
    }
    int32_t begin(hipStream_t s) {
        GORSE_HIP_CHECK(hipEventRecord(a, s));
        return GORSE_OK;
    }
    int32_t end(hipStream_t s) {  // synchronises the stream
        GORSE_HIP_CHECK(hipEventRecord(b, s));
        GORSE_HIP_CHECK(hipEventSynchronize(b));
        float t = 0.0f;
        GORSE_HIP_CHECK(hipEventElapsedTime(&t, a, b));
        ms += t;
        return GORSE_OK;
    }
};

}  // namespace

extern "C" void gorse_hip_test_set_recommend(int32_t slices, int32_t buffer, int64_t literal_chunk) {
    g_rec_slices = slices > 0 ? std::min<int32_t>(slices, kRecMaxSlices) : 0;
    g_rec_buffer = buffer > 0 ? buffer : 0;
    g_rec_literal_chunk = literal_chunk > 0 ? literal_chunk : 0;
}

extern "C" int32_t gorse_mf_recommend_stats(gorse_mf *h, int64_t *n_fast, int64_t *n_literal, double *device_ms) {
    if (!h) return fail(GORSE_ERR_INVALID, "handle is NULL");
    if (n_fast) *n_fast = h->rec_fast;
    if (n_literal) *n_literal = h->rec_literal;
    if (device_ms) *device_ms = h->rec_ms;
    return GORSE_OK;
}

namespace gorse {

int32_t mf_recommend_check(gorse_mf *h, int64_t n_users, const int32_t *users, int32_t k) {
    if (!h) return fail(GORSE_ERR_INVALID, "handle is NULL");
    if (k <= 0) return fail(GORSE_ERR_INVALID, "k <= 0");
    if (n_users < 0) return fail(GORSE_ERR_INVALID, "n_users < 0");
    if (!users && n_users > h->U) return fail(GORSE_ERR_INVALID, "users is NULL and n_users %lld > %lld users", (long long)n_users, (long long)h->U);
    if (n_users > ((int64_t)1 << 40) / k) return fail(GORSE_ERR_INVALID, "n_users * k too large");
    if (users)
        for (int64_t t = 0; t < n_users; t++)
            if (users[t] >= h->U) return fail(GORSE_ERR_RANGE, "user %d out of range [0,%lld)", users[t], (long long)h->U);
    return GORSE_OK;
}

int32_t mf_recommend_core(gorse_mf *h, int64_t n_users, const int32_t *users, int32_t k, const uint8_t *item_ok, const int64_t *d_sptr,
                          const int32_t *d_seen, int32_t *items_out, float *scores_out, int32_t *count_out, const MfDeviceRows *dev) {
    GORSE_TRY(h->use());
    GORSE_TRY(mf_sync_streams(h));  // behind every epoch still enqueued on the handle
    h->rec_fast = h->rec_literal = 0;
    h->rec_ms = 0.0;
    if (n_users == 0) return GORSE_OK;
    if (dev && k > kRecMaxK) return fail(GORSE_ERR_INVALID, "device rows are served for k <= %d", kRecMaxK);

    // ---- inputs to the device: users, the item filter
    const int64_t I = h->I;
    std::vector<uint8_t> ok_host;
    if (!item_ok) {
        ok_host.resize((size_t)I);
        for (int64_t i = 0; i < I; i++) ok_host[(size_t)i] = h->h_item_count[(size_t)i] > 0;  // IsItemPredictable
        item_ok = ok_host.data();
    }
    Carver in;
    const size_t o_users = in.take((size_t)n_users * 4), o_ok = in.take((size_t)I);
    GORSE_TRY(h->rec_in.ensure(in.off));
    int32_t *d_users = users ? (int32_t *)(h->rec_in.p + o_users) : nullptr;
    uint8_t *d_ok = (uint8_t *)(h->rec_in.p + o_ok);
    if (users) GORSE_HIP_CHECK(hipMemcpyAsync(d_users, users, (size_t)n_users * 4, hipMemcpyHostToDevice, h->stream));
    GORSE_HIP_CHECK(hipMemcpyAsync(d_ok, item_ok, (size_t)I, hipMemcpyHostToDevice, h->stream));

    std::vector<int32_t> items_tmp, count_tmp;
    std::vector<float> scores_tmp;
    if (!dev) {  // (the device route keeps no host rows: its few literal rows are assembled in buffers of their own below)
        if (!items_out) {
            items_tmp.resize((size_t)n_users * k);
            items_out = items_tmp.data();
        }
        if (!scores_out) {
            scores_tmp.resize((size_t)n_users * k);
            scores_out = scores_tmp.data();
        }
        if (!count_out) {
            count_tmp.resize((size_t)n_users);
            count_out = count_tmp.data();
        }
    }
    RecTimer timer;
    GORSE_TRY(timer.init());
    std::vector<int64_t> lit_query;  // the queries left to the literal path
    const int d = h->d;

    if (k <= kRecMaxK) {
        RecArgs A{};
        A.P = h->P.p;
        A.Q = h->Q.p;
        A.users = d_users;
        A.uptr = h->uptr.p;
        A.uidx_sorted = h->uidx_sorted.p;
        A.sptr = d_sptr;
        A.seen = d_seen;
        A.item_ok = d_ok;
        A.I = (int32_t)I;
        A.d = d;
        A.k = k;
        A.kk = k + 1;
        A.cap = std::max(32, 2 * A.kk);
        if (g_rec_buffer > 0) A.cap = std::max(A.kk + 1, g_rec_buffer);
        // too few query blocks to fill the chip: the items in slices across workgroups
        int slices = 1;
        const int64_t blocks = ceil_div(n_users, kGroupsPerBlock);
        while (slices < kRecMaxSlices && blocks * slices < 512 && I / (slices * 2) >= 256) slices *= 2;
        if (g_rec_slices > 0) slices = g_rec_slices;
        slices = (int)std::min<int64_t>(slices, I);
        A.slices = slices;
        A.slice_len = (int32_t)ceil_div(I, slices);
        A.tile_items = std::max(1, std::min({kRecTileFloats / d, kRecMaxTileItems, (int)A.slice_len}));
        const size_t lds_fast = ((size_t)A.tile_items * d + (factor_row_in_registers(d) ? 0 : (size_t)kGroupsPerBlock * d)) * sizeof(float);
        const size_t lds_fin = ((size_t)2 * slices * A.kk + (size_t)2 * A.kk) * 4;
        const size_t per_query = (size_t)slices * ((size_t)2 * A.cap * 8 + (size_t)A.kk * 8 + 4) + (size_t)k * 8 + 16;
        int64_t chunk = (int64_t)(kRecScratchBytes / per_query) / kGroupsPerBlock * kGroupsPerBlock;
        chunk = std::min<int64_t>(std::max<int64_t>(chunk, kGroupsPerBlock), n_users);
        Carver sc;
        const size_t o_bs = sc.take((size_t)chunk * slices * 2 * A.cap * 4), o_bi = sc.take((size_t)chunk * slices * 2 * A.cap * 4),
                     o_os = sc.take((size_t)chunk * slices * A.kk * 4), o_oi = sc.take((size_t)chunk * slices * A.kk * 4),
                     o_oc = sc.take((size_t)chunk * slices * 4), o_nan = sc.take((size_t)chunk * 4),
                     o_ri = sc.take((size_t)chunk * k * 4), o_rs = sc.take((size_t)chunk * k * 4), o_rc = sc.take((size_t)chunk * 4),
                     o_lit = sc.take((size_t)chunk * 4);
        GORSE_TRY(h->rec_buf.ensure(sc.off));
        char *base = h->rec_buf.p;
        A.buf_s = (float *)(base + o_bs);
        A.buf_i = (int32_t *)(base + o_bi);
        A.out_s = (float *)(base + o_os);
        A.out_i = (int32_t *)(base + o_oi);
        A.out_cnt = (int32_t *)(base + o_oc);
        A.nan_flag = (int32_t *)(base + o_nan);
        int32_t *d_ri = (int32_t *)(base + o_ri), *d_rc = (int32_t *)(base + o_rc), *d_lit = (int32_t *)(base + o_lit);
        float *d_rs = (float *)(base + o_rs);
        std::vector<int32_t> lit_host((size_t)chunk);
        for (int64_t q0 = 0; q0 < n_users; q0 += chunk) {
            const int64_t nq = std::min(chunk, n_users - q0);
            A.q0 = q0;
            A.nq = nq;
            GORSE_TRY(timer.begin(h->stream));
            GORSE_HIP_CHECK(hipMemsetAsync(A.nan_flag, 0, (size_t)nq * 4, h->stream));
            const dim3 grid((unsigned)ceil_div(nq, kGroupsPerBlock), (unsigned)slices);
            with_factor_chunks(d, [&](auto nc) { rec_fast_kernel<decltype(nc)::value><<<grid, dim3(kBlock), lds_fast, h->stream>>>(A); });
            GORSE_HIP_CHECK(hipGetLastError());
            rec_finish_kernel<<<dim3((unsigned)nq), dim3(kBlock), lds_fin, h->stream>>>(A, d_ri, d_rs, d_rc, d_lit);
            GORSE_HIP_CHECK(hipGetLastError());
            GORSE_TRY(timer.end(h->stream));
            if (dev) {  // the chunk's rows stay on the device
                GORSE_HIP_CHECK(hipMemcpyAsync(dev->items + q0 * k, d_ri, (size_t)nq * k * 4, hipMemcpyDeviceToDevice, h->stream));
                GORSE_HIP_CHECK(hipMemcpyAsync(dev->scores + q0 * k, d_rs, (size_t)nq * k * 4, hipMemcpyDeviceToDevice, h->stream));
                GORSE_HIP_CHECK(hipMemcpyAsync(dev->cnt + q0, d_rc, (size_t)nq * 4, hipMemcpyDeviceToDevice, h->stream));
            } else {
                GORSE_HIP_CHECK(hipMemcpyAsync(items_out + q0 * k, d_ri, (size_t)nq * k * 4, hipMemcpyDeviceToHost, h->stream));
                GORSE_HIP_CHECK(hipMemcpyAsync(scores_out + q0 * k, d_rs, (size_t)nq * k * 4, hipMemcpyDeviceToHost, h->stream));
                GORSE_HIP_CHECK(hipMemcpyAsync(count_out + q0, d_rc, (size_t)nq * 4, hipMemcpyDeviceToHost, h->stream));
            }
            GORSE_HIP_CHECK(hipMemcpyAsync(lit_host.data(), d_lit, (size_t)nq * 4, hipMemcpyDeviceToHost, h->stream));
            GORSE_HIP_CHECK(hipStreamSynchronize(h->stream));
            for (int64_t t = 0; t < nq; t++)
                if (lit_host[(size_t)t]) lit_query.push_back(q0 + t);
        }
    } else {
        for (int64_t t = 0; t < n_users; t++) {
            const int32_t u = users ? users[t] : (int32_t)t;
            if (u >= 0) {
                lit_query.push_back(t);
            } else {
                count_out[t] = 0;
                std::fill(items_out + t * k, items_out + (t + 1) * k, -1);
                std::fill(scores_out + t * k, scores_out + (t + 1) * k, 0.0f);
            }
        }
    }

    // ---- literal path: candidate lists on the device -> mf_rank_device, in chunks; scores of the ranked items afterwards
    const int64_t nl = (int64_t)lit_query.size();
    if (nl > 0) {
        std::vector<int32_t> lit_user((size_t)nl), cnt_host((size_t)nl);
        for (int64_t q = 0; q < nl; q++) lit_user[(size_t)q] = users ? users[lit_query[(size_t)q]] : (int32_t)lit_query[(size_t)q];
        Carver lc;
        const size_t o_lu = lc.take((size_t)nl * 4), o_lq = lc.take((size_t)nl * 8), o_cnt = lc.take((size_t)nl * 4);
        GORSE_TRY(h->rec_buf.ensure(lc.off));
        int32_t *d_lu = (int32_t *)(h->rec_buf.p + o_lu), *d_cnt = (int32_t *)(h->rec_buf.p + o_cnt);
        int64_t *d_lq = (int64_t *)(h->rec_buf.p + o_lq);
        GORSE_HIP_CHECK(hipMemcpyAsync(d_lu, lit_user.data(), (size_t)nl * 4, hipMemcpyHostToDevice, h->stream));
        GORSE_HIP_CHECK(hipMemcpyAsync(d_lq, lit_query.data(), (size_t)nl * 8, hipMemcpyHostToDevice, h->stream));
        GORSE_TRY(timer.begin(h->stream));
        rec_candidates_kernel<<<dim3((unsigned)nl), dim3(kBlock), 0, h->stream>>>(d_lu, d_lq, h->uptr.p, h->uidx_sorted.p, d_sptr, d_seen,
                                                                                 d_ok, (int32_t)I, nullptr, nullptr, d_cnt);
        GORSE_HIP_CHECK(hipGetLastError());
        GORSE_TRY(timer.end(h->stream));
        GORSE_HIP_CHECK(hipMemcpyAsync(cnt_host.data(), d_cnt, (size_t)nl * 4, hipMemcpyDeviceToHost, h->stream));
        GORSE_HIP_CHECK(hipStreamSynchronize(h->stream));
        std::vector<int32_t> rank((size_t)nl * k), rlen((size_t)nl);
        const int64_t bound = g_rec_literal_chunk > 0 ? g_rec_literal_chunk : kRecLiteralChunk;
        std::vector<int64_t> cptr;
        for (int64_t a = 0; a < nl;) {
            cptr.assign(1, 0);
            int64_t b = a;
            while (b < nl && (b == a || cptr.back() + cnt_host[(size_t)b] <= bound)) {
                cptr.push_back(cptr.back() + cnt_host[(size_t)b]);
                b++;
            }
            const int64_t nc = cptr.back();
            Carver cc;
            const size_t o_cp = cc.take((size_t)(b - a + 1) * 8), o_cd = cc.take((size_t)std::max<int64_t>(nc, 1) * 4);
            GORSE_TRY(h->rec_lit.ensure(cc.off));
            int64_t *d_cp = (int64_t *)(h->rec_lit.p + o_cp);
            int32_t *d_cd = (int32_t *)(h->rec_lit.p + o_cd);
            GORSE_HIP_CHECK(hipMemcpyAsync(d_cp, cptr.data(), (size_t)(b - a + 1) * 8, hipMemcpyHostToDevice, h->stream));
            GORSE_TRY(timer.begin(h->stream));
            rec_candidates_kernel<<<dim3((unsigned)(b - a)), dim3(kBlock), 0, h->stream>>>(d_lu + a, d_lq + a, h->uptr.p, h->uidx_sorted.p, d_sptr,
                                                                                          d_seen, d_ok, (int32_t)I, d_cp, d_cd, nullptr);
            GORSE_HIP_CHECK(hipGetLastError());
            UserLists lists;
            lists.n_users = b - a, lists.users = d_lu + a, lists.cand_ptr = d_cp, lists.cand = d_cd, lists.n_cand = nc;
            GORSE_TRY(mf_rank_device(h, lists, k, rank.data() + a * k, rlen.data() + a));
            GORSE_TRY(timer.end(h->stream));
            GORSE_HIP_CHECK(hipStreamSynchronize(h->stream));
            a = b;
        }
        // the ranked items' scores (internalPredict, the bits of gorse_mf_score)
        std::vector<int32_t> pu, pi;
        for (int64_t q = 0; q < nl; q++)
            for (int32_t r = 0; r < rlen[(size_t)q]; r++) {
                pu.push_back(lit_user[(size_t)q]);
                pi.push_back(rank[(size_t)q * k + r]);
            }
        const int64_t np = (int64_t)pu.size();
        std::vector<float> ps((size_t)np);
        if (np > 0) {
            Carver pc;
            const size_t o_pu = pc.take((size_t)np * 4), o_pi = pc.take((size_t)np * 4), o_ps = pc.take((size_t)np * 4);
            GORSE_TRY(h->rec_lit.ensure(pc.off));
            int32_t *d_pu = (int32_t *)(h->rec_lit.p + o_pu), *d_pi = (int32_t *)(h->rec_lit.p + o_pi);
            float *d_ps = (float *)(h->rec_lit.p + o_ps);
            GORSE_HIP_CHECK(hipMemcpyAsync(d_pu, pu.data(), (size_t)np * 4, hipMemcpyHostToDevice, h->stream));
            GORSE_HIP_CHECK(hipMemcpyAsync(d_pi, pi.data(), (size_t)np * 4, hipMemcpyHostToDevice, h->stream));
            GORSE_TRY(timer.begin(h->stream));
            GORSE_TRY(mf_score_device(h, d_pu, d_pi, np, d_ps));
            GORSE_TRY(timer.end(h->stream));
            GORSE_HIP_CHECK(hipMemcpyAsync(ps.data(), d_ps, (size_t)np * 4, hipMemcpyDeviceToHost, h->stream));
            GORSE_HIP_CHECK(hipStreamSynchronize(h->stream));
        }
        if (dev) {  // the literal rows, row after row in one buffer each, follow the threshold path's rows to the device
            items_tmp.resize((size_t)nl * k);
            scores_tmp.resize((size_t)nl * k);
        }
        int64_t p = 0;
        for (int64_t q = 0; q < nl; q++) {
            const int64_t t = lit_query[(size_t)q];
            const int32_t n = rlen[(size_t)q];
            int32_t *ri = dev ? items_tmp.data() + q * k : items_out + t * k;
            float *rs = dev ? scores_tmp.data() + q * k : scores_out + t * k;
            if (!dev) count_out[t] = n;
            for (int32_t r = 0; r < k; r++) {
                ri[r] = r < n ? rank[(size_t)q * k + r] : -1;
                rs[r] = r < n ? ps[(size_t)(p + r)] : 0.0f;
            }
            p += n;
        }
        if (dev) {
            for (int64_t q = 0; q < nl; q++) {
                const int64_t t = lit_query[(size_t)q];
                GORSE_HIP_CHECK(hipMemcpyAsync(dev->items + t * k, items_tmp.data() + q * k, (size_t)k * 4, hipMemcpyHostToDevice, h->stream));
                GORSE_HIP_CHECK(hipMemcpyAsync(dev->scores + t * k, scores_tmp.data() + q * k, (size_t)k * 4, hipMemcpyHostToDevice, h->stream));
                GORSE_HIP_CHECK(hipMemcpyAsync(dev->cnt + t, rlen.data() + q, 4, hipMemcpyHostToDevice, h->stream));
            }
            GORSE_HIP_CHECK(hipStreamSynchronize(h->stream));
        }
    }
    h->rec_literal = nl;
    h->rec_fast = n_users - nl;
    h->rec_ms = timer.ms;
    return GORSE_OK;
}

}  // namespace gorse

extern "C" int32_t gorse_mf_recommend(gorse_mf *h, int64_t n_users, const int32_t *users, int32_t k, const uint8_t *item_ok,
                                      const int64_t *seen_indptr, const int32_t *seen_items, int32_t *items_out, float *scores_out,
                                      int32_t *count_out) {
    GORSE_TRY(mf_recommend_check(h, n_users, users, k));
    const int64_t I = h->I;
    int64_t n_seen = 0;
    if (seen_indptr && n_users > 0) {
        if (seen_indptr[0] < 0) return fail(GORSE_ERR_INVALID, "seen_indptr[0] < 0");
        for (int64_t t = 0; t < n_users; t++)
            if (seen_indptr[t + 1] < seen_indptr[t]) return fail(GORSE_ERR_INVALID, "seen_indptr not monotone at row %lld", (long long)t);
        n_seen = seen_indptr[n_users] - seen_indptr[0];
        if (n_seen > 0 && !seen_items) return fail(GORSE_ERR_INVALID, "seen_items is NULL");
        for (int64_t e = seen_indptr[0]; e < seen_indptr[n_users]; e++)
            if (seen_items[e] < 0 || seen_items[e] >= I)
                return fail(GORSE_ERR_RANGE, "seen_items[%lld] = %d out of range [0,%lld)", (long long)e, seen_items[e], (long long)I);
    }
    if (n_users == 0) return mf_recommend_core(h, 0, users, k, item_ok, nullptr, nullptr, items_out, scores_out, count_out, nullptr);

    // ---- the seen rows sorted, to the device; the core reads a sorted device CSR (the candidate chain hands it its own)
    std::vector<int64_t> sptr_host;
    std::vector<int32_t> seen_host;
    const bool has_seen = seen_indptr && n_seen > 0;
    int64_t *d_sptr = nullptr;
    int32_t *d_seen = nullptr;
    if (has_seen) {
        GORSE_TRY(h->use());
        sptr_host.resize((size_t)n_users + 1);
        for (int64_t t = 0; t <= n_users; t++) sptr_host[(size_t)t] = seen_indptr[t] - seen_indptr[0];
        seen_host.assign(seen_items + seen_indptr[0], seen_items + seen_indptr[n_users]);
        parallel_rows(n_users, sptr_host.data(), [&](int, int64_t r0, int64_t r1) {
            for (int64_t r = r0; r < r1; r++) {
                int32_t *b = seen_host.data() + sptr_host[(size_t)r], *e = seen_host.data() + sptr_host[(size_t)r + 1];
                if (e - b > 1 && !std::is_sorted(b, e)) std::sort(b, e);
            }
        });
        Carver in;
        const size_t o_sptr = in.take((size_t)(n_users + 1) * 8), o_seen = in.take((size_t)n_seen * 4);
        GORSE_TRY(h->rec_seen.ensure(in.off));
        d_sptr = (int64_t *)(h->rec_seen.p + o_sptr);
        d_seen = (int32_t *)(h->rec_seen.p + o_seen);
        GORSE_HIP_CHECK(hipMemcpyAsync(d_sptr, sptr_host.data(), (size_t)(n_users + 1) * 8, hipMemcpyHostToDevice, h->stream));
        GORSE_HIP_CHECK(hipMemcpyAsync(d_seen, seen_host.data(), (size_t)n_seen * 4, hipMemcpyHostToDevice, h->stream));
    }
    return mf_recommend_core(h, n_users, users, k, item_ok, d_sptr, d_seen, items_out, scores_out, count_out, nullptr);
}
