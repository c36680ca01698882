// recommend_literal.hip -- gorse_mf_recommend's literal mode 1 (gorse_mf_set_recommend_literal(h, 1)): one workgroup answers one literal
// query end to end, with heap.TopKFilter's heap in LDS.  The result row has the bits of mode 0 (recommend.hip: candidate list ->
// mf_rank_device -> mf_score_device), because the same candidates meet the same GoHeap<false> push / pop in the same order with
// the same score bits; what differs is where the data lives and how many candidates reach the heap at all.
//
// Producer (all four waves).  The catalogue is walked in ascending order in tiles of kRecLitTile items, a tile in kRecLitSegs segments
// of 64 items, segment s of a tile owned by wave s % 4.  A wave tests its 64 items with rec_candidate, keeps the survivors in item
// order by ballot and prefix count in the segment's LDS list, and its four 16-lane groups score the survivors in the reference's
// _mm512_dot order (cf_device.hpp: the bits of gorse_mf_score and of rec_fast_kernel) -- the user's row in registers for d = 16 NC,
// in LDS otherwise, the item's row straight from global memory (64 contiguous bytes per chunk and group).  A segment is written and
// read back by its own wave only, so the producer needs no workgroup barrier; the consumer walks the segments in index order, which is
// item order.  Nothing is materialised in global memory: no candidate list, no pair array, no scores, no counts.
//
// Consumer (wave 0).  It owns the heap, k + 1 entries of (item, score).  Tiles are double-buffered: in round t wave 0 consumes tile t
// and then produces its share of tile t + 1 while the other waves produce theirs; one barrier per tile.  Lane 0 applies
// GoHeap<false>::push and, beyond k entries, ::pop to the buffered candidates in item order.
//
// Fast-forward.  With the heap full (n == k) a candidate with score s < w[0] (strictly) is pushed, rises to the root (it is less than
// every ancestor) and is popped straight away.  Let p_0 = 0, ..., p_m = parent(k) be the ancestors of position k.  The up-sift moves
// w[p_i] to p_{i+1} and w[p_m] to k; the pop puts X = w[p_m] at the root and sifts it down over positions < k.  The arrays come back
// as they were iff X retraces p_1 .. p_m and stops there:
//   at p_i the child p_{i+1} holds A = w[p_i], its sibling still B >= A (the heap property);
//   (a) the swap needs less(child, X): w[p_i] < w[p_m] strictly, for every i < m;
//   (b) a left child p_{i+1} is chosen unless B < A: always; a right child only if A < B: w[p_i] < w[p_{i+1} - 1] strictly;
//   at p_m the only child below k, if any, is k - 1 >= X by the heap property: the sift stops by itself.
// For k = 1, 2 (m = 0) there is no condition.  The heap property is assumed, so a NaN weight that ever entered the heap ends the
// fast-forward for the rest of the query.  Wave 0 keeps the rule's truth value ("ident") and recomputes it in O(log k) after every
// push that reached the heap; while it holds, 64 buffered scores at a time are balloted against the root with !(s < root) -- a NaN
// score passes that test like any score that is not less -- and only the first set bit is pushed, after which the ballot is retaken
// behind it.  While it does not hold (a tie on the ancestor path, a NaN) every candidate takes the serial push / pop.
//
// Drain.  Lane 0 pops the heap empty: pop() leaves each root just past the new end, so afterwards positions 0 .. n - 1 hold the
// entries in PopAll's reversed (descending) order, and the workgroup writes items, weights as scores, the -1 / 0 padding and the
// count into the result row.
#include <algorithm>

#include "goheap.hpp"
#include "rec_internal.hpp"

using namespace gorse;

namespace {

constexpr int kWave = 64;
constexpr int kWaves = kBlock / kWave;
constexpr int kRecLitSteps = 2;                      // segments of a tile per wave
constexpr int kRecLitSegs = kRecLitSteps * kWaves;   // segments of a tile
constexpr int kRecLitTile = kRecLitSegs * kWave;     // catalogue items of a tile
constexpr int64_t kRecLitGrid = 8192;                // workgroups (queries) per launch at most
static_assert(kWave / kGroup == 4, "a wave scores with four 16-lane groups");

int g_rec_lit_no_skip = 0;  // test hook: every candidate takes the serial push / pop

// the fast-forward rule on a full heap of k weights without NaN (file comment): true = push + pop of any s < w[0] is the identity
__device__ __forceinline__ bool rec_lit_identity(const float *w, int k) {
    int c = (k - 1) / 2;  // p_m
    const float wm = w[c];
    bool ok = true;
    while (c > 0) {  // c = p_{i+1}, p = p_i
        const int p = (c - 1) / 2;
        ok = ok && w[p] < wm;
        if ((c & 1) == 0) ok = ok && w[p] < w[c - 1];  // a right child: against its left sibling
        c = p;
    }
    return ok;
}

// NC > 0: d == 16 * NC, the user's row in registers; NC == 0: any d, the user's row in LDS
template <int NC>
__global__ __launch_bounds__(kBlock) void rec_literal_kernel(const RecLiteralArgs A) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int k = A.k, d = A.d, I = A.I;
    float *hw = smem;                                   // k + 1 weights
    int32_t *hv = (int32_t *)(hw + (k + 1));            // k + 1 items
    float *seg_s = (float *)(hv + (k + 1));             // 2 tiles of scores
    int32_t *seg_i = (int32_t *)(seg_s + 2 * kRecLitTile);  // 2 tiles of items
    int32_t *seg_n = seg_i + 2 * kRecLitTile;           // 2 * kRecLitSegs survivor counts
    int32_t *s_n = seg_n + 2 * kRecLitSegs;             // the heap's final count, from wave 0 to the row's writers
    float *urow = (float *)(s_n + 1);                   // d floats (NC == 0)

    const int64_t q = A.q0 + blockIdx.x;
    const int u = A.lit_user[q];
    const int tid = threadIdx.x, wave = tid / kWave, wl = tid % kWave;
    const int lane = tid & (kGroup - 1), grp = wl / kGroup;
    const VecShape vs(d);
    float a[NC > 0 ? NC : 1];
    if constexpr (NC > 0) {
#pragma unroll
        for (int c = 0; c < NC; c++) a[c] = A.P[(int64_t)u * d + 16 * c + lane];
    } else {
        for (int e = tid; e < d; e += kBlock) urow[e] = A.P[(int64_t)u * d + e];
    }
    const int32_t *trow = A.uidx_sorted + A.uptr[u], *srow = nullptr;
    const int64_t tn = A.uptr[u + 1] - A.uptr[u];
    int64_t sn = 0;
    if (A.sptr) {
        const int64_t t = A.lit_query[q];
        srow = A.seen + A.sptr[t];
        sn = A.sptr[t + 1] - A.sptr[t];
    }
    if constexpr (NC == 0) __syncthreads();  // the user's row is in LDS

    // ---- producer: this wave's segments of the tile at t0, into buffer buf
    auto produce = [&](int t0, int buf) {
        for (int st = 0; st < kRecLitSteps; st++) {
            const int seg = st * kWaves + wave;
            const int s0 = t0 + seg * kWave;  // (wave-uniform)
            float *ss = seg_s + (buf * kRecLitSegs + seg) * kWave;
            int32_t *si = seg_i + (buf * kRecLitSegs + seg) * kWave;
            const int item = s0 + wl;
            const bool c = item < I && rec_candidate(A.item_ok, trow, tn, srow, sn, item);
            const unsigned long long b = __ballot(c);
            const int cnt = __popcll(b);
            if (c) si[__popcll(b & ((1ull << wl) - 1ull))] = item;
            if (wl == 0) seg_n[buf * kRecLitSegs + seg] = cnt;
            __threadfence_block();  // the list is read back by other lanes of this wave
            __builtin_amdgcn_wave_barrier();
            for (int j = grp; j < cnt; j += kWave / kGroup) {
                const float *qrow = A.Q + (int64_t)si[j] * d;
                float s;
                if constexpr (NC > 0) {
                    float bq[NC];
#pragma unroll
                    for (int cc = 0; cc < NC; cc++) bq[cc] = qrow[16 * cc + lane];
                    s = dot512_regs<NC>(a, bq);
                } else {
                    s = dot512_lds(urow, qrow, vs, lane);
                }
                if (lane == 0) ss[j] = s;
            }
        }
    };

    // ---- consumer state (wave 0; uniform across its lanes)
    GoHeap<false> heap(hv, hw);
    int n = 0;              // entries of the heap
    int ident = 0;          // the heap is full and push + pop of a score below the root is the identity
    int nan_seen = 0;       // (lane 0) a NaN weight has entered the heap
    unsigned long long pushed = 0, skipped = 0;
    auto consume = [&](int buf) {
        for (int seg = 0; seg < kRecLitSegs; seg++) {
            const int cnt = seg_n[buf * kRecLitSegs + seg];
            const float *ss = seg_s + (buf * kRecLitSegs + seg) * kWave;
            const int32_t *si = seg_i + (buf * kRecLitSegs + seg) * kWave;
            int pos = 0;
            while (pos < cnt) {
                if (ident) {  // fast-forward to the first buffered score that is not below the root
                    const float root = hw[0];
                    const int e = pos + wl;
                    const unsigned long long m = __ballot(e < cnt && !(ss[e] < root));
                    const int f = m ? __ffsll((long long)m) - 1 : cnt - pos;
                    skipped += (unsigned long long)f;
                    pos += f;
                    if (pos >= cnt) break;
                }
                int id = 0;
                if (wl == 0) {
                    const float s = ss[pos];
                    heap.n = n;
                    heap.push(si[pos], s);
                    if (heap.n > k) heap.pop();
                    nan_seen |= s != s;
                    if (heap.n == k && !nan_seen && !A.no_skip) id = rec_lit_identity(hw, k) ? 1 : 0;
                }
                __threadfence_block();  // the root the other lanes read next is lane 0's
                ident = __builtin_amdgcn_readfirstlane(id);
                n = min(n + 1, k);
                pushed++;
                pos++;
            }
        }
    };

    const int ntiles = (I + kRecLitTile - 1) / kRecLitTile;
    if (ntiles > 0) produce(0, 0);
    __syncthreads();
    for (int t = 0; t < ntiles; t++) {
        if (wave == 0) consume(t & 1);
        if (t + 1 < ntiles) produce((t + 1) * kRecLitTile, (t + 1) & 1);
        __syncthreads();
    }

    // ---- drain: PopAll, reversed
    if (tid == 0) {
        *s_n = n;
        heap.n = n;
        while (heap.n > 0) heap.pop();
        atomicAdd(A.stats, pushed);
        atomicAdd(A.stats + 1, skipped);
    }
    __syncthreads();
    n = *s_n;
    const int64_t row = A.scatter ? A.lit_query[q] : q;
    if (tid == 0) A.cnt[row] = n;
    for (int r = tid; r < k; r += kBlock) {
        A.items[row * k + r] = r < n ? hv[r] : -1;
        A.scores[row * k + r] = r < n ? hw[r] : 0.0f;
    }
}

}  // namespace

namespace gorse {

size_t rec_literal_lds(int d, int k) {
    return ((size_t)2 * (k + 1) + (size_t)4 * kRecLitTile + (size_t)2 * kRecLitSegs + 1 + (factor_row_in_registers(d) ? 0 : (size_t)d)) * 4;
}

bool rec_literal_serves(int d, int k) { return k >= 1 && d >= 1 && rec_literal_lds(d, k) <= kRecLiteralLdsBytes; }

int32_t rec_literal_launch(const RecLiteralArgs &A0, int64_t nl, hipStream_t stream) {
    RecLiteralArgs A = A0;
    A.no_skip = g_rec_lit_no_skip;
    const size_t lds = rec_literal_lds(A.d, A.k);
    for (int64_t q0 = 0; q0 < nl; q0 += kRecLitGrid) {
        A.q0 = q0;
        const dim3 grid((unsigned)std::min(kRecLitGrid, nl - q0));
        with_factor_chunks(A.d, [&](auto nc) { rec_literal_kernel<decltype(nc)::value><<<grid, dim3(kBlock), lds, stream>>>(A); });
        GORSE_HIP_CHECK(hipGetLastError());
    }
    return GORSE_OK;
}

}  // namespace gorse

extern "C" int32_t gorse_mf_set_recommend_literal(gorse_mf *h, int32_t mode) {
    if (!h) return fail(GORSE_ERR_INVALID, "handle is NULL");
    if (mode != 0 && mode != 1) return fail(GORSE_ERR_INVALID, "recommend literal mode %d is neither 0 (candidate lists) nor 1 (LDS heap)", mode);
    h->rec_lit_mode = mode;
    return GORSE_OK;
}

extern "C" int32_t gorse_mf_get_recommend_literal(gorse_mf *h, int32_t *requested, int32_t *last_used) {
    if (!h) return fail(GORSE_ERR_INVALID, "handle is NULL");
    if (requested) *requested = h->rec_lit_mode;
    if (last_used) *last_used = h->rec_lit_used;
    return GORSE_OK;
}

extern "C" int32_t gorse_mf_recommend_literal_stats(gorse_mf *h, int64_t *n_queries, int64_t *n_pushed, int64_t *n_skipped) {
    if (!h) return fail(GORSE_ERR_INVALID, "handle is NULL");
    if (n_queries) *n_queries = h->rec_lit_queries;
    if (n_pushed) *n_pushed = h->rec_lit_pushed;
    if (n_skipped) *n_skipped = h->rec_lit_skipped;
    return GORSE_OK;
}

extern "C" void gorse_hip_test_set_recommend_literal(int32_t no_skip) { g_rec_lit_no_skip = no_skip ? 1 : 0; }
