// topk_tie.hip -- the tie path of path B of the exact top-k (topk_mfma.hip): the reference's heap history of one query, rebuilt
// from list + history.
// The rescoring kernel hands over queries whose top k+1 exact distances are not all distinct: there the reference's
// answer depends on the ARRANGEMENT of its heap array, i.e. on everything Bruteforce pushed (bruteforce.go:46-53:
// Push, then Pop when the queue holds more than k).  A history sweep (HIST) has recorded, for such a query, every
// vector whose approximate score reached the filter threshold of its time.  A vector that was NOT recorded had
// approx < threshold = (K-th best approx among earlier vectors) - 2 delta, so at least k EARLIER vectors are strictly
// closer in exact arithmetic: the reference pushed it to the root and popped it straight away.  Such a push/pop pair
// (operator T below) depends only on the heap state, not on the vector -- it is the identity unless equal distances
// sit on the path it touches, and then it permutes them with a short period (<= ~log2 k).  So the replay is: exact
// distances for the recorded vectors (reference arithmetic), sort by index, literal container/heap Push/Pop for each
// (goheap.hpp), and T^gap for every gap of unrecorded vectors in between, T^gap evaluated by cycle detection.
// Queries with a NaN, an overflowed history or an undetected cycle are flagged 2 and go to path A.
// (ReplayParams, the kernels' parameter block: topk_mfma_internal.hpp.)
#include <type_traits>

#include "topk_mfma_internal.hpp"

using namespace gorse;

namespace {

// stage 1 of the tie path: exact distances (the reference's arithmetic) of one query's recorded vectors, sorted by
// index; one workgroup per query, everything parallel.  Output: sidx / sdst (kReplayCap slots per query), scount.
__global__ __launch_bounds__(kBlock) void topk_tie_sort_kernel(ReplayParams p) {
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    const int d = p.d;
    int *s_idx = reinterpret_cast<int *>(smem_f);           // kReplayCap
    float *s_dst = smem_f + kReplayCap;                      // kReplayCap
    float *sq = s_dst + kReplayCap;                          // d
    float *sx = sq + d;                                      // kGroupsPerBlock * d
    int *s_misc = reinterpret_cast<int *>(sx + (size_t)kGroupsPerBlock * d);  // [0] NaN seen, [1] recorded rows kept by the join
    const int64_t t = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & (kGroup - 1), gib = tid / kGroup;
    // Join of the row slices.  Slice s swept its rows from a cold threshold, so its list + history hold every row of the slice
    // whose approximate score reached (K-th best approximate score among the slice's EARLIER rows) - 2 delta -- a superset
    // of what an unsliced sweep records there, and far too many.  A row of slice s is needed only if its score reaches
    // F_s = max over the earlier slices u < s of f_u, f_u = the threshold slice u ended with = (a lower bound of the K-th
    // best approximate score of slice u's rows) - 2 delta: a row below F_s has at least K earlier rows whose approximate
    // scores exceed its own by more than 2 delta, i.e. K earlier rows that are strictly closer in exact arithmetic, which
    // is the replay's condition for treating it as one of the unrecorded rows of a gap (see the head of this file).
    int *s_n = s_misc + 1;
    bool flagged = false;
    for (int sl = 0; sl < p.nslices; sl++) flagged |= p.cflag[(int64_t)sl * p.nq + t] != 0;
    if (flagged) {  // some slice could not hold this query (overflow): path A
        if (tid == 0) p.cflag[t] = 1;
        return;
    }
    const int64_t self = p.self[t];
    const int64_t row = p.pos[t];
    const float *qrow = p.Qf ? p.Qf + row * d : p.X + self * d;
    for (int e = tid; e < d; e += kBlock) sq[e] = qrow[e];
    if (tid == 0) s_misc[0] = 0, s_n[0] = 0;
    __syncthreads();
    float fprev = -__builtin_inff();
    for (int sl = 0; sl < p.nslices; sl++) {
        const int64_t qs = (int64_t)sl * p.nq + t;
        const int n1 = p.ccnt[qs], n2 = p.hcnt[qs];
        const uint2 *cb = p.cbuf + qs * kCap, *hb = p.hbuf + qs * kHistCap;
        for (int c = tid; c < n1 + n2; c += kBlock) {
            const uint2 ent = c < n1 ? cb[c] : hb[c - n1];
            if (fkey_inv(ent.x) >= fprev) {
                const int at = atomicAdd(s_n, 1);
                if (at < kReplayCap) s_idx[at] = (int)ent.y;
            }
        }
        fprev = fmaxf(fprev, p.fslice[qs]);
    }
    __syncthreads();
    const int n = s_n[0];
    if (n > kReplayCap) {  // more recorded rows than the replay sorts: path A
        if (tid == 0) p.cflag[t] = 1;
        return;
    }
    __syncthreads();
    const VecShape vs(d);
    const float qq = p.metric == GORSE_METRIC_COSINE ? p.qn2[row] : 0.0f;
    for (int c = gib; c < n; c += kGroupsPerBlock) {  // exact distances, as topk_rescore_kernel
        const int64_t i = s_idx[c];
        float *xr = sx + (size_t)gib * d;
        gather_row(xr, p.X, p.Xb, i, d, lane);
        __builtin_amdgcn_wave_barrier();
        float r;
        if (p.metric == GORSE_METRIC_EUCLIDEAN || p.metric == kMetricEuclidBf16) {
            r = euclid_any_lds(p.metric, sq, xr, vs, lane);
        } else {
            const float ab = dot512_lds(sq, xr, vs, lane);
            if (p.metric == GORSE_METRIC_NEG_DOT)
                r = -ab;
            else
                r = cosine_distance(ab, qq, p.norm2[i]);
        }
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) {
            s_dst[c] = r;
            if (r != r) s_misc[0] = 1;
        }
    }
    int P = 2;
    while (P < n) P <<= 1;
    for (int c = n + tid; c < P; c += kBlock) {
        s_idx[c] = 0x7fffffff;
        s_dst[c] = 0.0f;
    }
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1)  // bitonic sort by index
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int e = tid; e < P / 2; e += kBlock) {
                const int a = (e / stride) * 2 * stride + (e % stride), b = a + stride;
                const bool up = (a & size) == 0;
                const int ia = s_idx[a], ib = s_idx[b];
                if ((ia > ib) == up) {
                    s_idx[a] = ib;
                    s_idx[b] = ia;
                    const float da = s_dst[a];
                    s_dst[a] = s_dst[b];
                    s_dst[b] = da;
                }
            }
            __syncthreads();
        }
    for (int c = tid; c < n; c += kBlock) {
        p.sidx[t * kReplayCap + c] = s_idx[c];
        p.sdst[t * kReplayCap + c] = s_dst[c];
    }
    if (tid == 0) p.scount[t] = s_misc[0] ? -1 : n;  // -1: a NaN distance (the reference panics on it): path A
}

// ---- stage 2 of the tie path: the replay, one LANE per query ------------------------------------------------------
// The replay is scalar work: round 2's kernel, a wave per query with the heap in registers, issued ~1.8 M cycles of readlane /
// writelane traffic per query (18 ms for the 9,934 tie queries of C4, profiles/r03_r_probe_c4_replay.txt).  Here every lane
// replays its own query over the sorted entries (see the head of this file) and keeps its heap in its own LDS column (slot j of lane q at word j * QPW + q: bank q whatever the slot, so the
// lanes never conflict, and no lane ever reads another's column: no barriers).  The ancestors of a push and the path of
// the identity test are known before the first comparison, so their weights are read together -- one LDS round trip
// instead of one per level; only the pop walks level by level.
constexpr int kLaneDepth = 8;   // ancestors of slot 256
template <bool DESC, int stride>
struct LaneHeap {
    int *W, *V;  // this lane's column: slot j at [j * stride]
    int n;
    __device__ __forceinline__ static bool less(float a, float b) { return DESC ? a > b : a < b; }
    __device__ __forceinline__ float getw(int j) const { return __int_as_float(W[j * stride]); }
    __device__ __forceinline__ int getv(int j) const { return V[j * stride]; }
    // log (probe of change): slot and old value of everything written, when lg != nullptr
    int *lg;
    int nlog;
    __device__ __forceinline__ void set(int j, float wt, int val) {
        if (lg) {
            if (nlog < kLaneLog) {
                lg[(2 * nlog) * stride] = j;
                lg[(2 * nlog + 1) * stride] = V[j * stride];
            }
            nlog++;
        }
        W[j * stride] = __float_as_int(wt);
        V[j * stride] = val;
    }
    __device__ __forceinline__ void push(int val, float wt) {  // heap.Push: append, up(n - 1)
        int j = n++;
        int anc[kLaneDepth], av[kLaneDepth];
        float aw[kLaneDepth];
        int a = j;
#pragma unroll
        for (int l = 0; l < kLaneDepth; l++) {
            const bool ok = a > 0;
            a = ok ? (a - 1) / 2 : 0;
            anc[l] = ok ? a : -1;
            aw[l] = getw(a);
            av[l] = getv(a);
        }
#pragma unroll
        for (int l = 0; l < kLaneDepth; l++) {
            if (anc[l] < 0 || !less(wt, aw[l])) break;
            set(j, aw[l], av[l]);
            j = anc[l];
        }
        set(j, wt, val);
    }
    __device__ __forceinline__ void pop(int &val, float &wt) {  // heap.Pop: swap(0, n - 1), down(0, n - 1), take the last
        val = getv(0);
        wt = getw(0);
        const int m = --n;
        if (m == 0) return;
        const float wl = getw(m);
        const int vl = getv(m);
        int i = 0;
        for (;;) {
            const int j1 = 2 * i + 1;
            if (j1 >= m) break;
            const bool two = j1 + 1 < m;
            const int j2 = two ? j1 + 1 : j1;
            const float w1 = getw(j1), w2 = getw(j2);
            const int v1 = getv(j1), v2 = getv(j2);
            int j = j1, vj = v1;
            float wj = w1;
            if (two && less(w2, wj)) {
                j = j2;
                wj = w2;
                vj = v2;
            }
            if (!less(wj, wl)) break;
            set(i, wj, vj);
            i = j;
        }
        set(i, wl, vl);
    }
};

template <int QPW>  // queries (= active lanes) per workgroup: a constant so that a slot's address is a shift
__global__ __launch_bounds__(64) void topk_tie_replay_lane_kernel(ReplayParams p, int64_t nq, int slots) {
    constexpr int qpw = QPW;
    extern __shared__ int smem_i[];
    const int lane = threadIdx.x;
    const int64_t t = (int64_t)blockIdx.x * qpw + lane;
    if (lane >= qpw || t >= nq) return;
    if (p.cflag[t]) return;
    int *W = smem_i + lane, *V = W + slots * qpw, *LG = V + slots * qpw, *SN = LG + 2 * kLaneLog * qpw;  // SN: a snapshot of V
    const int n = p.scount[t];
    const int k = p.k;
    const int64_t self = p.self[t];
    const int64_t row = p.pos[t];
    bool undecided = n < 0;
    const float kInf = __builtin_inff();
    const unsigned long long t_begin = p.prof ? __builtin_amdgcn_s_memtime() : 0;
    unsigned long long n_push = 0, n_tpow = 0, n_slow_tpow = 0, n_T = 0;
    LaneHeap<true, QPW> mx;
    mx.W = W, mx.V = V, mx.n = 0, mx.lg = nullptr, mx.nlog = 0;
    // T leaves the heap array as it is unless equal weights sit where its push and pop look.  With the heap full (n = k),
    // push(+inf) climbs from slot n to the root and shifts the path's elements down one level; pop then sends the element
    // E that came to rest in slot n (the old occupant of slot p1 = parent(n)) back down from the root, and every level
    // restores its old occupant iff (a) the path's child wins the comparison of the two children -- certain when it is the
    // LEFT child (container/heap prefers the left on a tie), and when it is the right child only if the old parent is
    // strictly greater than the left child -- and (b) the old parent is strictly greater than E.  E then stops in p1, whose
    // remaining child cannot beat it.  A dozen comparisons instead of two sift passes and a snapshot compare
    // (tests/test_replay_claim_cpu.py checks the criterion against the literal T).  The path's weights are read before the
    // first comparison.
    auto t_is_identity = [&]() -> bool {
        const int hn = mx.n;
        if (hn < 1) return false;
        int child = (hn - 1) / 2;  // p1
        const float e = mx.getw(child);
        float wp[kLaneDepth], ws[kLaneDepth];
        bool has[kLaneDepth], right[kLaneDepth];
        int c = child;
#pragma unroll
        for (int l = 0; l < kLaneDepth; l++) {
            has[l] = c > 0;
            const int parent = has[l] ? (c - 1) / 2 : 0;
            right[l] = has[l] && (c & 1) == 0;
            wp[l] = mx.getw(parent);
            ws[l] = mx.getw(right[l] ? c - 1 : 0);
            c = parent;
        }
        if (!(e < kInf)) return false;
#pragma unroll
        for (int l = 0; l < kLaneDepth; l++) {
            if (!has[l]) break;
            if (!(wp[l] > e) || !(wp[l] < kInf)) return false;
            if (right[l] && !(wp[l] > ws[l])) return false;
        }
        return true;
    };
    auto apply_T = [&]() {  // a push that goes to the root and is popped at once
        int dv;
        float dw;
        mx.push(-1, kInf);
        mx.pop(dv, dw);
    };
    // T^gap when T is not the identity: literal applications until nothing changes (the change is read off the log of
    // what T wrote: a fixpoint is the usual case, else this is the pre-period), then the search for the period against a
    // snapshot of the values
    auto t_pow = [&](int64_t gap) {
        n_tpow++;
        if (t_is_identity()) return;
        n_slow_tpow++;
        int64_t steps = 0;
        while (steps < gap && steps < 16) {
            const int before = mx.n;
            mx.lg = LG;
            mx.nlog = 0;
            apply_T();
            mx.lg = nullptr;
            steps++;
            n_T++;
            bool same = mx.nlog <= kLaneLog;
            for (int r = 0; r < mx.nlog && same; r++) {
                const int sl = LG[(2 * r) * qpw];
                if (sl < before && V[sl * qpw] != LG[(2 * r + 1) * qpw]) same = false;
            }
            if (same) return;
        }
        if (steps == gap) return;
        const int hn = mx.n;
        for (int sl = 0; sl < hn; sl++) SN[sl * qpw] = V[sl * qpw];  // inside the cycle now (or not: then the query is flagged)
        int64_t period = 0;
        bool closed = false;
        while (period < 64) {
            apply_T();
            period++;
            steps++;
            n_T++;
            if (steps == gap) return;
            bool same = true;
            for (int sl = 0; sl < hn && same; sl++) same = SN[sl * qpw] == V[sl * qpw];
            if (same) {
                closed = true;
                break;
            }
        }
        if (!closed) {
            undecided = true;
            return;
        }
        const int64_t rem = (gap - steps) % period;
        for (int64_t r = 0; r < rem; r++) apply_T();
    };
    const int32_t *sidx = p.sidx + t * kReplayCap;
    const float *sdst = p.sdst + t * kReplayCap;
    int64_t prev = -1;
    int64_t pend = 0;
    // Lanes run in step, so an entry that only counts (strictly worse than a full heap's root: the reference pushes it to the
    // root and pops it at once) must not cost its lane a turn of the heap work the others do: every lane first walks over
    // such entries (inner loop), then the lanes that stopped at a real push do it together.
    float rootw = kInf;  // W[0] of a non-empty heap
    int e0 = 0;
    int nxt_i = n > 0 ? sidx[0] : 0;  // one entry ahead (16-byte groups two ahead were slower: profiles/r03_v_kernel_stats_default.txt)
    float nxt_d = n > 0 ? sdst[0] : 0.0f;
    while (e0 < n && !undecided) {
        int64_t i = 0;
        float dd = 0.0f;
        bool have = false;
        while (e0 < n) {
            i = nxt_i;
            dd = nxt_d;
            e0++;
            if (e0 < n) {
                nxt_i = sidx[e0];
                nxt_d = sdst[e0];
            }
            if (i == self) continue;
            if (i == prev) {
                undecided = true;
                break;
            }
            int64_t gap = i - prev - 1;
            if (self > prev && self < i) gap--;
            if (gap > 0 && mx.n < k) {
                undecided = true;
                break;
            }
            pend += gap;
            prev = i;
            if (mx.n == k && dd > rootw) {
                pend++;
                continue;
            }
            have = true;
            break;
        }
        if (!have || undecided) break;
        if (pend > 0) {
            t_pow(pend);
            pend = 0;
            if (undecided) break;
        }
        n_push++;
        mx.push((int32_t)i, dd);
        if (mx.n > k) {
            int dv;
            float dw;
            mx.pop(dv, dw);
        }
        rootw = mx.getw(0);
    }
    if (!undecided) {
        int64_t gap = p.N - 1 - prev;
        if (self > prev) gap--;
        if (gap > 0 && mx.n < k) undecided = true;
        pend += gap;
        if (!undecided && pend > 0) t_pow(pend);
    }
    if (p.prof) {
        const unsigned long long dt = __builtin_amdgcn_s_memtime() - t_begin;
        atomicAdd(p.prof + 0, dt);
        atomicMax(p.prof + 1, dt);
        atomicAdd(p.prof + 2, (unsigned long long)(n > 0 ? n : 0));
        atomicAdd(p.prof + 3, 1ull);
        atomicAdd(p.prof + 4, n_push);
        atomicAdd(p.prof + 5, n_tpow);
        atomicAdd(p.prof + 6, n_slow_tpow);
        atomicAdd(p.prof + 7, n_T);
        atomicMax(p.prof + 8, n_T);
        atomicMax(p.prof + 9, (unsigned long long)(n > 0 ? n : 0));
        atomicAdd(p.prof + 10, undecided ? 1ull : 0ull);
    }
    if (undecided) {
        p.cflag[t] = 2;
        return;
    }
    // Reverse(): re-push in array order (pq.go:121-128) -- in place: the min-heap of the first e entries lives in the slots
    // the max-heap's first e entries have been read from
    const int hn = mx.n;
    LaneHeap<false, QPW> mn;
    mn.W = W, mn.V = V, mn.n = 0, mn.lg = nullptr, mn.nlog = 0;
    for (int e = 0; e < hn; e++) {
        const int val = V[e * qpw];
        const float wt = __int_as_float(W[e * qpw]);
        mn.push(val, wt);
    }
    int cnt = 0;
    while (mn.n > 0) {
        int v;
        float w;
        mn.pop(v, w);
        if (!p.prune0 || w > 0) {
            p.out_idx[row * k + cnt] = v;
            p.out_dist[row * k + cnt] = w;
            cnt++;
        }
    }
    p.out_cnt[row] = cnt;
    for (int e = cnt; e < k; e++) {
        p.out_idx[row * k + e] = -1;
        p.out_dist[row * k + e] = kInf;
    }
}

// rows pos[t] of a bf16 operand matrix / a float vector -> compact arrays of the flagged queries
__global__ void gather_pos_kernel(const uint16_t *__restrict__ op, const float *__restrict__ margin,
                                  const int32_t *__restrict__ pos, int kpad, uint16_t *__restrict__ op_out,
                                  float *__restrict__ margin_out) {
    const int64_t t = blockIdx.x;
    const int64_t src = pos[t];
    const uint4 *s = reinterpret_cast<const uint4 *>(op + src * kpad);
    uint4 *o = reinterpret_cast<uint4 *>(op_out + t * kpad);
    for (int e = threadIdx.x; e < kpad / 8; e += blockDim.x) o[e] = s[e];
    if (threadIdx.x == 0) margin_out[t] = margin[src];
}

// The history sweep's row slices need not start cold (round 6).  A slice that starts at row r_s may drop every row whose approximate
// score stays below (K-th best approximate score among ANY set of rows in front of r_s) - 2 delta: at least K earlier rows are then
// strictly closer in exact arithmetic, and the reference's heap pushed such a row to its root and popped it at once (the head of this file).
// The main sweep's lists of a flagged query -- its own list and, after a symmetric sweep, its foreign list: ~270 distinct rows with
// their approximate scores, whatever became of the query's thresholds -- are such a set: one wave per flagged query takes the list
// entries in front of every slice and, where there are at least kth of them, leaves a lower bound of their kth-th best score minus
// the query's margin as the slice's starting threshold (the bound as compact_query forms it: the 16 leading key bits).  Slice 0 and
// the slices with fewer than kth list entries in front of them start cold (-inf).  At C4: ~270 entries per query, so from the fourth
// slice of eight on a slice records the few dozen rows that reach its bound instead of the ~710 a cold start accepts.
__global__ __launch_bounds__(64) void tie_warm_kernel(WarmParams p) {
    const int64_t t = blockIdx.x;
    const int lane = threadIdx.x;
    const int64_t q = p.pos[t];
    constexpr int EPL = kCapT / 64;  // at most kCapT entries are looked at: any subset of the lists is a valid set
    int n_at[kMaxOwnSlices + 2];
    n_at[0] = 0;
#pragma unroll
    for (int sl = 0; sl < kMaxOwnSlices; sl++) {
        int c = sl < p.own_slices ? p.ccnt[(int64_t)sl * p.own_stride + q] : 0;
        c = c < 0 ? 0 : (c > kCap ? kCap : c);
        n_at[sl + 1] = n_at[sl] + c;
    }
    int nf = p.fbuf ? p.fcnt[q] : 0;
    nf = nf < 0 ? 0 : (nf > kCapF ? kCapF : nf);
    const int n_own = n_at[kMaxOwnSlices];
    const int n_all = n_own + nf < kCapT ? n_own + nf : kCapT;
    uint32_t key[EPL];
    int64_t row[EPL];
#pragma unroll
    for (int j = 0; j < EPL; j++) {
        const int c = j * 64 + lane;
        uint2 ent = make_uint2(0u, 0u);
        if (c < n_all) {
            if (c >= n_own) {
                ent = p.fbuf[q * kCapF + (c - n_own)];
            } else {
                int sl = 0;
#pragma unroll
                for (int u = 1; u < kMaxOwnSlices; u++) sl += c >= n_at[u] ? 1 : 0;
                ent = p.cbuf[((int64_t)sl * p.own_stride + q) * kCap + (c - n_at[sl])];
            }
        }
        key[j] = c < n_all ? ent.x : 0u;
        row[j] = c < n_all ? (int64_t)ent.y : p.N;
    }
    const float mg = p.margin[t];
    const int64_t nt_all = (p.N + p.tile_rows - 1) / p.tile_rows;
    for (int s = 0; s < p.nsl; s++) {
        const int64_t r_s = (nt_all * s / p.nsl) * p.tile_rows;  // topk_sweep_kernel: the slice's first tile T0 = NT_all * y / slices
        uint32_t k_in[EPL];
        int cnt = 0;
#pragma unroll
        for (int j = 0; j < EPL; j++) {
            k_in[j] = row[j] < r_s ? key[j] : 0u;  // key 0: never counted (trial >= 2^16)
            cnt += __builtin_popcountll(__builtin_amdgcn_ballot_w64(k_in[j] != 0u));
        }
        float f = -__builtin_inff();
        if (s > 0 && cnt >= p.kth) {
            uint32_t prefix = 0;
            for (int b = 31; b >= 16; --b) {
                const uint32_t trial = prefix | (1u << b);
                int c = 0;
#pragma unroll
                for (int j = 0; j < EPL; j++) c += __builtin_popcountll(__builtin_amdgcn_ballot_w64(k_in[j] >= trial));
                if (c >= p.kth) prefix = trial;
            }
            f = fkey_inv(prefix) - mg;
        }
        if (lane == 0) p.fwarm[(int64_t)s * p.m2 + t] = f;
    }
}

}  // namespace

// One replay chunk: the flagged queries' operands and margins gathered, the slices' starting thresholds, the history sweep, the sort
// of every query's recorded rows, the lane replay, and the flags of what the replay left undecided back on the host.
int32_t gorse::tie_replay_chunk(gorse_topk *h, const ChunkState &cs, int64_t f0, int64_t m2, std::vector<uint8_t> &flags) {
    const int d = h->d, kpad = h->kp * 16, k = cs.k;
    const bool sym = cs.sym;
    const int32_t *pos_dev = h->fl_pos.p + f0;
    const int64_t *self_dev = h->fl_self.p + f0;
    GORSE_TRY(h->rp_op.ensure((size_t)m2 * kpad));
    GORSE_TRY(h->rp_margin.ensure((size_t)m2));
    const int nsl = hist_slices(g_topk_variant, h->N, m2);  // row slices (topk_plan.hpp)
    const size_t sm2 = (size_t)nsl * (size_t)m2;
    GORSE_TRY(h->rp_cbuf.ensure(sm2 * kCap));
    GORSE_TRY(h->rp_hbuf.ensure(sm2 * kHistCap));
    GORSE_TRY(h->rp_ccnt.ensure(sm2));
    GORSE_TRY(h->rp_hcnt.ensure(sm2));
    GORSE_TRY(h->rp_flag.ensure(sm2));
    GORSE_TRY(h->rp_fslice.ensure(sm2));
    gather_pos_kernel<<<dim3((unsigned)m2), dim3(64), 0, h->stream>>>(cs.Bop, h->qmargin.p, pos_dev, kpad,
                                                                     h->rp_op.p, h->rp_margin.p);
    GORSE_HIP_CHECK(hipGetLastError());
    GORSE_HIP_CHECK(hipMemsetAsync(h->rp_flag.p, 0, sm2, h->stream));
    GORSE_HIP_CHECK(hipMemsetAsync(h->rp_hcnt.p, 0, sm2 * 4, h->stream));
    GORSE_HIP_CHECK(hipMemsetAsync(h->rp_ccnt.p, 0, sm2 * 4, h->stream));
    SweepParams hp = cs.sp;
    hp.f0 = nullptr;  // the history sweep records what a threshold that starts at -inf would have kept
    hp.fwarm = nullptr;
    // ... or, slice by slice, what a threshold that starts at a bound the main sweep's lists prove would have kept
    // (tie_warm_kernel; COLD_SLICES: every slice cold, the form of rounds 2-5)
    if (nsl > 1 && !(g_topk_variant & GORSE_TEST_TOPK_COLD_SLICES)) {
        GORSE_TRY(h->rp_fwarm.ensure(sm2));
        WarmParams wp;
        wp.pos = pos_dev, wp.m2 = m2, wp.N = h->N, wp.nsl = nsl, wp.tile_rows = kHistTileRows, wp.kth = cs.kth;
        wp.cbuf = h->cbuf.p, wp.ccnt = h->ccnt.p;
        wp.own_slices = sym ? std::max(1, cs.sym_slices) : 1, wp.own_stride = cs.mb;
        wp.fbuf = sym ? h->fbuf.p : nullptr, wp.fcnt = sym ? h->fcnt.p : nullptr;
        wp.margin = h->rp_margin.p;
        wp.fwarm = h->rp_fwarm.p;
        tie_warm_kernel<<<dim3((unsigned)m2), dim3(64), 0, h->stream>>>(wp);
        GORSE_HIP_CHECK(hipGetLastError());
        hp.fwarm = h->rp_fwarm.p;
    }
    hp.B = h->rp_op.p;
    hp.qmargin = h->rp_margin.p;
    hp.cbuf = h->rp_cbuf.p;
    hp.ccnt = h->rp_ccnt.p;
    hp.cflag = h->rp_flag.p;
    hp.hbuf = h->rp_hbuf.p;
    hp.hcnt = h->rp_hcnt.p;
    hp.f_out = h->rp_fslice.p;
    hp.nslices = nsl;
    hp.nq = m2;
    int tok = h->prof.begin(GORSE_PROF_TOPK_HIST, h->stream);
    GORSE_TRY(dispatch_sweep(h, hp, true));
    h->prof.end(tok, h->stream);
    ReplayParams pp;
    pp.X = h->X.p;
    pp.Xb = h->dtype == GORSE_DTYPE_BF16 ? h->Xb.p : nullptr;
    pp.norm2 = h->norm2.p;
    pp.Qf = cs.Qf;
    pp.qn2 = cs.qn2;
    pp.self = self_dev;
    pp.pos = pos_dev;
    pp.cbuf = h->rp_cbuf.p;
    pp.ccnt = h->rp_ccnt.p;
    pp.hbuf = h->rp_hbuf.p;
    pp.hcnt = h->rp_hcnt.p;
    pp.fslice = h->rp_fslice.p;
    pp.nslices = nsl;
    pp.prof = (g_topk_variant & GORSE_TEST_TOPK_REPLAY_COUNTERS) && h->sweep_prof.n >= 16 ? h->sweep_prof.p : nullptr;
    if (pp.prof) GORSE_HIP_CHECK(hipMemsetAsync(pp.prof, 0, 16 * sizeof(unsigned long long), h->stream));
    pp.nq = m2;
    pp.cflag = h->rp_flag.p;
    pp.N = h->N;
    pp.d = d;
    pp.metric = h->kernel_metric();
    pp.k = k;
    pp.prune0 = cs.prune0;
    pp.out_idx = h->res_idx.p;
    pp.out_dist = h->res_dist.p;
    pp.out_cnt = h->res_cnt.p;
    GORSE_TRY(h->rp_sidx.ensure((size_t)m2 * kReplayCap));
    GORSE_TRY(h->rp_sdst.ensure((size_t)m2 * kReplayCap));
    GORSE_TRY(h->rp_scount.ensure((size_t)m2));
    pp.sidx = h->rp_sidx.p;
    pp.sdst = h->rp_sdst.p;
    pp.scount = h->rp_scount.p;
    const size_t rlds = tie_sort_lds_bytes(d, kGroupsPerBlock);
    GORSE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&topk_tie_sort_kernel),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)rlds));
    tok = h->prof.begin(GORSE_PROF_TOPK_REPLAY, h->stream);
    topk_tie_sort_kernel<<<dim3((unsigned)m2), dim3(kBlock), rlds, h->stream>>>(pp);
    GORSE_HIP_CHECK(hipGetLastError());
    {  // one lane per query
        const int slots = k + 1;
        const int qpw = replay_queries_per_wave(g_topk_variant, slots, m2);
        const size_t llds = lane_lds_bytes(slots, qpw);
        auto launch_lanes = [&](auto tag) -> int32_t {
            constexpr int Q = decltype(tag)::value;
            GORSE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&topk_tie_replay_lane_kernel<Q>),
                                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)llds));
            topk_tie_replay_lane_kernel<Q><<<dim3((unsigned)ceil_div(m2, Q)), dim3(64), llds, h->stream>>>(pp, m2, slots);
            GORSE_HIP_CHECK(hipGetLastError());
            return GORSE_OK;
        };
        if (qpw == 64) GORSE_TRY(launch_lanes(std::integral_constant<int, 64>()));
        else if (qpw == 32) GORSE_TRY(launch_lanes(std::integral_constant<int, 32>()));
        else GORSE_TRY(launch_lanes(std::integral_constant<int, 16>()));
    }
    h->prof.end(tok, h->stream);
    flags.resize((size_t)m2);
    GORSE_HIP_CHECK(hipMemcpyAsync(flags.data(), h->rp_flag.p, (size_t)m2, hipMemcpyDeviceToHost, h->stream));
    GORSE_HIP_CHECK(hipStreamSynchronize(h->stream));
    return GORSE_OK;
}
