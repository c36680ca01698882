// topk_rescore.hip -- the second stage of path B of the exact top-k (topk_mfma.hip): the candidate lists the sweep left are rescored
// in the reference's own arithmetic order and ranked; the queries that cannot be decided from their lists (ties in the top k + 1,
// NaN, an overflowed list, a warm start that cannot be verified) are flagged and listed for the tie path (topk_tie.hip).
#include "topk_mfma_internal.hpp"

using namespace gorse;

namespace {

// ---- exact rescoring + ranking of one query's candidate list ------------------------------------------
__global__ __launch_bounds__(kBlock) void topk_rescore_kernel(RescoreParams p) {
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    const int d = p.d;
    float *sq = smem_f;                          // d
    float *sx = sq + d;                          // 2 * kGroupsPerBlock * d
    float *s_e = sx + (size_t)2 * kGroupsPerBlock * d;  // kCapT
    int *s_i = reinterpret_cast<int *>(s_e + kCapT);  // kCapT
    int *s_misc = s_i + kCapT;                   // [0] nonpositive in top-k, [1] flag, [2] SYM: candidates that clear the warm start,
                                                 // [3], [4] the histogram selection's bin and remainder, [5] survivors of the pruning
    const int64_t t = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & (kGroup - 1), gib = tid / kGroup;
    const int k = p.k;
    if (p.tri_world > 1 && (int)((t / p.tri_bq) % p.tri_world) != p.tri_rank) return;  // another rank's query
    // SYM with row slices (a triangle shard whose long blocks are cut over several workgroups: topk_sweep_kernel, sym_slices): the
    // query has one own list, counter, flag and final threshold PER SLICE, slice-major like a history sweep's
    const int nsl = p.own_slices > 1 ? p.own_slices : 1;
    {
        uint8_t f = p.cflag[t];
        for (int sl = 1; sl < nsl; sl++) {
            const uint8_t g = p.cflag[(int64_t)sl * p.own_stride + t];
            f = f ? f : g;
        }
        if (f) {  // path A / the tie path fills this row (a flag of a later slice moves to where the host's list is made from)
            if (tid == 0 && !p.cflag[t]) p.cflag[t] = f;
            return;
        }
    }
    int n_own_at[kMaxOwnSlices + 1];
    n_own_at[0] = 0;
#pragma unroll
    for (int sl = 0; sl < kMaxOwnSlices; sl++) n_own_at[sl + 1] = n_own_at[sl] + (sl < nsl ? p.ccnt[(int64_t)sl * p.own_stride + t] : 0);
    const int n_own = n_own_at[kMaxOwnSlices];
    const int n_for = p.fbuf ? p.fcnt[t] : 0;
    if (n_for > kCapF || n_own + (n_for > 0 ? n_for : 0) > kCapT) {  // the foreign list overflowed (or, sliced, the lists together exceed
        if (tid == 0) {                                                // what this kernel ranks): the tie path sweeps this query on its own
            p.cflag[t] = 1;
            atomicAdd(p.sym_stats + 2, 1ull);
        }
        return;
    }
    const int n_all = n_own + n_for;
    const uint2 *fb = p.fbuf ? p.fbuf + t * kCapF : nullptr;
    const int64_t self = p.Qf ? -1 : (p.qid ? p.qid[t] : p.q0 + t);
    const float *qrow = p.Qf ? p.Qf + t * d : p.X + self * d;
    for (int e = tid; e < d; e += kBlock) sq[e] = qrow[e];
    if (tid < 6) s_misc[tid] = 0;
    __syncthreads();
    const VecShape vs(d);
    const float qq = p.metric == GORSE_METRIC_COSINE ? p.qn2[t] : 0.0f;
    const uint2 *cb = p.cbuf + t * kCap;
    // the candidates into registers: kCapT / kBlock per thread
    constexpr int EPT = kCapT / kBlock;
    uint32_t ekey[EPT], eidx[EPT];
    bool ev[EPT];
#pragma unroll
    for (int s = 0; s < EPT; s++) {
        const int c = tid + s * kBlock;
        ev[s] = c < n_all;
        uint2 ent = make_uint2(0u, 0u);
        if (ev[s]) {
            if (c >= n_own) {
                ent = fb[c - n_own];
            } else {
                int sl = 0;
#pragma unroll
                for (int u = 1; u < kMaxOwnSlices; u++) sl += c >= n_own_at[u] ? 1 : 0;
                ent = cb[(int64_t)sl * p.own_stride * kCap + (c - n_own_at[sl])];
            }
        }
        ekey[s] = ent.x;
        eidx[s] = ent.y;
    }
    // SYM: a warm start that the query's own list could not verify is verified here over both lists -- the threshold f0 is valid
    // iff (kth-th best approximate score) - margin >= f0, and with the own threshold still at f0 the two lists hold every row that
    // reaches f0.  (A final own threshold above f0 was derived from -- and verified by -- the own list; f0 = -inf needs no proof.)
    const float mg = p.qmargin[t];
    // (sliced: a slice that raised its threshold above f0 proved f0 over its own rows, a subset of all rows: that verifies it)
    float ffin = p.fbuf ? p.ffinal[t] : 0.0f;
    for (int sl = 1; sl < nsl && p.fbuf; sl++) ffin = fmaxf(ffin, p.ffinal[(int64_t)sl * p.own_stride + t]);
    const bool verify = p.fbuf && p.f0[t] > -__builtin_inff() && !(ffin > p.f0[t]);
    if (verify) {
        const float f0 = p.f0[t];
        int c_ok = 0;
#pragma unroll
        for (int s = 0; s < EPT; s++) c_ok += ev[s] && fkey_inv(ekey[s]) - mg >= f0;
        if (c_ok) atomicAdd(&s_misc[2], c_ok);
    }
    // Pruning by the approximate scores (round 5): only a row whose approximate score reaches (kth-th best approximate score of the
    // lists) - margin can be among the kth best in exact arithmetic -- the sweep's own rule, applied once more to what the lists hold
    // at the end (thresholds frozen for the foreign side, never tightened for a short own part: ~270 entries at C4, ~110 of which
    // pass) -- so the exact distances, whose gathers are this kernel's time, and the sort are those of the survivors.  The kth-th
    // largest key's 16 leading bits (a lower bound, as in compact_query) by two 256-bin histograms in LDS.
    int *s_h = reinterpret_cast<int *>(s_e);  // 256 bins (s_e is written later)
    float thr = -__builtin_inff();
    if (n_all >= p.kth && n_all > p.kth + 8) {  // uniform
        uint32_t prefix = 0;
        int need = p.kth;
#pragma unroll 1
        for (int pass = 0; pass < 2; pass++) {
            s_h[tid] = 0;  // kBlock == 256 bins
            __syncthreads();
            const int sh = pass == 0 ? 24 : 16;
#pragma unroll
            for (int s = 0; s < EPT; s++)
                if (ev[s] && (pass == 0 || (ekey[s] >> 24) == (prefix >> 24))) atomicAdd(&s_h[(ekey[s] >> sh) & 255u], 1);
            __syncthreads();
            if (tid < 64) {  // bins in DESCENDING order: position 4 tid + j is bin 255 - (4 tid + j)
                int c[4], tot = 0;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    c[j] = s_h[255 - (4 * tid + j)];
                    tot += c[j];
                }
                int incl = tot;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const int v = __shfl_up(incl, o, 64);
                    if (tid >= o) incl += v;
                }
                int acc = incl - tot;
                if (acc < need && incl >= need) {  // exactly one lane
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        if (acc < need && acc + c[j] >= need) {
                            s_misc[3] = 255 - (4 * tid + j);
                            s_misc[4] = need - acc;
                        }
                        acc += c[j];
                    }
                }
            }
            __syncthreads();
            prefix |= (uint32_t)s_misc[3] << sh;
            need = s_misc[4];
            __syncthreads();
        }
        thr = fkey_inv(prefix) - mg;
    } else {
        __syncthreads();
    }
    // the survivors' row ids, packed (any order)
#pragma unroll
    for (int s = 0; s < EPT; s++)
        if (ev[s] && fkey_inv(ekey[s]) >= thr) s_i[atomicAdd(&s_misc[5], 1)] = (int)eidx[s];
    __syncthreads();
    const int n = s_misc[5];
    // exact distances, two candidates per 16-lane group and step (their gathers in flight together: the loop is latency-bound)
    for (int c0 = gib; c0 < n; c0 += 2 * kGroupsPerBlock) {
        const int c1 = c0 + kGroupsPerBlock;
        const bool two = c1 < n;
        const int64_t i0 = s_i[c0], i1 = s_i[two ? c1 : c0];
        float *row0 = sx + (size_t)gib * d, *row1 = sx + (size_t)(kGroupsPerBlock + gib) * d;
        gather_row(row0, p.X, p.Xb, i0, d, lane);
        gather_row(row1, p.X, p.Xb, i1, d, lane);
        __builtin_amdgcn_wave_barrier();
        float r[2];
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const float *row = u ? row1 : row0;
            const int64_t i = u ? i1 : i0;
            if (p.metric == GORSE_METRIC_EUCLIDEAN || p.metric == kMetricEuclidBf16) {
                r[u] = euclid_any_lds(p.metric, sq, row, vs, lane);
            } else {
                const float ab = dot512_lds(sq, row, vs, lane);
                if (p.metric == GORSE_METRIC_NEG_DOT)
                    r[u] = -ab;
                else
                    r[u] = cosine_distance(ab, qq, p.norm2[i]);
            }
        }
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) {
            s_e[c0] = r[0];
            if (two) s_e[c1] = r[1];
        }
    }
    __syncthreads();
    // Order the admissible candidates by exact distance: a bitonic sort of (order-preserving key of the distance, index) in
    // LDS -- n = ~240 at C4, where ranking every candidate against every other one was two thirds of this kernel's time.
    // Equal distances are adjacent afterwards; one inside the top k + 1 hands the query to the tie path, so the order
    // among equals never shows.  The query itself, a NaN distance and the padding up to the power of two sort last.
    uint32_t *s_key = reinterpret_cast<uint32_t *>(s_e);
    int P = 2;
    while (P < n) P <<= 1;
    {
        uint32_t kreg[kCapT / kBlock];
        int ireg[kCapT / kBlock];
#pragma unroll
        for (int s = 0; s < kCapT / kBlock; s++) {
            const int c = tid + s * kBlock;
            kreg[s] = 0xffffffffu;
            ireg[s] = -1;
            if (c < n && s_i[c] != self) {
                const float e = s_e[c];
                if (e != e) {
                    s_misc[1] = 1;
                } else {
                    kreg[s] = gorse::rank::dist_key(e);
                    ireg[s] = s_i[c] | (gorse::rank::dist_is_negative_zero(e) ? (int)0x80000000 : 0);  // bit 31: the distance is -0
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < kCapT / kBlock; s++) {
            const int c = tid + s * kBlock;
            if (c < P) {
                s_key[c] = kreg[s];
                s_i[c] = ireg[s];
            }
        }
    }
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int x = tid; x < P / 2; x += kBlock) {
                const int lo = 2 * x - (x & (stride - 1));  // the x-th pair of this step: (lo, lo + stride)
                const int hi = lo + stride;
                const bool up = (lo & size) == 0;
                const uint32_t a = s_key[lo], b = s_key[hi];
                if ((a > b) == up) {
                    s_key[lo] = b;
                    s_key[hi] = a;
                    const int ia = s_i[lo];
                    s_i[lo] = s_i[hi];
                    s_i[hi] = ia;
                }
            }
            __syncthreads();
        }
    }
    int admissible = 0;  // the keys below the sentinel, counted by everyone (a binary search over the sorted keys)
    {
        int lo = 0, hi = P;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s_key[mid] != 0xffffffffu) lo = mid + 1;
            else hi = mid;
        }
        admissible = lo;
    }
    const int top = admissible < k ? admissible : k;
    // ties that reach the top k + 1; the non-positive distances among the top k (prune0: they are the first ones)
    for (int r = tid; r <= k && r < admissible; r += kBlock) {
        const uint32_t a = s_key[r];
        if ((r > 0 && s_key[r - 1] == a) || (r + 1 < admissible && s_key[r + 1] == a)) s_misc[1] = 1;
        if (r < k && p.prune0 && gorse::rank::dist_key_nonpositive(a)) atomicAdd(&s_misc[0], 1);
    }
    __syncthreads();
    if (verify && s_misc[2] < p.kth) {  // the warm start was too high: swept again from -inf with the tie queries
        if (tid == 0) {
            p.cflag[t] = 2;
            atomicAdd(p.sym_stats + 1, 1ull);
        }
        return;
    }
    if (s_misc[1] || top < p.expect) {  // ties, NaN, or a list that cannot hold the answer: path A
        if (tid == 0) p.cflag[t] = 1;
        return;
    }
    const int dropped = s_misc[0];
    for (int r = dropped + tid; r < top; r += kBlock) {
        const uint32_t a = s_key[r];
        const int iv = s_i[r];
        p.out_idx[t * k + r - dropped] = iv & 0x7fffffff;
        p.out_dist[t * k + r - dropped] = gorse::rank::dist_from_key(a, iv < 0);
    }
    const int cnt = top - dropped;
    for (int r = cnt + tid; r < k; r += kBlock) {
        p.out_idx[t * k + r] = -1;
        p.out_dist[t * k + r] = __builtin_inff();
    }
    if (tid == 0) p.out_cnt[t] = cnt;
}

// The flagged queries of a chunk, listed in ascending order by ONE workgroup (a megabyte of flag bytes: two passes of a few
// microseconds): pos[] their positions in the chunk, self[] the stored ids the tie path excludes (-1: a query vector), cnt[0] how
// many, cnt[1] how many of them carry flag 2 (a warm start that could not be verified).  Of a triangle shard only the queries this
// rank owns count.
__global__ __launch_bounds__(1024) void flag_compact_kernel(const uint8_t *__restrict__ cflag, int64_t m, int tri_rank, int tri_world, int bq,
                                                            int64_t q0, const int64_t *__restrict__ qid, int by_vector,
                                                            int32_t *__restrict__ pos, int64_t *__restrict__ self, long long *__restrict__ cnt) {
    __shared__ int part[1024], part2[1024];
    const int tid = threadIdx.x;
    const int64_t per = ((m + 1023) / 1024 + 15) & ~(int64_t)15, a = std::min<int64_t>(m, tid * per), b = std::min<int64_t>(m, a + per);
    auto mine = [&](int64_t t) { return tri_world <= 1 || (int)((t / bq) % tri_world) == tri_rank; };
    // sixteen flags per load (a thread's slice starts on a multiple of 16 and the buffer is 256-byte aligned; one byte per load was
    // 0.85 ms of every C4 pass for a million flags, profiles/r06_zl_timeline_topk_c4.txt), nearly all of them zero
    auto each_set = [&](auto &&f) {
        for (int64_t t0 = a; t0 < b; t0 += 16) {
            if (t0 + 16 <= m) {
                const uint4 w = *reinterpret_cast<const uint4 *>(cflag + t0);
                if (!(w.x | w.y | w.z | w.w)) continue;
            }
            const int64_t t1 = std::min<int64_t>(b, t0 + 16);
            for (int64_t t = t0; t < t1; t++) {
                const uint8_t v = cflag[t];
                if (v && mine(t)) f(t, v);
            }
        }
    };
    int c1 = 0, c2 = 0;
    each_set([&](int64_t, uint8_t v) { c1++, c2 += v == 2; });
    part[tid] = c1;
    part2[tid] = c2;
    __syncthreads();
    if (tid == 0) {
        int run = 0, run2 = 0;
        for (int i = 0; i < 1024; i++) {
            const int v = part[i];
            part[i] = run;
            run += v;
            run2 += part2[i];
        }
        cnt[0] = run;
        cnt[1] = run2;
    }
    __syncthreads();
    int at = part[tid];
    each_set([&](int64_t t, uint8_t) {
        pos[at] = (int32_t)t;
        self[at] = by_vector ? -1 : (qid ? qid[t] : q0 + t);
        at++;
    });
}

}  // namespace

int32_t gorse::rescore_chunk(gorse_topk *h, const ChunkState &cs, int64_t *n_flagged) {
    const int64_t m = cs.m, q0 = cs.q_contig_begin + cs.c0;
    const bool sym = cs.sym;
    RescoreParams rp;
    rp.X = h->X.p;
    rp.Xb = h->dtype == GORSE_DTYPE_BF16 ? h->Xb.p : nullptr;
    rp.norm2 = h->norm2.p;
    rp.Qf = cs.Qf;
    rp.qn2 = cs.qn2;
    rp.qid = cs.qid_host ? h->qid.p : nullptr;
    rp.q0 = q0;
    rp.tri_rank = cs.tri_rank, rp.tri_world = cs.tri_world, rp.tri_bq = kSymBQ;
    rp.own_slices = sym ? cs.sym_slices : 1, rp.own_stride = cs.mb;
    rp.cbuf = h->cbuf.p;
    rp.ccnt = h->ccnt.p;
    rp.cflag = h->cflag.p;
    rp.d = h->d;
    rp.metric = h->kernel_metric();
    rp.k = cs.k;
    rp.prune0 = cs.prune0;
    rp.expect = cs.expect;
    rp.out_idx = h->res_idx.p;
    rp.out_dist = h->res_dist.p;
    rp.out_cnt = h->res_cnt.p;
    rp.fbuf = sym ? h->fbuf.p : nullptr;
    rp.fcnt = sym ? h->fcnt.p : nullptr;
    rp.f0 = sym ? h->f0.p : nullptr;
    rp.ffinal = sym ? h->f1.p : nullptr;
    rp.sym_stats = sym ? h->sym_stats.p : nullptr;
    rp.qmargin = h->qmargin.p;
    rp.kth = cs.kth;
    const size_t lds = rescore_lds_bytes(h->d, kGroupsPerBlock);
    const int tok = h->prof.begin(GORSE_PROF_TOPK_SELECT, h->stream);
    topk_rescore_kernel<<<dim3((unsigned)m), dim3(kBlock), lds, h->stream>>>(rp);
    GORSE_HIP_CHECK(hipGetLastError());
    h->prof.end(tok, h->stream);
    // The queries the sweep + rescoring could not decide (ties in the top k + 1, NaN, overflow; of a triangle shard: among the queries
    // this rank owns -- a foreign query's flag, a staging overflow seen here, has travelled to its owner) are listed ON THE DEVICE,
    // in ascending order, with the stored ids the replay excludes: the host reads two words.  (Rounds 1-5 copied the chunk's flag
    // bytes out and walked them: 0.63 ms between the rescoring and the tie path of a C4 pass, profiles/r06_i_timeline_topk_c4_before.txt.)
    GORSE_TRY(h->fl_pos.ensure((size_t)cs.mb));
    GORSE_TRY(h->fl_self.ensure((size_t)cs.mb));
    GORSE_TRY(h->fl_cnt.ensure(2));
    flag_compact_kernel<<<dim3(1), dim3(1024), 0, h->stream>>>(h->cflag.p, m, cs.tri_rank, cs.tri_world, kSymBQ,
                                                              cs.by_vector ? (int64_t)-1 : q0, cs.qid_host ? h->qid.p : nullptr,
                                                              cs.by_vector ? 1 : 0, h->fl_pos.p, h->fl_self.p, h->fl_cnt.p);
    GORSE_HIP_CHECK(hipGetLastError());
    long long fl[2] = {0, 0};
    GORSE_HIP_CHECK(hipMemcpyAsync(fl, h->fl_cnt.p, sizeof(fl), hipMemcpyDeviceToHost, h->stream));
    GORSE_HIP_CHECK(hipStreamSynchronize(h->stream));
    *n_flagged = fl[0];
    h->n_resweep += fl[1];
    return GORSE_OK;
}
