// topk_compact.hpp -- the list compaction the candidate sweeps of path B share (topk_sweep.hip, topk_deep.hip): one wave raises a
// query's filter threshold to (K-th best approximate score so far) - margin and packs what survives.  A query's list has exactly one
// writer, the wave that owns the query.
#pragma once
#include "topk_mfma_internal.hpp"

namespace gorse {

// One wave raises the filter threshold of local query ql and compacts its list.
// HIST: the entries the new threshold drops are appended to the query's history (hb, counter s_hc[ql]) instead of
// being forgotten; list + history then hold every vector the reference's heap can have accepted.
// SYM: the list holds only the rows of the workgroup's OWN part of the sweep (the rest of the query's candidates are in its
// foreign list), so what it proves about the warm start is one-sided: a K-th-best bound that clears the threshold verifies it
// (the own rows are a subset of all rows) and raises it; one that does not proves nothing -- the warm start is then verified over
// both lists by topk_rescore_kernel, which learns from the final threshold (f_out) whether the sweep ever raised it.
template <bool HIST, bool SYM = false>
__device__ __forceinline__ void compact_query(uint2 *qb, int ql, int kth, int *s_cnt, float *s_f, const float *s_mg,
                                              uint8_t *flag, uint2 *hb = nullptr, int *s_hc = nullptr, bool trust = false) {
    const int lane = threadIdx.x & 63;
    // the list is two interleaved sub-lists: even slots belong to the lane holding rows 0-3, 8-11, ... of the query's
    // column (lane < 32), odd slots to its partner (lane >= 32); each appends at its own counter (slot 2 * c + half)
    const int n_lo = s_cnt[2 * ql], n_hi = s_cnt[2 * ql + 1];
    const int n = n_lo + n_hi;
    // The list is re-read by loads the compiler does not see (one asm statement: the wave's appends drained to L2, eight
    // L1-bypassing loads, their wait).  A load hipcc can see inside the tile loop makes its wait-count pass put
    // s_waitcnt vmcnt(0) at the head of every iteration (the load may be pending along the back edge), and that drains the
    // tiles the LDS-DMA has in flight.  All kCap slots are allocated, so the loads need no predicate; slots past the
    // sub-lists' lengths are masked below (key 0 = never counted: trial >= 1).
    static_assert(kEPL == 8, "compact_query loads eight entries per lane");
    unsigned long long ev[kEPL];
    {
        const uint2 *src = qb + lane;
        asm volatile("s_waitcnt vmcnt(0)\n\t"
                     "global_load_dwordx2 %0, %8, off sc1\n\t"
                     "global_load_dwordx2 %1, %8, off offset:512 sc1\n\t"
                     "global_load_dwordx2 %2, %8, off offset:1024 sc1\n\t"
                     "global_load_dwordx2 %3, %8, off offset:1536 sc1\n\t"
                     "global_load_dwordx2 %4, %8, off offset:2048 sc1\n\t"
                     "global_load_dwordx2 %5, %8, off offset:2560 sc1\n\t"
                     "global_load_dwordx2 %6, %8, off offset:3072 sc1\n\t"
                     "global_load_dwordx2 %7, %8, off offset:3584 sc1\n\t"
                     "s_waitcnt vmcnt(0)"
                     : "=&v"(ev[0]), "=&v"(ev[1]), "=&v"(ev[2]), "=&v"(ev[3]), "=&v"(ev[4]), "=&v"(ev[5]), "=&v"(ev[6]), "=&v"(ev[7])
                     : "v"(src)
                     : "memory");
    }
    uint32_t key[kEPL], idx[kEPL];
    bool valid[kEPL];
#pragma unroll
    for (int j = 0; j < kEPL; j++) {
        const int e = j * 64 + lane;
        valid[j] = (e & 1) ? (e >> 1) < n_hi : (e >> 1) < n_lo;
        key[j] = valid[j] ? (uint32_t)ev[j] : 0u;
        idx[j] = (uint32_t)(ev[j] >> 32);
    }
    float newf = -__builtin_inff();
    if (n >= kth) {
        // a lower bound of the K-th largest key: bisection on the 16 leading key bits (sign, exponent, 7 mantissa
        // bits), the rest left at zero.  Any bound <= the true K-th best keeps the exactness argument; the 2^-7
        // relative slack keeps a few more entries and halves the cost of a compaction.
        uint32_t prefix = 0;
        for (int b = 31; b >= 16; --b) {
            const uint32_t trial = prefix | (1u << b);
            int c = 0;
#pragma unroll
            for (int j = 0; j < kEPL; j++) c += __builtin_popcountll(__builtin_amdgcn_ballot_w64(key[j] >= trial));
            if (c >= kth) prefix = trial;
        }
        newf = fkey_inv(prefix) - s_mg[ql];
    }
    // SYM: the own list is a PART of the query's candidates, so its K-th best says nothing against the warm start: a bound
    // below the current threshold (or no bound at all) leaves threshold and list as they are
    if (SYM && newf <= s_f[ql]) {
        newf = s_f[ql];
        // nothing will be dropped: the next attempt waits for 64 more entries (s_hc, unused without HIST, holds the list length that
        // allows it) instead of following every append
        if (lane == 0) s_hc[ql] = n + 64;
    }
    // trust (a history slice started from tie_warm_kernel's bound): the starting threshold is a proven lower bound of the K-th best
    // score of the rows in front of the slice -- the slice's own rows need not prove it again, and it never falls
    if (trust && newf < s_f[ql]) newf = s_f[ql];
    if (newf < s_f[ql]) {
        // Only a warm-started threshold can be above what the list proves (thresholds derived from the list never fall):
        // the K-th best of everything above it is not known to clear it by the margin, so rows may have been dropped
        // wrongly.  The query is swept again from -inf by the host (flag 2).
        if (lane == 0) {
            s_f[ql] = __builtin_inff();
            s_cnt[2 * ql] = 0;  // the list is dropped: nothing of it triggers another compaction
            s_cnt[2 * ql + 1] = 0;
            *flag = 2;
        }
        return;
    }
    int base = 0;
    int hbase = HIST ? s_hc[ql] : 0;
    bool hist_full = false;
#pragma unroll
    for (int j = 0; j < kEPL; j++) {
        const bool keep = valid[j] && (fkey_inv(key[j]) >= newf);
        const uint64_t m = __builtin_amdgcn_ballot_w64(keep);
        if (keep) qb[base + lane_rank(m)] = make_uint2(key[j], idx[j]);  // survivors packed into slots 0 .. base-1
        base += __builtin_popcountll(m);
        if (HIST) {
            const uint64_t md = __builtin_amdgcn_ballot_w64(valid[j] && !keep);
            const int nd = __builtin_popcountll(md);
            if (hbase + nd > kHistCap)
                hist_full = true;
            else if (valid[j] && !keep)
                hb[hbase + lane_rank(md)] = make_uint2(key[j], idx[j]);
            if (!hist_full) hbase += nd;
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (lane == 0) {
        s_cnt[2 * ql] = (base + 1) >> 1;  // slots 0 .. base-1 read as the two interleaved sub-lists again
        s_cnt[2 * ql + 1] = base >> 1;
        s_f[ql] = newf;
        if (HIST) s_hc[ql] = hbase;
        if (base > kOverflowAt || hist_full) {  // ties / a margin too wide for the list: stop collecting, path A decides
            s_f[ql] = __builtin_inff();
            *flag = 1;
        }
    }
}

}  // namespace gorse
