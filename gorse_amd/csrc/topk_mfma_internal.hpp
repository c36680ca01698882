// topk_mfma_internal.hpp -- what the units of path B of the exact top-k share: the parameter blocks of its kernels, the state of a
// chunk, the small device helpers more than one unit needs and the host entry points that cross units.  One unit per stage:
//   topk_sweep.hip    the bf16 MFMA candidate sweep (main, pilot, history and symmetric forms) and its dispatch
//   topk_rescore.hip  exact rescoring and ranking of the candidate lists, the list of the queries that leaves undecided
//   topk_tie.hip      the tie path of one chunk of undecided queries: history sweep, sort, lane-heap replay
//   topk_mfma.hip     operands, error bound and the chunk driver (topk_mfma_prepare / _search)
//   topk_tri.hip      the triangle-sharded all-pairs search (gorse_topk_tri_*)
// The rules the host decides by live in topk_plan.hpp, which has no HIP in it.
#pragma once
#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "rank_keys.hpp"
#include "topk_internal.hpp"
#include "topk_plan.hpp"
#include "topk_sym.hpp"

namespace gorse {
using namespace topk_plan;
static_assert(kGroupsPerBlock * kGroup == kBlock && kCapT % kBlock == 0, "topk_rescore_kernel holds kCapT / kBlock candidates per thread");

using gorse::rank::fkey;      // order-preserving float -> uint of an approximate score, and back (rank_keys.hpp)
using gorse::rank::fkey_inv;
__device__ __forceinline__ int lane_rank(uint64_t m) {  // set bits of m below this lane
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
}

struct SweepParams {
    const uint16_t *A;     // candidate operands, N x KPAD bf16
    const uint16_t *B;     // query operands, nq x KPAD bf16
    const float *rscale;   // per-row value of the epilogue (cosine scale, Euclidean bias, 1 for -dot; NaN: row not admissible)
    const float *qmargin;  // per-query 2*delta_q
    uint2 *cbuf;           // nq x kCap (key, index)
    int32_t *ccnt;         // nq
    uint8_t *cflag;        // nq: 1 = this path cannot decide the query
    uint2 *hbuf;           // HIST sweeps: nq x kHistCap entries a compaction dropped, in arrival order
    int32_t *hcnt;         // HIST sweeps: nq
    int64_t N, nq;
    int kth;
    int compact_at;        // a sub-list longer than this triggers the compaction of its query: kCompactSubAt
    int ep;                // EP_SCALE / EP_BIAS / EP_COARSE: what the epilogue does with the per-row values (host side: picks the kernel)
    unsigned long long *prof;  // host side only: the handle's counters when GORSE_TEST_TOPK_REPLAY_COUNTERS asks the tie replay to count (ReplayParams::prof);
                               // the main sweep then keeps its square form.  No sweep reads it.
    // warm start (see topk_mfma_search): a PILOT sweep walks every tile_stride-th tile with kth = a small j and writes the
    // threshold it ends with to f_out; the main sweep starts from f0 and verifies it (compact_query: a threshold that a later
    // K-th-best bound does not reach flags the query 2 = "sweep again from -inf")
    const float *f0;   // nq initial thresholds or null (-inf)
    float *f_out;      // pilot: nq final thresholds; null otherwise
    int tile_stride;   // 1, or the pilot's sampling stride over the row tiles
    int nslices;       // HIST: row slices (grid.y); the per-query outputs are then nslices x nq long, slice-major
    const float *fwarm;  // HIST: nslices x nq starting thresholds of the slices (tie_warm_kernel: each a valid lower bound of the K-th
                         // best score among the rows IN FRONT of the slice, so nothing the reference's heap can have accepted is
                         // missed; -inf = cold), or null: every slice starts cold.  Trusted: a compaction never flags them.
    float rs_min, rs_max;  // smallest and largest row value of the index (EP_COARSE bound of the DMA sweeps)
    // SYM sweeps (the queries are the stored rows sym_q0 .. sym_q0 + nq): see topk_sweep_kernel
    int64_t sym_q0;        // row of query 0, a multiple of the tile height
    const float *frow;     // nq thresholds of the rows as queries (the pilot's: frozen for the foreign workgroups)
    const float *frow_raw; // RAWF: their raw-score form (raw_threshold of frow)
    uint2 *fbuf;           // nq x kCapF foreign lists
    int32_t *fcnt;         // nq entries appended to them (may exceed kCapF: the list then overflowed)
    unsigned long long *sym_stats;  // [0] queries without a pilot threshold, [1] warm starts the rescoring could not verify, [2] foreign
                                    // lists that overflowed, [3] (query, block) hits beyond a wave's staging area
    // SYM, triangle sharding over GPUs (gorse_topk_tri_*): this launch sweeps the query blocks C with C % sym_world == sym_rank only --
    // their own lists, and what they find for the rows of EVERY earlier block (foreign lists of queries other ranks own included);
    // 0 of 1 = the whole triangle
    int sym_rank, sym_world;
    int sym_slices;  // SYM: row slices per query block (grid.y; 1 = the whole block's tiles in one workgroup)
};

// What the epilogue does with a block's 32 x 32 raw scores before it compares them with the thresholds:
constexpr int EP_NONE = 0;    // nothing (-dot without a mask; register-staged sweeps only)
constexpr int EP_SCALE = 1;   // every score times its row's value (cosine with unequal norms; masked rows: NaN)
constexpr int EP_BIAS = 2;    // every score plus its row's value (Euclidean: -|x|^2 / 2)
constexpr int EP_COARSE = 3;  // the block's LARGEST raw score times the extreme row value bounds every scaled score of the block
                              // (values positive and nearly equal, or all 1): the rows are scaled only when that bound reaches a threshold

// A stored vector into the LDS row of a 16-lane group: from the bf16 rows as given when the index is bf16 (half the bytes,
// the same fp32 values once widened), else from the fp32 rows.
__device__ __forceinline__ void gather_row(float *row, const float *X, const uint16_t *Xb, int64_t i, int d, int lane) {
    if (Xb && (d & 7) == 0) {  // 16-byte pieces
        const uint4 *src = reinterpret_cast<const uint4 *>(Xb + i * d);
        for (int e = lane; e < d / 8; e += kGroup) {
            const uint4 v = src[e];
            float4 *dst = reinterpret_cast<float4 *>(row + 8 * e);
            dst[0] = make_float4(__uint_as_float(v.x << 16), __uint_as_float(v.x & 0xffff0000u), __uint_as_float(v.y << 16),
                                 __uint_as_float(v.y & 0xffff0000u));
            dst[1] = make_float4(__uint_as_float(v.z << 16), __uint_as_float(v.z & 0xffff0000u), __uint_as_float(v.w << 16),
                                 __uint_as_float(v.w & 0xffff0000u));
        }
    } else if (Xb) {
        for (int e = lane; e < d; e += kGroup) row[e] = __uint_as_float((uint32_t)Xb[i * d + e] << 16);
    } else {
        for (int e = lane; e < d; e += kGroup) row[e] = X[i * d + e];
    }
}

// ---- exact rescoring + ranking of one query's candidate list (topk_rescore.hip)
struct RescoreParams {
    const float *X;        // N x d fp32 stored vectors
    const uint16_t *Xb;    // the same vectors as given in bf16 (a bf16 index), or null: the rows are gathered from here -- half
                           // the bytes, the same fp32 values once widened
    const float *norm2;    // N
    const float *Qf;       // nq x d fp32 query vectors, or null (queries are stored vectors)
    const float *qn2;      // nq query norms (cosine)
    const int64_t *qid;    // stored-vector id per query, or null
    int64_t q0;            // used when qid == null and Qf == null: id = q0 + t
    const uint2 *cbuf;
    const int32_t *ccnt;
    uint8_t *cflag;
    int d, metric, k, prune0;
    int64_t expect;        // min(k, number of admissible vectors)
    int32_t *out_idx;
    float *out_dist;
    int32_t *out_cnt;
    // SYM sweeps: the query's foreign list, and what the verification of its warm start needs (see below)
    const uint2 *fbuf;     // nq x kCapF, or null
    const int32_t *fcnt;
    const float *f0;       // the thresholds the main sweep started from
    const float *ffinal;   // the thresholds its workgroups ended with (above f0: raised, hence verified, by the own list)
    unsigned long long *sym_stats;  // (SweepParams)
    const float *qmargin;
    int kth;
    int tri_rank, tri_world, tri_bq;  // triangle sharding: only the queries of the blocks this rank owns (t / tri_bq % tri_world == tri_rank)
    int own_slices;                   // SYM sweeps cut into row slices: own lists / counters / flags / final thresholds per slice ...
    int64_t own_stride;               // ... own_stride queries apart (slice-major)
};

// ---- tie replay (topk_tie.hip, whose head says what the replay is and why list + history suffice for it)
struct ReplayParams {
    const float *X;
    const uint16_t *Xb;    // bf16 index: the rows as given (see RescoreParams), else null
    const float *norm2;
    const float *Qf;       // by-vector queries: fp32 rows of the chunk (row pos[t]), or null
    const float *qn2;      // query norms of the chunk (row pos[t]), cosine only
    const int64_t *self;   // stored-vector id of the query, or -1 for by-vector queries
    const int32_t *pos;    // row of the query in the chunk's result arrays
    const uint2 *cbuf;
    const int32_t *ccnt;
    const uint2 *hbuf;
    const int32_t *hcnt;
    const float *fslice;   // nslices x nq: the threshold every slice of the history sweep ended with (-inf: none)
    int nslices;           // cbuf / ccnt / hbuf / hcnt / cflag / fslice hold nslices x nq entries, slice-major
    unsigned long long *prof;  // GORSE_TEST_TOPK_REPLAY_COUNTERS: the replay's counters, see gorse_hip_test_get_sweep_profile; else null
    int64_t nq;
    uint8_t *cflag;        // in: flags of the history sweep (non-zero: undecidable); out [0, nq): 2 = undecided here
    int64_t N;
    int d, metric, k, prune0;
    int32_t *out_idx;
    float *out_dist;
    int32_t *out_cnt;
    int32_t *sidx;         // per query kReplayCap recorded vector ids, ascending (stage 1 -> stage 2)
    float *sdst;           // their exact distances
    int32_t *scount;       // how many, or -1 when a distance is NaN
};

// the history slices' starting thresholds (tie_warm_kernel, topk_tie.hip)
struct WarmParams {
    const int32_t *pos;  // row of the flagged query in the chunk's arrays
    int64_t m2, N;
    int nsl, tile_rows, kth;
    const uint2 *cbuf;  // the main sweep's own lists (own_slices of them per query, own_stride queries apart) ...
    const int32_t *ccnt;
    int own_slices;
    int64_t own_stride;
    const uint2 *fbuf;  // ... and foreign lists (or null)
    const int32_t *fcnt;
    const float *margin;  // m2: the flagged queries' 2 delta (gather_pos_kernel)
    float *fwarm;         // nsl x m2, slice-major
};

// What the stages of one chunk of a search share.  topk_mfma_search runs them back to back; the triangle-sharded search
// (gorse_topk_tri_*) keeps the state in the handle between its calls: the pilots over THIS rank's slice of the queries, then -- once
// every rank's thresholds have arrived -- the main sweep over this rank's query blocks, then -- once the foreign lists have been
// exchanged -- rescoring and tie path for the queries this rank owns.
struct TopkChunkState {
    int64_t nq = 0, m = 0, c0 = 0, q_contig_begin = -1, mb = 0;
    const int64_t *qid_host = nullptr;
    const float *qv_dev = nullptr;
    bool by_vector = false, contiguous = false, euclid = false, warm = false, sym = false;
    int k = 0, kth = 0, prune0 = 0;
    int64_t expect = 0;
    float other = 0.0f;
    const uint16_t *Bop = nullptr;
    const float *qn2 = nullptr, *Qf = nullptr;
    SweepParams sp;
    int tri_rank = 0, tri_world = 1;
    int sym_slices = 1;  // row slices per query block of the symmetric main sweep (a triangle shard with few, long workgroups)
    int tri_stage = 0;  // gorse_topk_tri_*: 0 none, 1 begun (pilots of the own slice done), 2 swept, 3 finished
    int64_t tri_lo = 0, tri_hi = 0;  // the slice of the queries whose pilots this rank ran
};
using ChunkState = TopkChunkState;

// topk_sweep.hip: the sweep of h's operand depth -- hist: a history sweep (p.nslices row slices); sym: the symmetric form
int32_t dispatch_sweep(gorse_topk *h, const SweepParams &p, bool hist, bool sym = false);
// topk_rescore.hip: exact rescoring and ranking of the chunk's lists; the queries that leaves undecided are listed on the device
// (h->fl_pos, h->fl_self), *n_flagged of them
int32_t rescore_chunk(gorse_topk *h, const ChunkState &cs, int64_t *n_flagged);
// topk_tie.hip: the tie path for the flagged queries [f0, f0 + m2) of that list (m2 <= kReplayChunk); flags[r] != 0: still undecided
int32_t tie_replay_chunk(gorse_topk *h, const ChunkState &cs, int64_t f0, int64_t m2, std::vector<uint8_t> &flags);
// topk_mfma.hip: the stages of a chunk (topk_mfma_search runs them back to back, gorse_topk_tri_* call by call)
int32_t search_setup(gorse_topk *h, ChunkState &cs, const int64_t *qid_host, int64_t q_contig_begin, const float *qv_dev, int64_t nq,
                     int k, int prune0);
int32_t chunk_prepare(gorse_topk *h, ChunkState &cs);
int32_t chunk_pilots(gorse_topk *h, ChunkState &cs, int64_t lo, int64_t hi);
int32_t chunk_main(gorse_topk *h, ChunkState &cs);
int32_t chunk_finish(gorse_topk *h, ChunkState &cs);

}  // namespace gorse

