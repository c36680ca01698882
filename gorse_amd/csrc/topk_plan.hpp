// topk_plan.hpp -- the host side of path B of the exact top-k (topk_mfma.hip and the units it drives) that needs no device: the
// capacities of its lists, the launch geometry of the sweep (the kernel and its __launch_bounds__ use the same constexpr functions),
// the operand depth of an index, when a search is warm-started and when it has a symmetric form, the row slices of the history
// sweep and of a triangle shard, the lane replay's queries per wave, the geometry of a triangle-sharded search and the dynamic-LDS
// sizes of the rescoring, sort and lane kernels.  A function that a test switch (GORSE_TEST_TOPK_*, include/gorse_hip_test.h)
// overrides takes the switch bits as an argument.  No HIP in here: tests/cpp/topk_plan_main.cpp runs it under AddressSanitizer and
// UBSan without a device.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/gorse_hip_test.h"

namespace gorse {
namespace topk_plan {

constexpr int kMaxRB = 4;      // a tile holds RB 32-row MFMA blocks (RB = 2 or 4: 64 or 128 candidate rows per barrier)
constexpr int kWavesMain = 8;  // waves per workgroup of the main sweep, two per SIMD
constexpr int kNcbMain = 2;    // 32-query column blocks per wave for operand depths up to 8
constexpr int kSymBQ = 32 * kNcbMain * kWavesMain;  // queries per workgroup (= query block) of the main sweep: the unit of a triangle shard
// the history sweep serves the few queries with ties: small workgroups (2 waves = 64 * NCB queries) spread them over
// many CUs instead of a handful of 8-wave workgroups; deep operands keep more waves (the tile prefetch registers of a
// thread grow as the workgroup shrinks)
// Round 6: at the power-of-two depths that have LDS-DMA tiles the history sweep takes the main sweep's form instead --
// eight waves, 512 queries per workgroup, 64-row DMA tiles: the two-wave workgroups staged their tiles through registers and ran
// the matrix pipe at 0.22 PFLOP/s (C4: 11.7 ms for 10,136 queries against 9.5 ms; profiles/r06_zzk_probe_topk_c4_hist_dma_warm.txt).
// The other depths keep the two-wave form.
constexpr bool sweep_hist_dma(int kp) { return kp == 2 || kp == 4 || kp == 8; }
constexpr int sweep_waves(bool hist, int kp) { return !hist || sweep_hist_dma(kp) ? kWavesMain : (kp <= 8 ? 2 : (kp <= 12 ? 4 : 8)); }
// Tiles reach LDS by LDS-DMA (global_load_lds_dwordx4: 1 KB per wave-instruction, no VGPR round trip, no ds_write pass) when
// the operand depth is a power of two and the sweep is a main sweep: the LDS image of a tile is then lane-linear (unpadded
// rows), and the 16-byte pieces of a row are XOR-swizzled by the row number on the SOURCE address and again on the read, so
// that the 16 lanes of a ds_read_b128 group fall on 16 different slots of the 256-byte bank row.  Other depths (and their
// history sweeps' small workgroups) stage through registers into rows padded by 16 bytes.
constexpr bool sweep_dma(int kp, bool hist, int rb, int wv) {
    return (!hist || sweep_hist_dma(kp)) && (kp & (kp - 1)) == 0 && (32 * rb * kp * 2) % (64 * wv) == 0 && (32 * rb) % 64 == 0;
}
// LDS of a sweep workgroup: NBUF tile buffers (+ their row scales and, without DMA, block bounds), five words per query, the
// tile counters.  DMA: four buffers (tile t is multiplied while t + 1 has landed
// and t + 2 is in flight; the fourth keeps the waves a tile apart); register staging: three where they fit next to the rest
// in 144 KB (the main sweep up to KP = 8 with 128-row tiles), else two; the history sweep keeps two (its small workgroups
// share a CU).
constexpr size_t sweep_row_bytes(int kp, bool dma) { return (size_t)kp * 32 + (dma ? 0 : 16); }
constexpr size_t sweep_tile_bytes(int kp, int rb, bool dma) {
    return (size_t)32 * rb * sweep_row_bytes(kp, dma) + (size_t)32 * rb * 4 + (dma ? 0 : 2 * kMaxRB * 4);
}
constexpr size_t sweep_fixed_bytes(int bq) { return (size_t)5 * bq * 4 + 64; }
// SYM (the symmetric all-pairs sweep, see topk_sweep_kernel): per tile buffer the thresholds of the tile's rows AS QUERIES (their
// value and its raw-score form), per wave a staging area of kStageCap (key, row query | column) entries
constexpr int kStageCap = 128;      // staged foreign candidates per wave
constexpr int kStageFlushAt = 64;   // a wave empties its staging area once it holds this many
constexpr size_t sweep_sym_bytes(int rb, int wv, bool sym) { return sym ? (size_t)2 * 32 * rb * 4 : 0; }  // per tile buffer
constexpr size_t sweep_stage_bytes(int wv, bool sym) { return sym ? (size_t)wv * kStageCap * 8 + 64 : 0; }  // + 4 x kMaxRB block minima
constexpr int sweep_bufs(int kp, int rb, int bq, int wv, bool hist, bool sym = false) {
    if (sweep_dma(kp, hist, rb, wv))
        return 4 * (sweep_tile_bytes(kp, rb, true) + sweep_sym_bytes(rb, wv, sym)) + sweep_fixed_bytes(bq) + sweep_stage_bytes(wv, sym) <= (size_t)156 * 1024 ? 4 : 3;
    return !hist && 3 * sweep_tile_bytes(kp, rb, false) + sweep_fixed_bytes(bq) <= (size_t)144 * 1024 ? 3 : 2;
}
constexpr size_t sweep_lds_bytes(int kp, int rb, int bq, int wv, bool hist, bool sym = false) {
    return sweep_bufs(kp, rb, bq, wv, hist, sym) * (sweep_tile_bytes(kp, rb, sweep_dma(kp, hist, rb, wv)) + sweep_sym_bytes(rb, wv, sym)) +
           sweep_fixed_bytes(bq) + sweep_stage_bytes(wv, sym);
}
// the operand depths (k-steps of 16 bf16 values) the sweep is instantiated for (dispatch_sweep, topk_sweep.hip)
constexpr int kSupportedKP[] = {1, 2, 3, 4, 6, 8, 12, 16, 24};
// the operand depths whose main sweep has a symmetric form: 128-row DMA tiles, two column blocks per wave
constexpr bool sweep_sym_kp(int kp) { return kp == 2 || kp == 4 || kp == 8; }
// 128: one barrier per four MFMA row blocks, 8 % faster than 64 at C4 (profiles/r02_d_probe_topk_warm.txt)
inline int rows_per_tile(int variant) { return (variant & GORSE_TEST_TOPK_TILE64) ? 64 : 128; }
constexpr int kHistTileRows = 64;  // the history sweep keeps the 64-row form (launch_sweep)

constexpr int64_t kMinSweepQueries = 768;  // fewer queries in a call take the scan (see topk_mfma_usable)
constexpr int kCap = 512;      // candidate-list capacity per query
constexpr int kCapF = 512;     // SYM: capacity of a query's FOREIGN list (candidates other workgroups found for it)
constexpr int kCapT = kCap + kCapF;  // candidates the rescoring takes per query: its own list + its foreign list
constexpr int kEPL = kCap / 64;
constexpr int kCompactAt = kCap - 64;   // a list must be compacted once it holds more than this (a block adds <= 32)
// The sweep compacts a list (threshold raised to its K-th best) as soon as one of its two sub-lists holds more than kCompactSubAt:
// 4.7 ms of the C4 pass less than at kCompactAt / 2 = 224 (fewer rows accepted late in the sweep), 96 no better
// (profiles/r03_p_probe_c4_floor.txt)
constexpr int kCompactSubAt = 128;
static_assert(kCompactSubAt <= kCompactAt / 2, "a sub-list holds half of the list");
constexpr int kPilotStride = 16;        // the warm start's pilot sweeps every 16th row tile (chunk_prepare)
constexpr int kOverflowAt = kCap - 128; // a compaction that keeps more than this cannot make progress
constexpr int kMaxKth = 256;
constexpr int kHistCap = 4096;          // history entries per query of the tie-replay sweep (see topk_tie.hip)
constexpr int kReplayCap = 8192;        // power of two >= kCap + kHistCap: entries the replay sorts
static_assert((kReplayCap & (kReplayCap - 1)) == 0 && kReplayCap >= kCap + kHistCap, "the replay sorts a list and its history");
constexpr int64_t kReplayChunk = 16384; // flagged queries per history sweep (history buffers = 512 MB per row slice)
constexpr int kMaxSlices = 8;           // row slices of a history sweep (see topk_tie_sort_kernel)
constexpr int kMaxSlicesFew = 32;       // ... of one that serves few queries (hist_slices)
constexpr int64_t kChunkQ = (int64_t)1 << 20;
constexpr int kMaxOwnSlices = 4;        // row slices per query block of a symmetric main sweep at most (tri_own_slices)
constexpr int kLaneLog = 24;            // lane replay: slots one T can write (<= 9 by its push, <= 9 by its pop)

// The operand depth of an index of d values per row: bf16 rows as they are, fp32 rows as the three leading terms of the split
// product (split_f32_kernel), in the shallowest form the sweep is instantiated for; 0 = too deep for register-resident query
// operands (path A).
inline int operand_depth(bool bf16, int d) {
    const int64_t need = ((bf16 ? d : 3 * (int64_t)d) + 15) / 16;
    for (int c : kSupportedKP)
        if (c >= need) return c;
    return 0;
}

// Warm start.  A streaming threshold that begins at -inf accepts ~kth * ln(N / kth) * (its lag) rows per query (1800
// at C4) and every accepted row costs its 32 x 32 block the slow epilogue.  A pilot sweep over every 16th row tile
// with kth_pilot = j yields the j-th best score of a 1/16 sample: with X ~ Binomial(kth - 1, 1/16) sample members
// among the true kth - 1 best, that score is below the kth best of ALL rows unless X >= j -- j is chosen for a
// tail of ~1e-3 -- and about 16 j rows lie above it.  The main sweep starts there and VERIFIES it (compact_query
// flags a query whose K-th-best bound does not reach its threshold); those few queries join the tie queries' stage.
// (Every 8th and every 32nd tile, and the 1/16 pilot without the 1/256 one in front, were measured at C4 and lost by
// 6 to 28 ms of the 224 ms pass: profiles/r06_a_probe_gpu_probe_topk_c4_pilot.txt.)
// Test switches: WARM_OFF = no warm start, WARM_ALWAYS = warm start whatever N, PILOT_KTH2 = a pilot kth of 2 (thresholds
// far too high: most queries fail the verification and are swept again)
inline bool warm_start(int variant, int kth, int64_t N) {
    return !(variant & GORSE_TEST_TOPK_WARM_OFF) && kth >= 8 && (N >= (int64_t)1 << 17 || (variant & GORSE_TEST_TOPK_WARM_ALWAYS));
}
// the kth of a pilot over 1 / ratio of the rows that proposes the threshold of a sweep with kth = of
inline int pilot_kth(int of, int ratio) {
    const double lam = (double)(of - 1) / ratio;
    return (int)std::ceil(lam + 3.3 * std::sqrt(lam) + 1.5);
}
// two pilots: the 1/16 sample's own sweep would start cold (and a cold start accepts ~1500 rows per query however
// few rows there are: every block of its 1/16 of the tiles would take the slow epilogue), so a 1/256 sample --
// a subset of the 1/16 sample -- proposes ITS thresholds first, by the same rule
inline bool two_pilots(int variant, int64_t N) { return N >= (int64_t)1 << 18 || (variant & GORSE_TEST_TOPK_WARM_ALWAYS); }

// The symmetric form (topk_sweep_kernel, SYM) of the search of the stored rows [q0, q0 + nq) as queries: the range starts on a tile
// boundary, the sweep is warm-started (a foreign workgroup cannot tighten a threshold: it needs a good one from the start), the
// operands have a depth with a symmetric sweep, in 128-row tiles, and there are at least two query blocks.  SYM_OFF switches it
// off (the square sweep: tests, ablation); with REPLAY_COUNTERS the main sweep keeps its square form.
inline bool sym_eligible(int variant, int kp, int kth, int64_t N, int64_t q0, int64_t nq) {
    return warm_start(variant, kth, N) && !(variant & (GORSE_TEST_TOPK_SYM_OFF | GORSE_TEST_TOPK_REPLAY_COUNTERS)) && sweep_sym_kp(kp) &&
           rows_per_tile(variant) == 128 && q0 % 128 == 0 && nq >= 2 * kSymBQ;
}

// Row slices of the history sweep of m2 flagged queries: a history sweep serves few queries (1 % of a chunk), so its workgroups
// are few, and each would walk all N rows on its own -- 56 ms for 10,000 queries at C4, three quarters of the tie path.  Cut into
// slices of rows, slices x as many workgroups each walk 1 / slices of the rows; topk_tie_sort_kernel joins the slices.
// SLICES8: eight slices whatever N (lets small test inputs take the path); SLICE1: one slice.
inline int hist_slices(int variant, int64_t N, int64_t m2) {
    int nsl = (int)std::min<int64_t>(kMaxSlices, std::max<int64_t>(1, N / 32768));
    // Few flagged queries -- a rank of a sharded search holds 1 / world of them, and the history sweep's time does not
    // shrink with their number: every workgroup (128 queries) walks its slice of the rows whatever else runs -- take more,
    // shorter slices until the launch has ~512 workgroups (at most kMaxSlicesFew, slices of at least 16384 rows).  A full
    // single-GPU C4 pass (10,136 queries: 80 x 8 workgroups) keeps its eight: sixteen were measured there, 9.2 + 14.0 ms
    // against 11.4 + 11.4 (every slice starts cold, the join and the replay pay for it).
    // (counted in 128-query units whatever the history workgroup holds -- 512 queries in the eight-wave DMA form of round 6:
    // with that form's true count the rule would take 32 slices at C4's 10,136 queries, measured 228.3 ms per pass against
    // 220.2 with eight, 224.3 with sixteen: profiles/r06_zzl_probe_topk_c4_hist_slices.txt)
    const int64_t wgs = (m2 + 64 * kNcbMain - 1) / (64 * kNcbMain);
    while (nsl >= kMaxSlices && nsl < kMaxSlicesFew && wgs * nsl < 512 && N / (2 * (int64_t)nsl) >= 16384) nsl *= 2;
    if (variant & GORSE_TEST_TOPK_SLICES8) nsl = kMaxSlices;
    if (variant & GORSE_TEST_TOPK_SLICE1) nsl = 1;
    return nsl;
}

// LDS of the lane replay (topk_tie_replay_lane_kernel): per query `slots` heap weights and values, a snapshot of the values, the log
constexpr size_t lane_lds_bytes(int slots, int qpw) { return (size_t)(3 * slots + 2 * kLaneLog) * qpw * 4; }
// Queries per wave of the lane replay of m2 queries with heaps of `slots` = k + 1 slots: 64 where their columns fit in LDS.
// The lanes of a wave replay their queries in step: a wave takes as long as its lanes' branches laid end to end, and
// the launch as long as its slowest wave, however few queries there are (1,250 queries of one rank of eight: 11.9 ms,
// the 10,136 of a whole C4 pass: 11.5).  Fewer queries per wave while the launch has fewer waves than the chip has CUs
// (REPLAY_WAVE64: 64 whatever the size).
inline int replay_queries_per_wave(int variant, int slots, int64_t m2) {
    int qpw = 64;
    while (qpw > 16 && lane_lds_bytes(slots, qpw) > (size_t)144 * 1024) qpw >>= 1;
    while (qpw > 16 && !(variant & GORSE_TEST_TOPK_REPLAY_WAVE64) && (m2 + qpw - 1) / qpw < 256) qpw >>= 1;
    return qpw;
}
// LDS of topk_rescore_kernel (the query, two rows per 16-lane group, kCapT distances and indices, eight words) and of
// topk_tie_sort_kernel (kReplayCap indices and distances, the query, a row per group, four words); groups = 16-lane groups per workgroup
constexpr size_t rescore_lds_bytes(int d, int groups) { return ((size_t)(1 + 2 * groups) * d + 2 * kCapT + 8) * 4; }
constexpr size_t tie_sort_lds_bytes(int d, int groups) { return ((size_t)2 * kReplayCap + (size_t)(1 + groups) * d + 4) * 4; }

// A launch is as long as its longest workgroup, and the longest block of the triangle sweeps every row with its 512 queries on ONE
// CU: 40 ms at C4, whatever the number of ranks (a rank of eight holds 244 workgroups for 256 CUs: its main sweep took those 40 ms
// where its share of the work is 19).  Few, long workgroups are therefore cut by ROWS: slice y of a block takes an even share of
// its tiles, with own lists of its own (slice-major, like a history sweep's: topk_rescore_kernel takes them together); 1, 2 or 4
// slices, the fewest that give the launch ~768 workgroups.  (TRI_SLICES(n) forces 1 / 2 / 4: tests, ablation.)
// blocks = the query blocks this rank sweeps.
inline int tri_own_slices(int variant, int64_t blocks, int world) {
    int S = 1;
    while (S < kMaxOwnSlices && blocks * S < 768) S *= 2;
    const int forced = (variant & GORSE_TEST_TOPK_TRI_SLICES(3)) / GORSE_TEST_TOPK_TRI_SLICES(1);
    if (forced) S = forced == 1 ? 1 : (forced == 2 ? 2 : 4);
    return world > 1 || forced ? S : 1;
}

// The triangle-sharded search of nq queries over `world` ranks: rank r sweeps the query blocks C with C % world == r (and owns
// their queries), and runs the pilots of a contiguous slice of the queries.
struct TriGeom {
    int64_t nq, nblk;
    int world;
    TriGeom(int64_t nq_, int world_) : nq(nq_), nblk((nq_ + kSymBQ - 1) / kSymBQ), world(world_) {}
    int64_t blocks_of(int r) const { return nblk > r ? (nblk - r + world - 1) / world : 0; }
    int64_t owned(int r) const {  // queries rank r owns: whole blocks, but for the globally last one
        const int64_t nb = blocks_of(r);
        if (nb == 0) return 0;
        const int64_t last = r + (nb - 1) * world;  // its last block
        return (nb - 1) * kSymBQ + std::min<int64_t>(kSymBQ, nq - last * kSymBQ);
    }
    void slice(int r, int64_t *lo, int64_t *hi) const {  // the queries whose pilots rank r runs: whole blocks, even split
        *lo = std::min(nq, nblk * r / world * kSymBQ);
        *hi = std::min(nq, nblk * (r + 1) / world * kSymBQ);
    }
};

}  // namespace topk_plan
}  // namespace gorse
