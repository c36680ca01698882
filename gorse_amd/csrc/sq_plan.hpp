// sq_plan.hpp -- the size and launch rules of the scalar-quantised index (sq.hip), stated once: the padded code row, which path a
// call takes, the sweep's tile rows for a code row, the pilot's stride, the survivor lists' capacity, the row slices of the two
// matrix launches and the queries of one launch round.  Plain C++, no HIP: the host compiles it as it stands.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace gorse {
namespace sq {

constexpr int kMaxD = 4096;          // |t| <= 4096 * 127 * 127 < 2^31
constexpr int kMaxK = 1024;
constexpr int kKStep = 32;           // codes of one v_mfma_i32_32x32x32_i8 step; a code row is padded to whole steps with zeros
constexpr int kQueries = 128;        // queries of a sweep workgroup: 32 per wave, stationary as B fragments
constexpr int kBlockThreads = 256;
constexpr int kSweepMaxD = 1024;     // 4 VGPRs of query codes per step: 128 at 32 steps
constexpr int kSweepMaxK = 256;
constexpr int kBaseStride = 16;      // every 16th stored row is sampled ...
constexpr int kMaxSample = 32768;    // ... unless that is more than the 128 KB of keys the threshold is selected from in LDS
constexpr int kMaxCap = 16384;       // survivor keys of one query: 128 KB sorted in LDS
constexpr int kScanBuf = 2048;       // keys of the scan's running selection
constexpr int kTargetBlocks = 512;   // sweep workgroups wanted before the rows stop being sliced
constexpr int kMaxSlices = 1024;
constexpr int kPadRow = 16;          // bytes between two code rows of an LDS tile: row starts fall on every 16-byte bank group
constexpr size_t kSampleBytes = (size_t)256 << 20;  // sampled scores of one launch round
constexpr int64_t kPlanSweepQueries = 256, kPlanSweepRows = 4096;  // below either the scan answers the call

enum Path { kScan = 1, kSweep = 2 };

constexpr int64_t ceil_div64(int64_t a, int64_t b) { return (a + b - 1) / b; }

// K steps the sweep is compiled for; a code row is padded to the next of them
constexpr int kSteps[] = {1, 2, 3, 4, 6, 8, 12, 16, 24, 32};
constexpr int steps_for(int d) {
    const int need = (d + kKStep - 1) / kKStep;
    for (int s : kSteps)
        if (s >= need) return s;
    return need;  // d > kSweepMaxD: the scan only, whole steps
}
constexpr int padded_d(int d) { return steps_for(d) * kKStep; }
// rows of an LDS tile: 1024 / steps (eight 16-byte loads per thread), a power of two in 32 .. 256: two tiles stay below 80 KB
constexpr int tile_rows(int steps) { return steps <= 4 ? 256 : steps <= 8 ? 128 : steps <= 16 ? 64 : 32; }
constexpr size_t sweep_lds(int steps) {
    return (size_t)2 * tile_rows(steps) * (steps * kKStep + kPadRow) + (size_t)2 * tile_rows(steps) * 3 * 4;  // codes | row constants
}

constexpr bool sweep_serves(int64_t N, int d, int k, int kk) {
    return d <= kSweepMaxD && k <= kSweepMaxK && ceil_div64(N, std::max<int64_t>(kBaseStride, ceil_div64(N, kMaxSample))) >= kk;
}
// forced: 0 = by plan, 1 = scan only, 2 = sweep wherever it serves
constexpr Path choose(int forced, int64_t nq, int64_t N, int d, int k, int kk) {
    if (forced == 1 || !sweep_serves(N, d, k, kk)) return kScan;
    if (forced == 2) return kSweep;
    return nq >= kPlanSweepQueries && N >= kPlanSweepRows ? kSweep : kScan;
}

struct Plan {
    int32_t steps = 0, tile = 0;
    int32_t stride = 0, n_sample = 0, samp_ld = 0;  // rows 0, stride, 2 stride, ...; a sample row padded to 256 floats
    int32_t cap = 0;                                // keys of a query's survivor list
    int32_t pilot_slices = 0, pilot_slice_len = 0, sweep_slices = 0, sweep_slice_len = 0;
    int64_t chunk = 0;                              // queries of one launch round: whole workgroups
    size_t select_lds = 0, pilot_lds = 0;
};

// n rows in runs of whole tiles, enough runs for kTargetBlocks workgroups where the rows have them
inline void slice(int64_t n, int tile, int64_t qblocks, int32_t *slices, int32_t *len) {
    const int64_t tiles = std::max<int64_t>(1, ceil_div64(n, tile));
    const int64_t want = std::min<int64_t>(std::min<int64_t>(kMaxSlices, tiles), std::max<int64_t>(1, ceil_div64(kTargetBlocks, qblocks)));
    const int64_t per = ceil_div64(tiles, want);
    *len = (int32_t)(per * tile);
    *slices = (int32_t)ceil_div64(tiles, per);
}

constexpr int64_t pow2_ceil(int64_t n) {
    int64_t p = 1;
    while (p < n) p *= 2;
    return p;
}

// cap_hint > 0 replaces the list capacity (the test hook).  sweep_serves(N, d, k, kk) holds.
inline Plan make_plan(int64_t N, int d, int kk, int64_t nq, int32_t cap_hint) {
    Plan p;
    p.steps = steps_for(d);
    p.tile = tile_rows(p.steps);
    p.stride = (int32_t)std::max<int64_t>(kBaseStride, ceil_div64(N, kMaxSample));
    p.n_sample = (int32_t)ceil_div64(N, p.stride);
    p.samp_ld = (int32_t)(ceil_div64(p.n_sample, 256) * 256);
    // the survivors of a query are the rows at or above the kk-th best of a 1-in-stride sample: kk * stride expected
    p.cap = cap_hint > 0 ? std::min<int32_t>(cap_hint, kMaxCap) : (int32_t)std::min<int64_t>(kMaxCap, (int64_t)2 * kk * p.stride + 1024);
    const int64_t fit = (int64_t)(kSampleBytes / ((size_t)p.samp_ld * 4)) / kQueries * kQueries;
    p.chunk = std::min<int64_t>(std::max<int64_t>(fit, kQueries), ceil_div64(nq, kQueries) * kQueries);
    const int64_t qblocks = p.chunk / kQueries;
    slice(p.n_sample, p.tile, qblocks, &p.pilot_slices, &p.pilot_slice_len);
    slice(N, p.tile, qblocks, &p.sweep_slices, &p.sweep_slice_len);
    p.pilot_lds = ((size_t)p.n_sample + 256) * 4;      // keys | histogram
    p.select_lds = (size_t)pow2_ceil(p.cap) * 8;
    return p;
}

}  // namespace sq
}  // namespace gorse
