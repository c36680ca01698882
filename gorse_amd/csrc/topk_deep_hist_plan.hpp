// topk_deep_hist_plan.hpp -- the host rules of the tie path of a DEEP handle (gorse_topk_set_deep_tie_replay): the shape of the deep
// history sweep (topk_deep_hist.hip) and the staging groups of topk_tie_sort_kernel for wide rows.  No HIP in here:
// tests/cpp/topk_deep_hist_plan_main.cpp walks it over every served width under AddressSanitizer and UBSan.
//
// The history sweep of a deep handle is the deep sweep's K-loop (topk_deep_body.hpp: 128-row tiles, K-slices of 64 bf16 values by
// LDS-DMA, three slices resident, one barrier per slice) under the shallow history sweep's contract (topk_sweep_kernel<..., HIST>:
// row slices in grid.y, slice-major outputs, warm slice thresholds, a history of what a compaction drops).  It differs from the main
// deep sweep in ONE figure: a workgroup takes 128 queries, not 256.  A replay chunk holds hundreds to a few thousand queries, and
// every workgroup walks its row slice whatever else runs; 128 is the query block topk_plan::hist_slices counts in (64 * kNcbMain),
// so its slice rule applies as it stands, and the call has twice the workgroups of a 256-query form at the same slice count.  A wave
// then owns ONE 32-query column block and all four 32-row blocks: 64 accumulators per lane, five ds_read_b128 per four MFMAs.
#pragma once
#include "topk_deep_plan.hpp"

namespace gorse {
namespace topk_deep_hist_plan {
using namespace topk_deep_plan;

constexpr int kHistQueriesPerWave = 32;  // one 32-query column block
constexpr int kHistQueries = kWaves * kHistQueriesPerWave;  // per workgroup
static_assert(kHistQueries == 64 * topk_plan::kNcbMain, "the query block topk_plan::hist_slices counts workgroups in");
constexpr size_t kHistSliceBytes = (size_t)(kRows + kHistQueries) * kSliceRowBytes;  // the A rows, then the B rows: 32 KB
// LDS-DMA instructions per wave and slice: the wave's share of the A rows (kDmaA, as the main form) and its own queries' B rows
constexpr int kHistDmaB = kHistQueriesPerWave * kSliceRowBytes / 1024;
constexpr int kHistDmaPerSlice = kDmaA + kHistDmaB;  // the s_waitcnt vmcnt() immediate that leaves exactly one slice in flight
static_assert(kHistDmaB * 1024 == kHistQueriesPerWave * kSliceRowBytes && kHistDmaPerSlice == 8 && 2 * kHistDmaPerSlice + 1 < 63,
              "whole DMA instructions; two slices in flight and a tile's row values fit vmcnt");
// three slices, the row values of two tiles, five words per query (two sub-list lengths, threshold, margin, history length)
constexpr size_t hist_lds_bytes() { return kBufs * kHistSliceBytes + (size_t)2 * kRows * 4 + (size_t)5 * kHistQueries * 4; }
static_assert(kHistSliceBytes == 32768 && hist_lds_bytes() <= (size_t)160 * 1024, "a workgroup of the deep history sweep fits the CU's LDS");
constexpr int kDeepHistTileRows = kRows;  // what tie_warm_kernel computes the slices' first rows with (WarmParams::tile_rows)

// topk_tie_sort_kernel stages the query and one row per 16-lane group as d floats each beside 2 x kReplayCap words: the groups that
// take part in the exact distances of a deep index, the most of 16, 8, 4, 2, 1 whose launch fits the CU's 160 KB (16 up to
// d = 1445, 4 at d = 4096).  Handles that are not deep keep all 16.
inline int tie_sort_groups(int d) {
    int g = 16;
    while (g > 1 && topk_plan::tie_sort_lds_bytes(d, g) > (size_t)160 * 1024) g >>= 1;
    return g;
}

}  // namespace topk_deep_hist_plan
}  // namespace gorse
