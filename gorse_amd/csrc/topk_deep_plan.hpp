// topk_deep_plan.hpp -- the host rules of the DEEP sweep form of path B of the exact top-k (topk_deep.hip): which indices it serves,
// the padded operand depth, the tile and K-slice sizes, the LDS of a workgroup and the staging groups of the rescoring of deep rows.
// No HIP in here: tests/cpp/topk_deep_plan_main.cpp walks it over every served width under AddressSanitizer and UBSan.
//
// Path B's first form (topk_sweep.hip) keeps a query's whole operand in registers and therefore ends at 24 k-steps
// (topk_plan::operand_depth).  The deep form streams BOTH operands through LDS in K-slices and keeps the score tile in accumulator
// registers instead, so its depth is bounded only by what was chosen to be served:
//   bf16 rows  384 < d <= 4096
//   fp32 rows  128 < d <= 1536   (the three-term bf16 split of split_f32_kernel: the operand is 3 d deep, at most 4608)
// The shape, from the compiler's resource report of topk_deep_sweep_kernel (gfx950: no scratch, no spills):
// four waves, one per SIMD; a tile of 128 rows x 256 queries; a wave owns 64 of the queries and multiplies all 128 rows, i.e. eight
// 32 x 32 blocks = 128 fp32 accumulators per lane, which with fragments and addresses fits the 512 registers a wave has at one wave
// per SIMD.  Fewer queries per wave halve the MFMAs per ds_read (the A fragments are shared by a wave's column blocks); more do not
// fit the register file.  A K-slice is 64 bf16 values (128 bytes, four k-steps): 48 KB for both operands, three slices resident
// (one multiplied, two in flight) = 144 KB of the CU's 160 KB.
#pragma once
#include "topk_plan.hpp"

namespace gorse {
namespace topk_deep_plan {

constexpr int kMaxBf16D = 4096;  // widest bf16 row served
constexpr int kMaxF32D = 1536;   // widest fp32 row served (operand 3 d = 4608)
constexpr int kSlice = 64;       // bf16 values of an operand row per K-slice: four k-steps of v_mfma_f32_32x32x16_bf16
constexpr int kSliceRowBytes = kSlice * 2;
constexpr int kRows = 128;       // candidate rows per tile (four 32-row blocks)
constexpr int kWaves = 4;
constexpr int kQueriesPerWave = 64;  // two 32-query column blocks
constexpr int kQueries = kWaves * kQueriesPerWave;  // per workgroup
constexpr int kThreads = kWaves * 64;
constexpr int kBufs = 3;         // K-slices resident: the one being multiplied and two in flight behind it
constexpr size_t kSliceBytes = (size_t)(kRows + kQueries) * kSliceRowBytes;  // the A rows, then the B rows
// LDS-DMA instructions (64 lanes x 16 bytes) per wave and slice: the wave's share of the A rows, and its own queries' B rows
constexpr int kDmaA = kRows * kSliceRowBytes / 1024 / kWaves;
constexpr int kDmaB = kQueriesPerWave * kSliceRowBytes / 1024;
constexpr int kDmaPerSlice = kDmaA + kDmaB;  // the s_waitcnt vmcnt() immediate that leaves exactly one slice in flight
static_assert(kDmaA * kWaves * 1024 == kRows * kSliceRowBytes && 2 * kDmaPerSlice < 63, "whole DMA instructions; two slices in flight fit vmcnt");
// three slices, the row values of two tiles, four words per query (two sub-list lengths, threshold, margin)
constexpr size_t lds_bytes() { return kBufs * kSliceBytes + (size_t)2 * kRows * 4 + (size_t)4 * kQueries * 4; }
static_assert(lds_bytes() <= (size_t)160 * 1024, "a workgroup of the deep sweep fits the CU's LDS");

// Fewer queries in a call take the scan.  The deep form starts from the register-resident form's threshold; the crossover at deep
// operands has not been measured (scripts/bench_topk_deep.py measures whole passes only).
constexpr int64_t kMinDeepQueries = topk_plan::kMinSweepQueries;

inline int operand_values(bool bf16, int d) { return bf16 ? d : 3 * d; }
// does the deep form serve rows of d values: too deep for the register-resident form, within the served widths
inline bool serves(bool bf16, int d) { return d > 0 && topk_plan::operand_depth(bf16, d) == 0 && d <= (bf16 ? kMaxBf16D : kMaxF32D); }
// bf16 values per operand row: whole K-slices, zero padded; 0 = not served
inline int padded_depth(bool bf16, int d) { return serves(bf16, d) ? (operand_values(bf16, d) + kSlice - 1) / kSlice * kSlice : 0; }
inline int slices(bool bf16, int d) { return padded_depth(bf16, d) / kSlice; }

// topk_rescore_kernel stages the query and two rows per 16-lane group as d floats each: the groups that take part in the exact
// distances of a deep index, the most of 16, 8, 4, 2, 1 whose staging fits 144 KB (16 up to d = 1054, 2 at d = 4096)
inline int rescore_groups(int d) {
    int g = 16;
    while (g > 1 && topk_plan::rescore_lds_bytes(d, g) > (size_t)144 * 1024) g >>= 1;
    return g;
}

}  // namespace topk_deep_plan
}  // namespace gorse
