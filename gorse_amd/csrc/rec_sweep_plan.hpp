// rec_sweep_plan.hpp -- the size and launch rules of gorse_mf_recommend's pilot-threshold schedule (recommend_sweep.hip), stated once:
// the sample stride, the sample's bound inside LDS, the survivor lists' capacity, the item slices of the two matrix launches and the
// queries of one launch round.  No HIP in here: tests/cpp/rec_sweep_plan_main.cpp runs it under AddressSanitizer and UBSan.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace gorse {
namespace recsweep {

constexpr int kTile = 32;           // items of a matrix tile; a sample row is padded to whole tiles
constexpr int kQueries = 128;       // queries of a matrix workgroup
constexpr int kBlockThreads = 256;
constexpr int kMaxK = 256;
constexpr int kLdsBytes = 160 * 1024;          // of a gfx950 workgroup
constexpr int kMaxSample = 32768;              // sampled scores of one query: 128 KB of keys, selected in LDS
constexpr int kBaseStride = 16;                // every 16th item is sampled (profiles/recommend_sweep_bench.json: 8 / 16 / 32 on C3)
constexpr int kMaxCap = 12288;                 // survivor entries of one query at most: 96 KB in the finish kernel's LDS
constexpr int kMaxSlices = 16;
constexpr size_t kScratchBytes = (size_t)512 << 20;  // sample scores and survivor lists of one launch round

constexpr bool serves(int d, int k) { return d % 16 == 0 && d >= 16 && d <= 256 && k >= 1 && k <= kMaxK; }

struct Plan {
    int32_t kk = 0;             // k + 1: the threshold is the kk-th best sampled candidate
    int32_t stride = 0;         // items 0, stride, 2 stride, ... are sampled
    int32_t n_sample = 0;       // ceil(I / stride)
    int32_t samp_ld = 0;        // n_sample padded to whole tiles: floats of a query's sample row
    int32_t cap = 0;            // entries of a query's survivor list
    int32_t pilot_slices = 0, sweep_slices = 0;  // grid.y of the two matrix launches: the sampled / all items in equal runs of whole tiles
    int32_t pilot_slice_len = 0, sweep_slice_len = 0;
    int64_t chunk = 0;          // queries of one launch round, a multiple of kQueries unless it is the whole call
    size_t per_query_bytes = 0; // sample row, survivor list (items | scores), threshold, count, flag
    size_t select_lds = 0, finish_lds = 0;
};

constexpr int64_t ceil_div64(int64_t a, int64_t b) { return (a + b - 1) / b; }

// slices of n items for `blocks` query blocks: doubled while the grid is short of 512 workgroups and a slice keeps 256 items
inline void slice(int64_t n, int64_t blocks, int32_t *slices, int32_t *len) {
    int s = 1;
    while (s < kMaxSlices && blocks * s < 512 && n / (s * 2) >= 256) s *= 2;
    const int64_t l = ceil_div64(ceil_div64(n, s), kTile) * kTile;  // whole tiles: a slice starts on a tile edge
    *len = (int32_t)l;
    *slices = (int32_t)std::max<int64_t>(1, ceil_div64(n, l));
}

// stride_hint > 0 replaces kBaseStride (the tuning runs); the rules below still bound it.  I >= 1, 1 <= k <= kMaxK, n_users >= 1.
inline Plan make_plan(int64_t I, int32_t k, int64_t n_users, int32_t stride_hint) {
    Plan p;
    p.kk = k + 1;
    int64_t s = stride_hint > 0 ? stride_hint : kBaseStride;
    while (s > 1 && ceil_div64(I, s) < (int64_t)4 * p.kk) s /= 2;  // a sample of at least 4 kk items where the catalogue has them
    s = std::max<int64_t>(s, ceil_div64(I, kMaxSample));            // and of at most kMaxSample: it is selected in LDS
    p.stride = (int32_t)s;
    p.n_sample = (int32_t)ceil_div64(I, s);
    p.samp_ld = (int32_t)(ceil_div64(p.n_sample, kTile) * kTile);
    // The survivors of a query are the items at or above the kk-th best of a 1-in-stride sample: kk * stride expected, with a
    // standard deviation of about stride * sqrt(kk).  Twice the mean and eight strides on top; excluded items among them come extra.
    p.cap = (int32_t)std::min<int64_t>(kMaxCap, (int64_t)2 * p.kk * s + 8 * s);
    p.per_query_bytes = (size_t)p.samp_ld * 4 + (size_t)p.cap * 8 + 12;
    int64_t chunk = (int64_t)(kScratchBytes / p.per_query_bytes) / kQueries * kQueries;
    p.chunk = std::min<int64_t>(std::max<int64_t>(chunk, kQueries), n_users);
    const int64_t blocks = ceil_div64(p.chunk, kQueries);
    slice(p.n_sample, blocks, &p.pilot_slices, &p.pilot_slice_len);
    slice(I, blocks, &p.sweep_slices, &p.sweep_slice_len);
    p.select_lds = ((size_t)p.n_sample + 256) * 4;                 // keys | histogram
    p.finish_lds = ((size_t)2 * p.cap + (size_t)2 * p.kk) * 4;     // survivors kept (scores | items) | the kk best (scores | items)
    return p;
}

// the sampled scores as unsigned keys, ascending with the score; 0 is kept for "no candidate" and kKeyNaN for a NaN candidate
constexpr uint32_t kKeyNaN = 0xffffffffu;
#if defined(__HIPCC__)
__host__ __device__
#endif
inline uint32_t score_key(uint32_t bits) {
    return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}
#if defined(__HIPCC__)
__host__ __device__
#endif
inline uint32_t key_score_bits(uint32_t key) {
    return (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key;
}

}  // namespace recsweep
}  // namespace gorse
