// fm_rank_order.hpp -- the order gorse_fm_rank_users ranks one user's candidates in, stated once for the host (plain C++, no
// HIP: the stand-alone test program of tests/ compiles this file alone) and once as a sort key for the device.
//   descending score; equal scores (as floats: -0 == +0) by ascending position; NaN scores last, by ascending position.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

namespace gorse {
namespace fm {

// a ranks strictly before b by score alone (a strict weak order: all NaNs are equivalent and rank behind every number)
inline bool rank_before(float a, float b) {
    if (a != a) return false;
    if (b != b) return true;
    return a > b;
}

// The same order as an unsigned key, ascending: numbers descending with -0 folded onto +0, every NaN at 0xffffffff whatever its
// sign and payload (no number maps there: only the bit pattern 0xffffffff, a NaN, would).
#if defined(__HIPCC__)
__host__ __device__
#endif
inline uint32_t rank_key(uint32_t bits) {
    if ((bits & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
    if (bits == 0x80000000u) bits = 0;
    const uint32_t ascending = (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
    return ~ascending;
}

// order[r] = position of the r-th ranked of n scores; ties keep their positions' order (std::stable_sort)
inline void rank_positions(const float *scores, int64_t n, int32_t *order) {
    for (int64_t i = 0; i < n; i++) order[i] = (int32_t)i;
    std::stable_sort(order, order + n, [scores](int32_t a, int32_t b) { return rank_before(scores[a], scores[b]); });
}

}  // namespace fm
}  // namespace gorse
