// cand_replace_plan.hpp -- the host side of the replacement stage (cand_replace.hip) that needs no device: the validation of
// gorse_cand_add_replacement's history rows against the state of the pass and of gorse_fm_rank_cand_decayed's decays, the word a
// history entry travels in, the key the decayed doubles sort by, and the host's statement of the decayed order (the fallback of
// lists longer than the device sort's cap).  No HIP in here: tests/cpp/cand_replace_plan_main.cpp runs it under AddressSanitizer
// and UBSan without a device.
#pragma once
#include <algorithm>
#include <cstring>

#include "cand_plan.hpp"
#include "fm_rank_order.hpp"

namespace gorse {
namespace cand {

// gorse_cand_add_replacement against the pass: finished, and not grown yet
inline int32_t validate_replacement_pass(const Pass &P, std::string *msg) {
    if (!P.begun || !P.finished) return *msg = "no finished pass (gorse_cand_finish)", GORSE_ERR_INVALID;
    if (P.replaced) return *msg = "the pass has its replacement rows already: gorse_cand_begin starts the next one", GORSE_ERR_INVALID;
    return GORSE_OK;
}

// the history rows: a CSR from 0, a kind of 1 or 2 and an item of [0, n_items) per entry
inline int32_t validate_history(int64_t n_queries, const int64_t *indptr, const int32_t *items, const uint8_t *kind, int64_t n_items,
                                std::string *msg) {
    if (!indptr) return *msg = "hist_indptr is NULL", GORSE_ERR_INVALID;
    if (indptr[0] != 0) return *msg = "hist_indptr[0] != 0", GORSE_ERR_INVALID;
    for (int64_t t = 0; t < n_queries; t++) {
        if (indptr[t + 1] < indptr[t]) return *msg = fmt("hist_indptr not monotone at row %lld", t), GORSE_ERR_INVALID;
        if (indptr[t + 1] - indptr[t] > INT32_MAX) return *msg = fmt("history row %lld too long", t), GORSE_ERR_INVALID;
    }
    const int64_t n = indptr[n_queries];
    if (n > 0 && (!items || !kind)) return *msg = "hist_items or hist_kind is NULL", GORSE_ERR_INVALID;
    for (int64_t e = 0; e < n; e++) {
        if (kind[e] != GORSE_CAND_KIND_POSITIVE && kind[e] != GORSE_CAND_KIND_READ)
            return *msg = fmt("hist_kind[%lld] = %lld is neither 1 (positive) nor 2 (read)", e, kind[e]), GORSE_ERR_INVALID;
        if (items[e] < 0 || items[e] >= n_items)
            return *msg = fmt("hist_items[%lld] = %lld out of range [0,%lld)", e, items[e], n_items), GORSE_ERR_RANGE;
    }
    return GORSE_OK;
}

// validate:"gt=0" (config/config.go:403-404): zero, a negative number and NaN are refused
inline int32_t validate_decays(double positive_decay, double read_decay, std::string *msg) {
    if (!(positive_decay > 0.0)) return *msg = "positive_decay must be > 0", GORSE_ERR_INVALID;
    if (!(read_decay > 0.0)) return *msg = "read_decay must be > 0", GORSE_ERR_INVALID;
    return GORSE_OK;
}

// One history entry as the device sorts it: item * 2 + (read ? 1 : 0).  An item is below 2^31, so the word holds it, and
// ascending words are ascending items with an item's positive entry in front of its read ones.
#if defined(__HIPCC__)
__host__ __device__
#endif
inline uint32_t history_word(int32_t item, uint8_t kind) {
    return ((uint32_t)item << 1) | (kind == GORSE_CAND_KIND_READ ? 1u : 0u);
}

// The decayed order as an unsigned key, ascending: numbers descending with -0 folded onto +0, every NaN at the top whatever its
// sign and payload (fm_rank_order.hpp's rank_key, 64 bits wide).
#if defined(__HIPCC__)
__host__ __device__
#endif
inline uint64_t decay_key(uint64_t bits) {
    const uint64_t sign = (uint64_t)1 << 63;
    if ((bits & ~sign) > 0x7ff0000000000000ull) return ~(uint64_t)0;
    if (bits == sign) bits = 0;
    const uint64_t ascending = (bits & sign) ? ~bits : (bits | sign);
    return ~ascending;
}

inline uint64_t double_bits(double x) {
    uint64_t b;
    memcpy(&b, &x, 8);
    return b;
}

// a ranks strictly before b by the decayed score alone
inline bool decayed_before(double a, double b) {
    if (a != a) return false;
    if (b != b) return true;
    return a > b;
}

// order[r] = position of the r-th of n entries: descending final, ties and NaNs in the ranker's order (fm::rank_positions on the
// float scores).  The device's (decay_key, rank_key, position) order, by two stable sorts.
inline void decayed_positions(const float *scores, const double *fin, int64_t n, int32_t *order) {
    fm::rank_positions(scores, n, order);
    std::stable_sort(order, order + n, [fin](int32_t a, int32_t b) { return decayed_before(fin[a], fin[b]); });
}

}  // namespace cand
}  // namespace gorse
