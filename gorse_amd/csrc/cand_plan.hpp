// cand_plan.hpp -- the host side of the candidate chain (cand.hip) that needs no device: the validation of gorse_cand_begin's rows,
// of a stage against the state of the pass, and of the list stages' inputs.  Every gorse_cand_* call runs these before it launches or
// replaces anything, so an error leaves the chain as it was.  No HIP in here: tests/cpp/cand_plan_main.cpp runs it under
// AddressSanitizer and UBSan without a device.
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>

#include "../../include/gorse_hip.h"

namespace gorse {
namespace cand {

constexpr int64_t kMaxSharedList = 65536;  // gorse_cand_add_shared's n_list at most

inline std::string fmt(const char *f, long long a = 0, long long b = 0, long long c = 0) {
    char buf[256];
    snprintf(buf, sizeof(buf), f, a, b, c);
    return buf;
}

// What a pass has come to: the stage rule bounds a query's candidates by the sum of the stages' k.
struct Pass {
    bool begun = false, finished = false;
    bool replaced = false;  // the finished rows hold the replacement stage's entries (cand_replace_plan.hpp)
    int64_t n_queries = 0;
    int32_t capacity = 0, n_stages = 0;
    int64_t sum_k = 0;
};

// gorse_cand_begin's arguments: the base exclusion rows as a CSR (indptr == NULL: no rows) and the candidate rows' capacity.
inline int32_t validate_begin(int64_t n_queries, const int64_t *indptr, const int32_t *items, int32_t capacity, int64_t n_items,
                              std::string *msg) {
    if (n_queries < 0 || n_queries > INT32_MAX) return *msg = fmt("n_queries = %lld", n_queries), GORSE_ERR_INVALID;
    if (capacity < 1) return *msg = fmt("capacity = %lld < 1", capacity), GORSE_ERR_INVALID;
    if (n_queries > 0 && (int64_t)capacity > (((int64_t)1 << 40) / n_queries))
        return *msg = fmt("n_queries * capacity = %lld * %lld too large", n_queries, capacity), GORSE_ERR_INVALID;
    if (!indptr) return GORSE_OK;
    if (indptr[0] != 0) return *msg = "excl_indptr[0] != 0", GORSE_ERR_INVALID;
    for (int64_t t = 0; t < n_queries; t++) {
        if (indptr[t + 1] < indptr[t]) return *msg = fmt("excl_indptr not monotone at row %lld", t), GORSE_ERR_INVALID;
        if (indptr[t + 1] - indptr[t] > INT32_MAX) return *msg = fmt("exclusion row %lld too long", t), GORSE_ERR_INVALID;
    }
    const int64_t n = indptr[n_queries];
    if (n > 0 && !items) return *msg = "excl_items is NULL", GORSE_ERR_INVALID;
    for (int64_t e = 0; e < n; e++)
        if (items[e] < 0 || items[e] >= n_items)
            return *msg = fmt("excl_items[%lld] = %lld out of range [0,%lld)", e, items[e], n_items), GORSE_ERR_RANGE;
    return GORSE_OK;
}

// A further stage of k entries per query at most against the state of the pass.
inline int32_t validate_stage(const Pass &P, int32_t k, std::string *msg) {
    if (!P.begun) return *msg = "no pass begun (gorse_cand_begin)", GORSE_ERR_INVALID;
    if (P.finished) return *msg = "the pass is finished: gorse_cand_begin starts the next one", GORSE_ERR_INVALID;
    if (k < 1 || k > GORSE_CAND_MAX_K) return *msg = fmt("k = %lld outside 1 .. %lld", k, GORSE_CAND_MAX_K), GORSE_ERR_INVALID;
    if (P.n_stages >= GORSE_CAND_MAX_STAGES) return *msg = fmt("more than %lld stages", GORSE_CAND_MAX_STAGES), GORSE_ERR_INVALID;
    if (P.sum_k + k > P.capacity)
        return *msg = fmt("%lld candidates so far at most, k = %lld more would pass the capacity of %lld", P.sum_k, k, P.capacity),
               GORSE_ERR_INVALID;
    return GORSE_OK;
}

// gorse_cand_add_shared's list
inline int32_t validate_shared(int64_t n_list, const int32_t *items, const double *scores, int64_t n_items, std::string *msg) {
    if (n_list < 0 || n_list > kMaxSharedList) return *msg = fmt("n_list = %lld outside 0 .. %lld", n_list, kMaxSharedList), GORSE_ERR_INVALID;
    if (n_list > 0 && (!items || !scores)) return *msg = "items or scores is NULL", GORSE_ERR_INVALID;
    for (int64_t e = 0; e < n_list; e++)
        if (items[e] < 0 || items[e] >= n_items)
            return *msg = fmt("items[%lld] = %lld out of range [0,%lld)", e, items[e], n_items), GORSE_ERR_RANGE;
    return GORSE_OK;
}

// gorse_cand_add_lists' CSR: one list per query
inline int32_t validate_lists(int64_t n_queries, const int64_t *indptr, const int32_t *items, const double *scores, int64_t n_items,
                              std::string *msg) {
    if (!indptr) return *msg = "indptr is NULL", GORSE_ERR_INVALID;
    if (indptr[0] != 0) return *msg = "indptr[0] != 0", GORSE_ERR_INVALID;
    for (int64_t t = 0; t < n_queries; t++) {
        if (indptr[t + 1] < indptr[t]) return *msg = fmt("indptr not monotone at row %lld", t), GORSE_ERR_INVALID;
        if (indptr[t + 1] - indptr[t] > INT32_MAX) return *msg = fmt("list %lld too long", t), GORSE_ERR_INVALID;
    }
    const int64_t n = indptr[n_queries];
    if (n > 0 && (!items || !scores)) return *msg = "items or scores is NULL", GORSE_ERR_INVALID;
    for (int64_t e = 0; e < n; e++)
        if (items[e] < 0 || items[e] >= n_items)
            return *msg = fmt("items[%lld] = %lld out of range [0,%lld)", e, items[e], n_items), GORSE_ERR_RANGE;
    return GORSE_OK;
}

}  // namespace cand
}  // namespace gorse
