// nbr_plan.hpp -- the host side of gorse_nbr_recommend that needs no device: validation of a neighbour table and of a call's
// arguments, the per-row and per-query bounds on the accumulator's entries, and the launch plan that sorts the queries into
// LDS-table classes and the global-table path and cuts each into launches; the validation of gorse_nbr_set_table_from_topk /
// _from_sparse's arguments.  No HIP in here: tests/cpp/nbr_plan_main.cpp and tests/cpp/nbr_build_main.cpp run it under
// AddressSanitizer and UBSan without a device.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/gorse_hip.h"

namespace gorse {
namespace nbr {

constexpr int32_t kWaveSlots = 512;    // an LDS table of at most this many slots is walked by ONE wave (a 64-thread workgroup)
constexpr int32_t kMidSlots = 4096;    // the middle class: a 256-thread workgroup, two tables per CU
constexpr int32_t kMaxLdsSlots = 13056;  // the largest LDS table: 12 bytes per slot beside 6208 bytes of staging in 160 KiB
constexpr int64_t kScratchSlots = (int64_t)1 << 25;  // slots of global tables per launch at most (384 MiB), one query at least

inline std::string fmt(const char *f, long long a = 0, long long b = 0, long long c = 0) {
    char buf[256];
    snprintf(buf, sizeof(buf), f, a, b, c);
    return buf;
}

// A table as gorse_nbr_set_table takes it.  max_index = the largest index of the table (-1 when it has no entry).
inline int32_t validate_table(int32_t which, int64_t n_rows, const int64_t *indptr, const int32_t *indices, const float *weights,
                              int32_t transform, double scale, int64_t n_items, int64_t *max_index, std::string *msg) {
    if (which != GORSE_NBR_HOP1 && which != GORSE_NBR_HOP2) return *msg = fmt("which = %lld is neither hop", which), GORSE_ERR_INVALID;
    if (n_rows < 0 || n_rows > INT32_MAX) return *msg = fmt("n_rows = %lld", n_rows), GORSE_ERR_INVALID;
    if (!indptr) return *msg = "indptr is NULL", GORSE_ERR_INVALID;
    if (indptr[0] != 0) return *msg = "indptr[0] != 0", GORSE_ERR_INVALID;
    for (int64_t r = 0; r < n_rows; r++) {
        if (indptr[r + 1] < indptr[r]) return *msg = fmt("indptr not monotone at row %lld", r), GORSE_ERR_INVALID;
        if (indptr[r + 1] - indptr[r] > INT32_MAX) return *msg = fmt("row %lld has more than 2^31 - 1 entries", r), GORSE_ERR_INVALID;
    }
    const int64_t nnz = indptr[n_rows];
    if (nnz > 0 && !indices) return *msg = "indices is NULL", GORSE_ERR_INVALID;
    if (weights) {
        if (transform != GORSE_NBR_RAW && transform != GORSE_NBR_RECIP) return *msg = fmt("transform = %lld", transform), GORSE_ERR_INVALID;
        if (!std::isfinite(scale)) return *msg = "scale is not finite", GORSE_ERR_INVALID;
        for (int64_t e = 0; e < nnz; e++)
            if (!std::isfinite(weights[e])) return *msg = fmt("weights[%lld] is not finite", e), GORSE_ERR_INVALID;
    }
    int64_t mx = -1;
    const int64_t hi = which == GORSE_NBR_HOP2 ? n_items : (int64_t)INT32_MAX;  // hop 1 is held against hop 2's rows at the call
    for (int64_t e = 0; e < nnz; e++) {
        if (indices[e] < 0 || indices[e] >= hi)
            return *msg = fmt("indices[%lld] = %lld out of range [0,%lld)", e, indices[e], hi), GORSE_ERR_RANGE;
        mx = std::max<int64_t>(mx, indices[e]);
    }
    if (which == GORSE_NBR_HOP2 && weights) {  // one addend per item and list: the kernel's order argument rests on it
        std::vector<int32_t> row;
        for (int64_t r = 0; r < n_rows; r++) {
            row.assign(indices + indptr[r], indices + indptr[r + 1]);
            std::sort(row.begin(), row.end());
            if (std::adjacent_find(row.begin(), row.end()) != row.end())
                return *msg = fmt("weighted hop-2 row %lld repeats an index", r), GORSE_ERR_INVALID;
        }
    }
    if (max_index) *max_index = mx;
    return GORSE_OK;
}

// The arguments of gorse_nbr_set_table_from_topk / _from_sparse against the index's rows (index_n) and the handle's n_items.
// The valid sources, in row order, go to `rows` (the table row) and `src` (the stored row searched): a source < 0 is an empty row.
inline int32_t validate_from_search(int32_t which, int64_t n_rows, const int64_t *sources, int32_t n, int32_t transform, double scale,
                                    int64_t index_n, int64_t n_items, std::vector<int64_t> *rows, std::vector<int64_t> *src,
                                    std::string *msg) {
    if (which != GORSE_NBR_HOP1 && which != GORSE_NBR_HOP2) return *msg = fmt("which = %lld is neither hop", which), GORSE_ERR_INVALID;
    if (n_rows < 0 || n_rows > INT32_MAX) return *msg = fmt("n_rows = %lld", n_rows), GORSE_ERR_INVALID;
    if (n < 1 || n > GORSE_NBR_MAX_LIST) return *msg = fmt("n = %lld outside 1 .. %lld", n, GORSE_NBR_MAX_LIST), GORSE_ERR_INVALID;
    if (!std::isfinite(scale)) return *msg = "scale is not finite", GORSE_ERR_INVALID;
    if (transform != GORSE_NBR_RAW && transform != GORSE_NBR_RECIP) return *msg = fmt("transform = %lld", transform), GORSE_ERR_INVALID;
    if (which == GORSE_NBR_HOP2 && index_n > n_items)
        return *msg = fmt("the index has %lld rows, the handle %lld items", index_n, n_items), GORSE_ERR_RANGE;
    if (!sources && n_rows > index_n) return *msg = fmt("sources is NULL and n_rows %lld > %lld index rows", n_rows, index_n), GORSE_ERR_RANGE;
    rows->clear(), src->clear();
    for (int64_t r = 0; r < n_rows; r++) {
        const int64_t s = sources ? sources[r] : r;
        if (s >= index_n) return *msg = fmt("sources[%lld] = %lld beyond the index's %lld rows", r, s, index_n), GORSE_ERR_RANGE;
        if (s < 0) continue;
        rows->push_back(r);
        src->push_back(s);
    }
    return GORSE_OK;
}

// src_sum[r] = the entries a walk from hop-1 row r meets: the sum of the hop-2 row lengths over the row's entries
inline void row_bounds(int64_t n_rows1, const int64_t *ptr1, const int32_t *idx1, const int64_t *ptr2, std::vector<int64_t> *src_sum) {
    src_sum->assign((size_t)n_rows1, 0);
    for (int64_t r = 0; r < n_rows1; r++) {
        int64_t s = 0;
        for (int64_t p = ptr1[r]; p < ptr1[r + 1]; p++) s += ptr2[idx1[p] + 1] - ptr2[idx1[p]];
        (*src_sum)[(size_t)r] = s;
    }
}

// The arguments of gorse_nbr_recommend against the tables' sizes.
inline int32_t validate_call(int64_t n_queries, const int32_t *rows, int32_t k, const int64_t *seen_indptr, const int32_t *seen_items,
                             int64_t n_rows1, int64_t n_items, std::string *msg) {
    if (k < 1 || k > GORSE_NBR_MAX_K) return *msg = fmt("k = %lld outside 1 .. %lld", k, GORSE_NBR_MAX_K), GORSE_ERR_INVALID;
    if (n_queries < 0 || n_queries > INT32_MAX) return *msg = fmt("n_queries = %lld", n_queries), GORSE_ERR_INVALID;
    if (!rows && n_queries > n_rows1)
        return *msg = fmt("rows is NULL and n_queries %lld > %lld hop-1 rows", n_queries, n_rows1), GORSE_ERR_RANGE;
    if (rows)
        for (int64_t t = 0; t < n_queries; t++)
            if (rows[t] >= n_rows1) return *msg = fmt("rows[%lld] = %lld beyond the %lld hop-1 rows", t, rows[t], n_rows1), GORSE_ERR_RANGE;
    if (seen_indptr && n_queries > 0) {
        if (seen_indptr[0] < 0) return *msg = "seen_indptr[0] < 0", GORSE_ERR_INVALID;
        for (int64_t t = 0; t < n_queries; t++) {
            if (seen_indptr[t + 1] < seen_indptr[t]) return *msg = fmt("seen_indptr not monotone at row %lld", t), GORSE_ERR_INVALID;
            if (seen_indptr[t + 1] - seen_indptr[t] > INT32_MAX) return *msg = fmt("seen row %lld too long", t), GORSE_ERR_INVALID;
        }
        if (seen_indptr[n_queries] > seen_indptr[0] && !seen_items) return *msg = "seen_items is NULL", GORSE_ERR_INVALID;
        for (int64_t e = seen_indptr[0]; e < seen_indptr[n_queries]; e++)
            if (seen_items[e] < 0 || seen_items[e] >= n_items)
                return *msg = fmt("seen_items[%lld] = %lld out of range [0,%lld)", e, seen_items[e], n_items), GORSE_ERR_RANGE;
    }
    return GORSE_OK;
}

// the keys a query's table can come to hold: every item it reaches, and its seen row's blocked keys
inline int64_t query_bound(int64_t n_items, int64_t src_sum, int64_t seen_len) { return std::min(n_items, src_sum) + seen_len; }

struct Launch {
    int64_t q0, q1;   // positions [q0, q1) of Plan::order
    int32_t slots;    // LDS path: the table's slots; 0 = global path (Plan::cap / Plan::off per position)
    int32_t threads;  // 64 = one wave per query (no barrier stands between two lists), 256 = a workgroup with a barrier between lists
};
struct Plan {
    std::vector<int32_t> order;  // the queries, grouped by class, in ascending order inside a class
    std::vector<int32_t> cap;    // per position: the table's slots
    std::vector<int64_t> off;    // per position: the table's first slot in the launch's global scratch (0 on the LDS path)
    std::vector<Launch> launches;
    int64_t n_lds = 0, n_global = 0;
};

// A table must keep one slot empty, so a query fits a table of `slots` slots when bound + 1 <= slots.  lds_slots = the LDS
// capacity in force, query_chunk > 0 = queries per launch at most, scratch_slots = the global tables' budget per launch.
// A global table takes half as many slots again as the bound, so that probe chains stay short.  Returns false when a query's table
// exceeds 2^31 - 1 slots.
inline bool make_plan(int64_t n_queries, const int64_t *bound, int32_t lds_slots, int64_t query_chunk, int64_t scratch_slots, Plan *P) {
    *P = Plan();
    lds_slots = std::max<int32_t>(2, std::min(lds_slots, kMaxLdsSlots));
    const int32_t cls_slots[3] = {std::min(kWaveSlots, lds_slots), std::min(kMidSlots, lds_slots), lds_slots};
    std::vector<int32_t> members[4];
    for (int64_t t = 0; t < n_queries; t++) {
        int c = 0;
        while (c < 3 && bound[t] + 1 > cls_slots[c]) c++;
        members[c].push_back((int32_t)t);
    }
    for (int c = 0; c < 4; c++) {
        const std::vector<int32_t> &m = members[c];
        const int64_t n = (int64_t)m.size();
        (c < 3 ? P->n_lds : P->n_global) += n;
        int64_t a = 0;
        while (a < n) {
            Launch L;
            L.q0 = (int64_t)P->order.size();
            L.slots = c < 3 ? cls_slots[c] : 0;
            L.threads = (c < 3 && cls_slots[c] <= kWaveSlots) ? 64 : 256;
            int64_t b = a, used = 0;
            while (b < n && (query_chunk <= 0 || b - a < query_chunk)) {
                int64_t slots = cls_slots[std::min(c, 2)];
                if (c == 3) {
                    const int64_t bd = bound[m[(size_t)b]];
                    slots = bd + 1 + bd / 2;
                    if (slots > INT32_MAX) return false;
                    if (b > a && used + slots > scratch_slots) break;
                }
                P->order.push_back(m[(size_t)b]);
                P->cap.push_back((int32_t)slots);
                P->off.push_back(c == 3 ? used : 0);
                if (c == 3) used += slots;
                b++;
            }
            L.q1 = (int64_t)P->order.size();
            P->launches.push_back(L);
            a = b;
        }
    }
    return true;
}

}  // namespace nbr
}  // namespace gorse
