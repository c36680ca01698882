// fm_eval_plan.hpp -- the host side of scoring resident rows that needs no device: the order gorse_fm_set_test keeps the test
// rows in (EvaluateClassification's, evaluator.go:46-63: positives first, then the others, each side in dataset order) and the
// slice and round planner of gorse_fm_evaluate (segments: the two sides) and gorse_fm_rank_users (segments: the users'
// candidate lists).  No HIP in here: tests/cpp/fm_eval_plan_main.cpp runs it under AddressSanitizer and UBSan without a device.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace gorse {
namespace fm {

// order[r] = the dataset row resident row r holds; rows [0, n_pos) are the positives (target > 0), the rest the negatives
// (a target of exactly 0, and one that is NaN, is a negative: `target > 0` is what the reference asks)
inline int64_t eval_partition(const float *target, int64_t n, std::vector<int32_t> &order) {
    order.resize((size_t)n);
    int64_t n_pos = 0;
    for (int64_t i = 0; i < n; i++)
        if (target[i] > 0) order[(size_t)n_pos++] = (int32_t)i;
    int64_t at = n_pos;
    for (int64_t i = 0; i < n; i++)
        if (!(target[i] > 0)) order[(size_t)at++] = (int32_t)i;
    return n_pos;
}

// element offset of a row in an n x D table: 64 bits, n x D may pass 2^31
inline int64_t eval_emb_offset(int64_t row, int32_t D) { return row * (int64_t)D; }

// The slices and launch rounds of rows that are scored from resident data.  The rows lie in segments (seg_ptr, n_segs + 1
// entries from 0, non-decreasing: the positives and the negatives of a test split, or every user's candidates); an empty segment
// and an empty whole are legal.
struct SlicePlan {
    std::vector<int32_t> desc;         // segment | item | slice's first row inside its round | slice length, n entries each
    std::vector<int64_t> round_begin;  // first row of every launch round, then n
    int64_t n_slices = 0, max_round = 0;
    int64_t rounds() const { return (int64_t)round_begin.size() - 1; }
};

constexpr int64_t kRoundBytes = (int64_t)256 << 20;  // scratch of one launch round at most (unless one slice alone needs more)

// rows of a launch round: as many as kRoundBytes hold at the maxD + 2 d + 2 floats of scratch a row needs (s; vx and h; the
// Softmax's maximum and sum), or what a test hook asks for; never less than a slice
inline int64_t round_rows_for(int maxD, int d, int32_t batch_size, int64_t hook) {
    const int64_t row_floats = (int64_t)maxD + 2 * d + 2;
    return std::max<int64_t>(batch_size, hook > 0 ? hook : kRoundBytes / (row_floats * (int64_t)sizeof(float)));
}

// BatchInternalPredict's slices (fm.go:168-176): batch_size rows from a segment's first row, the segment's last one partial, and
// afresh in the next segment; a launch round holds whole slices of at most round_rows rows in all (raised to batch_size: a
// slice is never split).  item[r] is what row r's embedding row is looked up by; NULL = the row's own number.
inline void plan_slices(const int64_t *seg_ptr, int64_t n_segs, const int32_t *item, int32_t batch_size, int64_t round_rows,
                        SlicePlan &out) {
    const int64_t n = seg_ptr[n_segs];
    const int64_t R = std::max<int64_t>(round_rows, batch_size);
    out.desc.assign((size_t)n * 4, 0);
    out.round_begin.assign(1, 0);
    out.n_slices = out.max_round = 0;
    int32_t *seg = out.desc.data(), *it = seg + n, *row0 = it + n, *len = row0 + n;
    for (int64_t s = 0; s < n_segs; s++)
        for (int64_t s0 = seg_ptr[s]; s0 < seg_ptr[s + 1]; s0 += batch_size) {
            const int64_t sn = std::min<int64_t>(batch_size, seg_ptr[s + 1] - s0);
            if (s0 + sn - out.round_begin.back() > R) out.round_begin.push_back(s0);
            const int64_t local0 = s0 - out.round_begin.back();
            for (int64_t r = s0; r < s0 + sn; r++) {
                seg[r] = (int32_t)s;
                it[r] = item ? item[r] : (int32_t)r;
                row0[r] = (int32_t)local0;
                len[r] = (int32_t)sn;
            }
            out.n_slices++;
        }
    if (n > 0) out.round_begin.push_back(n);
    for (int64_t k = 0; k < out.rounds(); k++)
        out.max_round = std::max(out.max_round, out.round_begin[(size_t)k + 1] - out.round_begin[(size_t)k]);
}

}  // namespace fm
}  // namespace gorse
