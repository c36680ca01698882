// fm_eval_plan.hpp -- the host side of gorse_fm_set_test / gorse_fm_evaluate that needs no device: the order the test rows are
// kept in (EvaluateClassification's, evaluator.go:46-63: positives first, then the others, each side in dataset order) and the
// slice descriptors of the scoring launches (BatchInternalPredict's slices, fm.go:168-176, each side sliced on its own).  No HIP
// in here: tests/cpp/fm_eval_plan_main.cpp runs it under AddressSanitizer and UBSan without a device.
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

struct EvalSlices {
    std::vector<int32_t> desc;         // row | slice's first row inside its round | slice length, n entries each
    std::vector<int64_t> round_begin;  // first row of every launch round, then n
    int64_t n_slices = 0, max_round = 0;
    int64_t rounds() const { return (int64_t)round_begin.size() - 1; }
};

// Slices of batch_size rows from the first positive, the positives' last one partial, and afresh from the first negative; a
// launch round holds whole slices of at most round_rows rows in all (raised to batch_size: a slice is never split).
inline void eval_slices(int64_t n_pos, int64_t n_neg, int32_t batch_size, int64_t round_rows, EvalSlices &out) {
    const int64_t n = n_pos + n_neg;
    const int64_t R = std::max<int64_t>(round_rows, batch_size);
    out.desc.assign((size_t)n * 3, 0);
    out.round_begin.assign(1, 0);
    out.n_slices = out.max_round = 0;
    int32_t *row = out.desc.data(), *row0 = row + n, *len = row0 + n;
    const int64_t side[3] = {0, n_pos, n};
    for (int s = 0; s < 2; s++)
        for (int64_t s0 = side[s]; s0 < side[s + 1]; s0 += batch_size) {
            const int64_t sn = std::min<int64_t>(batch_size, side[s + 1] - s0);
            if (s0 + sn - out.round_begin.back() > R) out.round_begin.push_back(s0);
            const int64_t local0 = s0 - out.round_begin.back();
            for (int64_t r = s0; r < s0 + sn; r++) {
                row[r] = (int32_t)r;
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
