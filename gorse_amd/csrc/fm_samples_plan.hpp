// fm_samples_plan.hpp -- the host side of training from (user, item) samples that needs no device: the row a sample stands for
// (BatchPredict's order, fm.go:183-206: user lead | item lead | user rest | item rest, zero values skipped -- what ComposedRows
// walks on the device) and the per-batch plan of the gradient accumulation: for every batch the features it touches (ascending)
// and, per feature, its entries as (batch-local row, value) by ascending row and within a row by position -- the order
// build_plan (fm.hip) gives the same rows when they are materialised and padded.  No HIP in here:
// tests/cpp/fm_samples_plan_main.cpp runs it under AddressSanitizer and UBSan without a device.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace gorse {
namespace fm {

// the feature rows of one side as a CSR; lead[i] = the row's leading entries (NULL: none)
struct SideRows {
    const int64_t *ptr;
    const int32_t *idx;
    const float *val;
    const int32_t *lead;
};

// fn(feature, value) for every nonzero entry of the row composed for user u and catalogue row c, in the row's order
template <class F>
inline void compose_row(const SideRows &U, int32_t u, const SideRows &I, int32_t c, F &&fn) {
    const int64_t u0 = U.ptr[u], u1 = U.ptr[u + 1], um = u0 + (U.lead ? U.lead[u] : 0);
    const int64_t i0 = I.ptr[c], i1 = I.ptr[c + 1], im = i0 + (I.lead ? I.lead[c] : 0);
    auto span = [&](const SideRows &S, int64_t j0, int64_t j1) {
        for (int64_t j = j0; j < j1; j++)
            if (S.val[j] != 0.0f) fn(S.idx[j], S.val[j]);
    };
    span(U, u0, um);
    span(I, i0, im);
    span(U, um, u1);
    span(I, im, i1);
}

// the longest composed row's nonzero entries: the width the materialised rows need at least
inline int64_t composed_width(const SideRows &U, const SideRows &I, const int32_t *user, const int32_t *item, int64_t n) {
    int64_t w = 0;
    for (int64_t i = 0; i < n; i++) {
        int64_t c = 0;
        compose_row(U, user[i], I, item[i], [&](int32_t, float) { c++; });
        w = std::max(w, c);
    }
    return w;
}

struct SamplePlan {
    std::vector<int32_t> uniq;        // batch k's features, ascending: slots [uoff[k], uoff[k + 1])
    std::vector<int32_t> seg;         // batch k's slots + 1 batch-local entry offsets, from seg[uoff[k] + k]
    std::vector<int32_t> row;         // per entry the batch-local row; batch k's entries [eoff[k], eoff[k + 1])
    std::vector<float> val;           // per entry the value
    std::vector<int64_t> uoff, eoff;  // n_batches + 1 each
    int64_t max_slots = 0;
};

struct SerialBatches {
    template <class F>
    void operator()(int64_t nb, F fn) const { fn((int64_t)0, nb); }
};

// The plan of samples [0, n) in batches of bs rows (the last one partial).  run(nb, fn) has fn(k0, k1) work on the batches
// [k0, k1), on as many threads as it likes.  false: a batch holds more than 2^31 - 1 nonzero entries.
template <class Run = SerialBatches>
inline bool plan_samples(const SideRows &U, const SideRows &I, const int32_t *user, const int32_t *item, int64_t n, int32_t bs,
                         SamplePlan &out, Run run = Run()) {
    struct Batch {
        std::vector<int32_t> uniq, seg, row;
        std::vector<float> val;
        bool ok = true;
    };
    const int64_t nb = n > 0 ? (n + bs - 1) / bs : 0;
    std::vector<Batch> parts((size_t)nb);
    run(nb, [&](int64_t k0, int64_t k1) {
        std::vector<uint64_t> keys;  // feature << 32 | the entry's number in the batch: rows ascending, positions ascending
        std::vector<int32_t> erow;
        std::vector<float> eval;
        for (int64_t k = k0; k < k1; k++) {
            Batch &B = parts[(size_t)k];
            const int64_t r0 = k * bs, r1 = std::min<int64_t>(n, r0 + bs);
            keys.clear(), erow.clear(), eval.clear();
            for (int64_t r = r0; r < r1 && B.ok; r++)
                compose_row(U, user[r], I, item[r], [&](int32_t f, float x) {
                    if (keys.size() >= (size_t)INT32_MAX) {
                        B.ok = false;
                        return;
                    }
                    keys.push_back(((uint64_t)(uint32_t)f << 32) | (uint64_t)keys.size());
                    erow.push_back((int32_t)(r - r0));
                    eval.push_back(x);
                });
            if (!B.ok) continue;
            std::sort(keys.begin(), keys.end());
            B.row.reserve(keys.size()), B.val.reserve(keys.size());
            for (size_t q = 0; q < keys.size(); q++) {
                const int32_t f = (int32_t)(keys[q] >> 32);
                if (q == 0 || (int32_t)(keys[q - 1] >> 32) != f) {
                    B.uniq.push_back(f);
                    B.seg.push_back((int32_t)q);
                }
                const size_t e = (size_t)(keys[q] & 0xffffffffu);
                B.row.push_back(erow[e]);
                B.val.push_back(eval[e]);
            }
            B.seg.push_back((int32_t)keys.size());
        }
    });
    out = SamplePlan();
    out.uoff.assign((size_t)nb + 1, 0);
    out.eoff.assign((size_t)nb + 1, 0);
    for (int64_t k = 0; k < nb; k++) {
        const Batch &B = parts[(size_t)k];
        if (!B.ok) return false;
        out.uoff[(size_t)k + 1] = out.uoff[(size_t)k] + (int64_t)B.uniq.size();
        out.eoff[(size_t)k + 1] = out.eoff[(size_t)k] + (int64_t)B.row.size();
        out.max_slots = std::max<int64_t>(out.max_slots, (int64_t)B.uniq.size());
    }
    out.uniq.reserve((size_t)out.uoff[(size_t)nb]);
    out.seg.reserve((size_t)(out.uoff[(size_t)nb] + nb));
    out.row.reserve((size_t)out.eoff[(size_t)nb]);
    out.val.reserve((size_t)out.eoff[(size_t)nb]);
    for (int64_t k = 0; k < nb; k++) {
        Batch &B = parts[(size_t)k];
        out.uniq.insert(out.uniq.end(), B.uniq.begin(), B.uniq.end());
        out.seg.insert(out.seg.end(), B.seg.begin(), B.seg.end());
        out.row.insert(out.row.end(), B.row.begin(), B.row.end());
        out.val.insert(out.val.end(), B.val.begin(), B.val.end());
        B = Batch();
    }
    return true;
}

}  // namespace fm
}  // namespace gorse
