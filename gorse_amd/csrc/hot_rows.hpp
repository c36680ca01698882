// hot_rows.hpp -- which items of a BPR handle are HOT, and how many replica rows each one gets (csrc/bpr.hip, HotRows), shared by
// gorse_mf_create and by the CPU test of the rule (host library hook gh_test_bpr_hot_layout, tests/test_bpr_hot_layout_cpu.py).
// Pure host C++ apart from the three constexpr helpers the kernels decode a slot's word with.  Reference semantics of the rates: a
// sample draws its user uniformly among the users with feedback, then a positive uniformly from that user's row, then a negative
// uniformly from the catalogue (model/cf/model.go:452-468).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace gorse {

// A hot item's word (hot_slot[item] and hot_meta[slot]): its first replica row << 4 | log2 of its replica count.  Every other class
// of hot_slot is negative (-1 warm, -2 cold), so `word >= 0` still means "hot".
constexpr int32_t hot_code(int64_t base, int lg) { return (int32_t)((base << 4) | lg); }
constexpr int64_t hot_base(int32_t code) { return (int64_t)(code >> 4); }
constexpr int hot_lg(int32_t code) { return code & 15; }

// the hot SET: share of the training feedback >= 1/8192 and >= 64 feedbacks, at most 1024 items and a quarter of the catalogue
// (the most frequent ones, ties to the lower id); item ids ascending
inline std::vector<int32_t> hot_items_select(const std::vector<int64_t> &cnt, int64_t nnz) {
    const int64_t I = (int64_t)cnt.size();
    // 1/2048 until round 3: with the negatives routed through the replicas too, 1/8192 is 6 % faster at C2
    // (profiles/r03_zx_probe_bpr_hot.txt).  A replica's content reaches Q one folder pass late, so the hot items stay a
    // minority: at least 64 feedbacks, at most a quarter of the items (S-ml100k with two thirds of its items hot lost
    // 0.011 of NDCG@10 in the per-sample schedule; with every item hot S-ml1m's fit diverges)
    const int64_t hdiv = 8192;
    const size_t hcap = (size_t)std::min<int64_t>(1024, std::max<int64_t>(1, I / 4));
    const int64_t thr = std::max<int64_t>(64, (nnz + hdiv - 1) / hdiv);
    std::vector<int32_t> hot;
    for (int64_t i = 0; i < I; i++)
        if (cnt[(size_t)i] >= thr) hot.push_back((int32_t)i);
    if (hot.size() > hcap) {
        std::nth_element(hot.begin(), hot.begin() + hcap, hot.end(),
                         [&](int32_t a, int32_t b) { return cnt[(size_t)a] != cnt[(size_t)b] ? cnt[(size_t)a] > cnt[(size_t)b] : a < b; });
        hot.resize(hcap);
        std::sort(hot.begin(), hot.end());
    }
    return hot;
}

// whether the user-run schedule sends the NEGATIVE's update of a hot item through the replicas too: only where a draw has a fair
// chance of meeting a hot item (C2: a quarter of the items are hot; at the 10M x 1M set one in ten thousand, and the look-up of the
// negative's class cost 4 % of the epoch)
inline bool hot_neg_replicas(int64_t n_hot, int64_t I) { return n_hot * 64 >= I; }

// The positive draws' share of rows [r0, r1) for every hot slot, in units of 2^-32 / (users with feedback): a sample takes user u with
// probability 1 / U' and then each entry of u's row with probability 1 / len_u.  Fixed point, so that the sum is the same in every
// order (gorse_mf_create adds up the rows in parallel).  slot_of: I entries, >= 0 = the item's slot.
inline void hot_shares_rows(const int64_t *uptr, const int32_t *uidx, const int32_t *slot_of, int64_t r0, int64_t r1, uint64_t *acc) {
    for (int64_t u = r0; u < r1; u++) {
        const int64_t len = uptr[u + 1] - uptr[u];
        if (len <= 0) continue;
        const uint64_t w = ((uint64_t)1 << 32) / (uint64_t)len;
        for (int64_t t = uptr[u]; t < uptr[u + 1]; t++) {
            const int32_t s = slot_of[uidx[t]];
            if (s >= 0) acc[s] += w;
        }
    }
}

// Replica rows per hot slot.  R_s = the smallest power of two >= share_s / unit, in [1, max_r], where share_s is the expected number of
// updates the item receives per sample (its positive share, + 1 / I where negatives go through the replicas as well).  The rows lie
// compactly, slot after slot: meta[s] = hot_code(first row, log2 R_s).  Returns the rows in all (sum of R_s).
inline int64_t hot_replica_layout(const std::vector<uint64_t> &acc, int64_t users_with_feedback, int64_t I, bool neg, double unit,
                                  int max_r, std::vector<int32_t> &meta) {
    meta.assign(acc.size(), 0);
    int64_t rows = 0;
    for (size_t s = 0; s < acc.size(); s++) {
        const double share = (double)acc[s] / 4294967296.0 / (double)std::max<int64_t>(1, users_with_feedback) + (neg ? 1.0 / (double)I : 0.0);
        int lg = 0;
        while ((1 << lg) < max_r && (double)(1 << lg) * unit < share) lg++;
        meta[s] = hot_code(rows, lg);
        rows += (int64_t)1 << lg;
    }
    return rows;
}

}  // namespace gorse
