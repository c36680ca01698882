// hot_rows.hpp -- which items of a BPR handle are HOT, and how many replica rows each one gets (csrc/bpr_fold.hpp, HotRows), shared by
// gorse_mf_create and by the CPU test of the rule (host library hook gh_test_bpr_hot_layout, tests/test_bpr_hot_layout_cpu.py).
// Pure host C++ apart from the constexpr helpers the kernels call too: the three that decode a slot's word, and the owner mapping of the
// sole-writer fold at the end (host hook gh_test_bpr_fold_owner, tests/test_bpr_fold_owner_cpu.py).  Reference semantics of the rates: a
// sample draws its user uniformly among the users with feedback, then a positive uniformly from that user's row, then a negative
// uniformly from the catalogue (model/cf/model.go:452-468).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace gorse {

// A hot item's word (hot_slot[item] and hot_meta[slot]): its first replica row << 4 | log2 of its replica count.  Every other class
// of hot_slot is negative (-1 warm, -2 cold), so `word >= 0` means "add to that row" -- a hot item's replica or, on a handle with the
// accumulated tier (below), a warm item's one accumulator row (log2 = 0).
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

// class "cold" (-2): an item expected to be touched -- its share of the feedback as a positive, 1 / I as a negative -- less than once
// per `window` samples (0 = no item is cold)
inline bool item_is_cold(int64_t cnt, int64_t nnz, int64_t I, int64_t window) {
    return window > 0 && nnz > 0 && ((double)cnt / (double)nnz + 1.0 / (double)I) * (double)window < 1.0;
}

// ---- the ACCUMULATED tier: one accumulator row for every warm item of a small catalogue ------------------------------------------
// Atomics onto rows that the same launch gathers run slower than atomics onto rows nobody reads, and the penalty belongs to small
// tables: 24 % at 0.9 MB, 6 % at 7.6 MB, 3 % at 268 MB (profiles/r04_s_probe_atomics3.txt: 318 G dwords/s alone, 241 with agent-scope
// loads of the same rows, 311 with the loads from another table).  Where the whole of Q fits one XCD's L2 (4 MiB) the warm items'
// updates therefore go to a row of their own too, which the tier's folders add to Q every few fold periods (csrc/bpr_fold.hpp).
constexpr int64_t kAccTableBytes = (int64_t)4 << 20;  // I x nFactors x 4 at most: one XCD's L2, between the probe's 0.9 MB and 7.6 MB
constexpr int64_t kUserRunUsers = 4096;               // users from which a handle takes the user-run schedule (bpr_plan.hpp bpr_schedule)
inline bool user_run_width(int d) { return d == 8 || d == 16 || d == 32 || d == 64 || d == 128; }

// whether a handle gets the tier: the user-run schedule natively, no cold item at create (a cold row's update is a store: the store
// route and the tier exclude each other), and a catalogue within kAccTableBytes
inline bool acc_rows_eligible(int64_t U, int64_t I, int d, int64_t n_cold) {
    return U >= kUserRunUsers && user_run_width(d) && n_cold == 0 && I * (int64_t)d * 4 <= kAccTableBytes;
}

// The tier's layout.  slot: the class of every item after the hot layout (hot_code of a hot item, -1 warm, -2 cold); first_row: the
// replica rows in front (hot_replica_layout's return).  Every warm item, ids ascending, takes ONE row behind them: slot[item] and
// meta[k] become hot_code(row, 0), items[k] the item.  Returns the tier's rows (0 and nothing changed where the handle is not
// eligible).
inline int64_t acc_rows_layout(std::vector<int32_t> &slot, int64_t first_row, int64_t U, int d, int64_t n_cold, std::vector<int32_t> &items,
                               std::vector<int32_t> &meta) {
    items.clear();
    meta.clear();
    const int64_t I = (int64_t)slot.size();
    if (!acc_rows_eligible(U, I, d, n_cold)) return 0;
    for (int64_t i = 0; i < I; i++)
        if (slot[(size_t)i] == -1) {
            const int32_t code = hot_code(first_row + (int64_t)items.size(), 0);
            slot[(size_t)i] = code;
            items.push_back((int32_t)i);
            meta.push_back(code);
        }
    return (int64_t)items.size();
}

// ---- the SOLE-WRITER fold: who owns which elements of which slot (csrc/bpr_fold.hpp run_folders, fold_sole_pass) ------------------------
// On a launch whose workers never write Q (every item has a row: the accumulated tier) the folder workgroups are Q's only writers and
// fold with loads and stores: Q <- base + (the slot's rows).  What replaces the atomics is this invariant: every (slot, element group)
// has exactly ONE owner thread for the whole launch, the same in the periodic passes and in the last one.  The hot tier's slots
// [0, n_hot) are shared among the hot tier's workgroups (the first hot_blocks of the `folders`), the accumulated tier's slots
// [n_hot, n_hot + n_acc) among the workgroups behind them; a group is kFoldGroup consecutive elements of a slot (d is a multiple of
// it: user_run_width), groups are numbered slot after slot inside a tier and strided over the tier's threads.
constexpr int kFoldGroup = 2;        // floats a folder thread moves per access: one 8-byte load or store
constexpr int kFolderThreads = 256;  // threads of a folder workgroup (the update kernels' block)
struct FoldShare {
    int s0, s1;         // the tier's slots
    int tid, nthreads;  // this thread among the tier's: it owns the groups tid, tid + nthreads, ... of [0, (s1 - s0) * d / kFoldGroup)
};
// the share of thread `thread` of folder workgroup `block` (a launch with no workgroups behind the hot tier's: one tier of all slots)
constexpr FoldShare fold_share(int block, int thread, int n_hot, int n_acc, int folders, int hot_blocks) {
    if (folders <= hot_blocks) return FoldShare{0, n_hot + n_acc, block * kFolderThreads + thread, folders * kFolderThreads};
    if (block < hot_blocks) return FoldShare{0, n_hot, block * kFolderThreads + thread, hot_blocks * kFolderThreads};
    return FoldShare{n_hot, n_hot + n_acc, (block - hot_blocks) * kFolderThreads + thread, (folders - hot_blocks) * kFolderThreads};
}
constexpr int fold_groups(const FoldShare &sh, int d) { return (sh.s1 - sh.s0) * (d / kFoldGroup); }
// group g of a share: its slot and its first element
constexpr int fold_group_slot(const FoldShare &sh, int g, int d) { return sh.s0 + g / (d / kFoldGroup); }
constexpr int fold_group_elem(int g, int d) { return (g % (d / kFoldGroup)) * kFoldGroup; }

}  // namespace gorse
