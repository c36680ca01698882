// cand_internal.hpp -- the gorse_cand handle (cand.hip, cand_replace.hip); fm_rank.hip reads a finished pass's rows from it.
#pragma once
#include "cand_replace_plan.hpp"
#include "common.hpp"

struct gorse_cand {
    int device = 0;
    int64_t n_items = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    gorse::cand::Pass pass;
    // the base exclusion rows, ascending, as gorse_cand_begin left them
    gorse::DevBuf<int64_t> base_ptr;
    gorse::DevBuf<int32_t> base_items;
    int64_t base_total = 0;
    // the current exclusion rows: a compact CSR with ascending rows in buffer `cur`; a stage merges into the other one
    gorse::DevBuf<int64_t> cur_ptr[2];
    gorse::DevBuf<int32_t> cur_items[2];
    int cur = 0;
    std::vector<int64_t> cur_ptr_h;  // the host's copy of the current row pointer: the one thing a stage brings back
    // the candidates: rows of pass.capacity entries and a count per query
    gorse::DevBuf<int32_t> c_item, c_cnt;
    gorse::DevBuf<unsigned long long> c_score;
    gorse::DevBuf<uint8_t> c_stage;
    int64_t n_candidates = 0;
    // one stage's kept entries (stride k) before they are appended and merged; its inputs
    gorse::DevBuf<int32_t> st_item, st_cnt;
    gorse::DevBuf<unsigned long long> st_score;
    gorse::DevBuf<long long> sums;
    gorse::DevBuf<uint8_t> keep;
    gorse::DevBuf<int64_t> l_ptr;
    gorse::DevBuf<int32_t> l_items;
    gorse::DevBuf<unsigned long long> l_scores;
    gorse::DevBuf<int32_t> mf_items, mf_cnt;  // gorse_mf_recommend's rows, left here by its core
    gorse::DevBuf<float> mf_scores;
    // the finished pass: a compact CSR
    gorse::DevBuf<int64_t> f_ptr;
    gorse::DevBuf<int32_t> f_item;
    gorse::DevBuf<unsigned long long> f_score;
    gorse::DevBuf<uint8_t> f_stage;
    std::vector<int64_t> f_ptr_h;
    std::vector<double> stage_ms, chain_ms;
    // the replacement rows of a pass with pass.replaced (cand_replace.hip): a compact CSR, rows ascending, a kind per item
    gorse::DevBuf<int64_t> r_ptr;
    gorse::DevBuf<int32_t> r_item;
    gorse::DevBuf<uint8_t> r_kind;
    int64_t r_total = 0, r_added = 0, r_positive = 0, r_read = 0;
    double r_ms = 0.0;
    int32_t use() {
        GORSE_HIP_CHECK(hipSetDevice(device));
        return GORSE_OK;
    }
};

namespace gorse {
// cand_replace.hip: every candidate of the chain's finished rows decayed by its kind in its query's replacement row (scores: the
// ranker's floats, CSR-indexed, on the device) into fin, and every list of up to cap entries sorted into order; enqueued on st
int32_t cand_decay_sort(const gorse_cand *c, hipStream_t st, const float *scores, double positive_decay, double read_decay, int32_t cap,
                        double *fin, int32_t *order);
}  // namespace gorse
