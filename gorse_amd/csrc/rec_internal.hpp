// rec_internal.hpp -- what the units of gorse_mf_recommend share: the launch's arguments, the candidate test and the survivor
// buffer's compaction (recommend.hip: the vector kernel, the merge, the literal path, the planner and its constants;
// recommend_mfma.hip: the matrix-core kernel; recommend_sweep.hip: the pilot-threshold schedule; recommend_literal.hip: literal mode 1).
#pragma once
#include <cmath>

#include "mf_internal.hpp"

namespace gorse {

struct RecArgs {
    const float *P, *Q;
    const int32_t *users;  // null: query t is user t
    const int64_t *uptr;
    const int32_t *uidx_sorted;
    const int64_t *sptr;  // null: no seen rows
    const int32_t *seen;  // every row sorted ascending
    const uint8_t *item_ok;
    int64_t q0, nq;  // the launch's queries are [q0, q0 + nq)
    int32_t I, d, k, kk, cap, slices, slice_len, tile_items;
    float *buf_s;     // nq * slices * 2 * cap: two halves per (query, slice), a compaction moves from one to the other
    int32_t *buf_i;
    float *out_s;     // nq * slices * kk: the slice's kk best, sorted by score descending
    int32_t *out_i;
    int32_t *out_cnt;   // nq * slices
    int32_t *nan_flag;  // nq
    // the pilot schedule's second launch (rec_fast_kernel and rec_finish_kernel only): launch query tq is query qmap[tq] of the
    // call, and its result row is qmap[tq] - q0; null: query q0 + tq, row tq
    const int64_t *qmap;
};

// recommend_sweep.hip: the pilot-threshold schedule (gorse_mf_set_recommend_schedule(h, 1)).  One round over the queries [q0, q0 + nq) of
// R: the pilot's thresholds, the sweep's survivor lists, and rec_finish_kernel's result arrays for every query it answers; hb[t] = 1
// marks a query handed back to schedule 0 (its result row is not written), cnt[t] = survivors the sweep counted for it.
struct RecSweepArgs {
    RecArgs R;  // P .. item_ok, q0, nq, I, d, k, kk; the rest is schedule 0's
    int32_t stride, n_sample, samp_ld, cap, pilot_slices, pilot_slice_len, sweep_slices, sweep_slice_len;
    float *samp;       // ceil(nq / 128) * 128 * samp_ld: the sampled scores, a row per query of every launched block
    float *tau;        // nq
    int32_t *cnt;      // nq
    int32_t *hb;       // nq
    int32_t *surv_i;   // nq * cap
    float *surv_s;
    size_t select_lds, finish_lds;
};
int32_t rec_sweep_launch(const RecSweepArgs &S, int32_t *res_items, float *res_scores, int32_t *res_cnt, int32_t *lit, hipStream_t stream);

__device__ __forceinline__ bool rec_candidate(const uint8_t *__restrict__ item_ok, const int32_t *trow, int64_t tn, const int32_t *srow,
                                              int64_t sn, int32_t item) {
    return item_ok[item] != 0 && !row_contains(trow, tn, item) && !(sn > 0 && row_contains(srow, sn, item));
}

// One 16-lane group: the kk best of cnt buffered entries to dst, sorted by score descending (equal scores in buffer order).  Every
// entry is ranked by counting the entries ahead of it.  Returns the kk-th best score (-inf when there are fewer).  No NaN is buffered.
__device__ __forceinline__ float rec_compact(const float *ss, const int32_t *si, int cnt, float *ds, int32_t *di, int kk, int lane) {
    float kth = -INFINITY;
    for (int e = lane; e < cnt; e += kGroup) {
        const float s = ss[e];
        int rank = 0;
        for (int j = 0; j < cnt; j++) {
            const float o = ss[j];
            rank += (o > s || (o == s && j < e)) ? 1 : 0;
        }
        if (rank < kk) {
            ds[rank] = s;
            di[rank] = si[e];
            if (rank == kk - 1) kth = s;
        }
    }
    for (int m = 8; m >= 1; m >>= 1) kth = fmaxf(kth, __shfl_xor(kth, m, kGroup));
    return kth;
}

// recommend_mfma.hip: the matrix-core producer of out_s / out_i / out_cnt / nan_flag (route 1).  It serves nFactors = 16, 32, ... 256;
// a workgroup owns kRecMfmaQueries queries and one slice, so the grid is ceil(nq / kRecMfmaQueries) x slices.
constexpr int kRecMfmaQueries = 128;
constexpr bool rec_mfma_serves(int d) { return d % 16 == 0 && d >= 16 && d <= 256; }
int32_t rec_mfma_launch(const RecArgs &A, hipStream_t stream);

// recommend_literal.hip: literal mode 1 (gorse_mf_set_recommend_literal(h, 1)).  One workgroup per literal query q of [0, nl): user
// lit_user[q], seen row lit_query[q]; the result row -- items, the heap's weights as scores, the -1 / 0 padding, the count -- goes to
// row lit_query[q] of items / scores / cnt (scatter != 0: the call's own device rows) or to row q (a compact nl * k buffer).
// stats[0] / stats[1] gain the candidates that went through push / that were fast-forwarded; the caller clears them.
struct RecLiteralArgs {
    const float *P, *Q;
    const int64_t *uptr;
    const int32_t *uidx_sorted;
    const int64_t *sptr;  // null: no seen rows
    const int32_t *seen;
    const uint8_t *item_ok;
    const int32_t *lit_user;
    const int64_t *lit_query;
    int32_t I, d, k, scatter, no_skip;
    int64_t q0;  // (the launcher's: first query of the launch)
    int32_t *items;
    float *scores;
    int32_t *cnt;
    unsigned long long *stats;
};
// The kernel's LDS: the heap's k + 1 entries, two tiles of buffered candidates and, where it is not held in registers, the user's
// row.  It serves every (d, k) whose sum fits this budget -- k <= 4095 at any nFactors up to 4096 -- and the call takes mode 0
// as a whole otherwise.
constexpr size_t kRecLiteralLdsBytes = (size_t)64 << 10;
size_t rec_literal_lds(int d, int k);
bool rec_literal_serves(int d, int k);
int32_t rec_literal_launch(const RecLiteralArgs &A, int64_t nl, hipStream_t stream);

}  // namespace gorse
