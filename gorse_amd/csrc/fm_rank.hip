// fm_rank.hip -- ranking many users' candidates by the CTR model from a resident item catalogue: the bulk form of the worker's
// per-user loop (worker/pipeline.go:451-499, rankByClickTroughRate -> BatchPredict, model/ctr/fm.go:180-229 -> cache.SortDocuments).
//
// gorse_fm_set_items keeps the item side on the device: the items' feature rows (one CSR), each row's count of leading entries,
// and one n_items x D bf16 embedding table per field.  gorse_fm_rank_users plans the call's slices (every user's candidates
// sliced on their own, fm_eval_plan.hpp), uploads the users and the plan once, has score_rounds (fm_resident.hip) compose and
// score every (user, candidate) row on the device in BatchPredict's order (fm.go:183-206), and sorts every user's list there:
//   fm_rank_sort_kernel     one workgroup per user list of up to kSortCap entries: a bitonic sort of (key << 32 | position) in
//                           LDS.  The keys are unique, so the network's instability cannot show.
// gorse_fm_rank_cand takes the lists from a finished candidate chain on the device; gorse_fm_rank_cand_decayed scores the same way
// and hands the scores to cand_replace.hip's decay and sort (cand_decay_sort) in place of the sort above.
#include "cand_internal.hpp"
#include "fm_internal.hpp"
#include "fm_rank_order.hpp"

namespace gorse {
namespace fm {

constexpr int kSortCap = 4096;  // entries of the longest list sorted on the device: 32 KB of LDS

// test hooks (gorse_hip_test_set_fm_rank): 0 = the library's choice
static int64_t g_round_rows = 0;
static int32_t g_sort_cap = 0;

struct SortArgs {
    const int64_t *cptr;  // n_users + 1
    const float *scores;
    int32_t *order;
    int32_t cap;  // lists longer than this are left to the host
};

__global__ __launch_bounds__(kBlock) void fm_rank_sort_kernel(SortArgs a) {
    __shared__ uint64_t key[kSortCap];
    const int64_t base = a.cptr[blockIdx.x];
    const int64_t n64 = a.cptr[blockIdx.x + 1] - base;
    if (n64 <= 0 || n64 > a.cap) return;  // the whole workgroup
    const int n = (int)n64;
    int P = 1;
    while (P < n) P <<= 1;
    for (int i = threadIdx.x; i < P; i += kBlock)
        key[i] = i < n ? ((uint64_t)rank_key(__float_as_uint(a.scores[base + i])) << 32) | (uint32_t)i : ~(uint64_t)0;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < P / 2; i += kBlock) {
                const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo | j;
                const bool ascending = (lo & k) == 0;
                const uint64_t x = key[lo], y = key[hi];
                if ((x > y) == ascending) {
                    key[lo] = y;
                    key[hi] = x;
                }
            }
            __syncthreads();
        }
    }
    for (int i = threadIdx.x; i < n; i += kBlock) a.order[base + i] = (int32_t)(uint32_t)key[i];
}

// pointer[0] == 0 and non-decreasing
int32_t check_pointer(const int64_t *ptr, int64_t n, const char *what) {
    if (!ptr) return fail(GORSE_ERR_INVALID, "%s is NULL", what);
    if (ptr[0] != 0) return fail(GORSE_ERR_INVALID, "%s[0] must be 0 (got %lld)", what, (long long)ptr[0]);
    for (int64_t i = 0; i < n; i++)
        if (ptr[i + 1] < ptr[i]) return fail(GORSE_ERR_INVALID, "%s decreases at %lld", what, (long long)i);
    return GORSE_OK;
}

// the feature rows of one side: entries in range, lead[i] within row i
int32_t check_side(const gorse_fm *h, int64_t n, const int64_t *ptr, const int32_t *idx, const float *val, const int32_t *lead,
                   const char *what) {
    GORSE_TRY(check_pointer(ptr, n, what));
    const int64_t nnz = ptr[n];
    if (nnz > 0 && (!idx || !val)) return fail(GORSE_ERR_INVALID, "%s: indices / values are NULL", what);
    for (int64_t e = 0; e < nnz; e++)
        if (idx[e] < 0 || idx[e] >= h->nf)
            return fail(GORSE_ERR_RANGE, "%s: feature index %d at entry %lld out of range [0,%lld)", what, idx[e], (long long)e,
                        (long long)h->nf);
    if (lead)
        for (int64_t i = 0; i < n; i++)
            if (lead[i] < 0 || lead[i] > ptr[i + 1] - ptr[i])
                return fail(GORSE_ERR_INVALID, "%s: lead %d of row %lld is beyond its %lld entries", what, lead[i], (long long)i,
                            (long long)(ptr[i + 1] - ptr[i]));
    return GORSE_OK;
}

// the device's order of the lists up to cap entries; longer lists (host_scores != NULL when there are any) by std::stable_sort
// with the same comparator
int32_t download_order(gorse_fm *h, int64_t n_users, const int64_t *cand_indptr, int32_t cap, const float *host_scores,
                       int32_t *order_out) {
    const int64_t total = cand_indptr[n_users];
    GORSE_HIP_CHECK(hipMemcpy(order_out, h->r_order.p, (size_t)total * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (host_scores)
        for (int64_t t = 0; t < n_users; t++) {
            const int64_t c0 = cand_indptr[t], n = cand_indptr[t + 1] - c0;
            if (n > cap) rank_positions(host_scores + c0, n, order_out + c0);
        }
    return GORSE_OK;
}

}  // namespace fm
}  // namespace gorse

using namespace gorse;

extern "C" void gorse_hip_test_set_fm_rank(int64_t round_rows, int32_t sort_cap) {
    fm::g_round_rows = round_rows > 0 ? round_rows : 0;
    fm::g_sort_cap = sort_cap > 0 ? std::min<int32_t>(sort_cap, fm::kSortCap) : 0;
}

extern "C" int32_t gorse_fm_set_items(gorse_fm *h, int64_t n_items, const int64_t *indptr, const int32_t *indices,
                                      const float *values, const int32_t *lead, const uint16_t *const *emb) {
    if (!h) return fail(GORSE_ERR_INVALID, "handle is NULL");
    if (n_items < 0 || n_items > INT32_MAX) return fail(GORSE_ERR_INVALID, "n_items must be in [0, 2^31)");
    GORSE_HIP_CHECK(hipSetDevice(h->device));
    if (n_items == 0) {
        GORSE_HIP_CHECK(hipStreamSynchronize(h->s));
        fm::drop_sample_sets(h);  // they index the catalogue that goes away
        h->cat.reset();
        return GORSE_OK;
    }
    GORSE_TRY(fm::check_side(h, n_items, indptr, indices, values, lead, "items"));
    GORSE_TRY(fm::check_emb(h, emb));
    const int64_t nnz = indptr[n_items];
    double bytes = (double)(n_items + 1) * 8 + (double)n_items * 4 + (double)nnz * 8;
    for (int k = 0; k < h->n_fields; k++) bytes += (double)n_items * h->fld[k].D * 2;
    GORSE_TRY(fm::check_fits(bytes, "catalogue"));
    // built beside the resident one, which stays until the new one is complete
    std::unique_ptr<fm::Catalogue> c(new (std::nothrow) fm::Catalogue());
    if (!c) return fail(GORSE_ERR_NOMEM, "out of host memory");
    c->n_items = n_items;
    GORSE_TRY(fm::upload(c->ptr, indptr, (size_t)n_items + 1));
    GORSE_TRY(fm::upload(c->idx, indices, (size_t)nnz));
    GORSE_TRY(fm::upload(c->val, values, (size_t)nnz));
    if (lead) {
        GORSE_TRY(fm::upload(c->lead, lead, (size_t)n_items));
    } else {
        GORSE_TRY(c->lead.alloc((size_t)n_items));
        GORSE_HIP_CHECK(hipMemset(c->lead.p, 0, (size_t)n_items * sizeof(int32_t)));
    }
    for (int k = 0; k < h->n_fields; k++) GORSE_TRY(fm::upload(c->emb[k], emb[k], (size_t)n_items * (size_t)h->fld[k].D));
    // the host's copy of the rows (not of the tables): what a sample-form training set's plan is built from
    c->h_ptr.assign(indptr, indptr + n_items + 1);
    c->h_idx.assign(indices, indices + nnz);
    c->h_val.assign(values, values + nnz);
    if (lead) c->h_lead.assign(lead, lead + n_items);
    else c->h_lead.assign((size_t)n_items, 0);
    GORSE_HIP_CHECK(hipStreamSynchronize(h->s));
    fm::drop_sample_sets(h);  // they index the catalogue that is replaced
    h->cat = std::move(c);
    return GORSE_OK;
}

// The validated call: user t's candidates are cand[cand_indptr[t] ..) on the host, or, with cand == NULL, d_cand[cand_indptr[t] ..)
// on the device (a finished candidate chain's items).
static int32_t rank_lists(gorse_fm *h, int64_t n_users, const int64_t *user_indptr, const int32_t *user_indices, const float *user_values,
                          const int32_t *user_lead, const int64_t *cand_indptr, const int32_t *cand, const int32_t *d_cand,
                          int32_t batch_size, const volatile int32_t *cancel, float *scores_out, int32_t *order_out) {
    const fm::Catalogue &cat = *h->cat;
    const int64_t total = cand_indptr[n_users];
    GORSE_HIP_CHECK(hipSetDevice(h->device));

    // rows, slices (per user, batch_size rows each, the last one partial) and launch rounds (whole slices, at most R rows)
    const int maxD = fm::max_emb_dim(h);
    const int32_t cap = fm::g_sort_cap > 0 ? fm::g_sort_cap : fm::kSortCap;
    int64_t n_long = 0;
    for (int64_t t = 0; t < n_users; t++) n_long += cand_indptr[t + 1] - cand_indptr[t] > cap;
    fm::SlicePlan plan;
    fm::plan_slices(cand_indptr, n_users, cand, batch_size, fm::round_rows_for(maxD, h->d, batch_size, fm::g_round_rows), plan);

    // one upload of the users and the plan; scratch for the longest round
    std::vector<int32_t> zero_lead;
    if (!user_lead) zero_lead.assign((size_t)n_users, 0);
    GORSE_TRY(fm::upload(h->r_uptr, user_indptr, (size_t)n_users + 1));
    GORSE_TRY(fm::upload(h->r_uidx, user_indices, (size_t)user_indptr[n_users]));
    GORSE_TRY(fm::upload(h->r_uval, user_values, (size_t)user_indptr[n_users]));
    GORSE_TRY(fm::upload(h->r_ulead, user_lead ? user_lead : zero_lead.data(), (size_t)n_users));
    GORSE_TRY(fm::upload(h->r_cptr, cand_indptr, (size_t)n_users + 1));
    GORSE_TRY(fm::upload_plan(h->r_plan, plan, total));
    if (!cand && total > 0)  // the plan's item column (segment | item | ...) from the lists on the device, on the stream of its readers
        GORSE_HIP_CHECK(hipMemcpyAsync(h->r_plan.desc.p + total, d_cand, (size_t)total * sizeof(int32_t), hipMemcpyDeviceToDevice, h->s));
    GORSE_TRY(h->r_scores.ensure((size_t)total));
    if (order_out) GORSE_TRY(h->r_order.ensure((size_t)total));
    if (h->n_fields > 0) GORSE_TRY(h->rs.ensure(h->r_plan.max_round, h->d, maxD));
    GORSE_TRY(fm::ensure_events(h->r_ev));

    GORSE_HIP_CHECK(hipEventRecord(h->r_ev[0], h->s));
    fm::ComposedRows src{};
    src.uptr = h->r_uptr.p, src.uidx = h->r_uidx.p, src.uval = h->r_uval.p, src.ulead = h->r_ulead.p;
    src.iptr = cat.ptr.p, src.iidx = cat.idx.p, src.ival = cat.val.p, src.ilead = cat.lead.p;
    GORSE_TRY(fm::score_rounds(h, h->r_plan, src, cat.emb, cancel, h->rs, h->r_scores.p));
    if (order_out && total > 0) {
        fm::SortArgs s{h->r_cptr.p, h->r_scores.p, h->r_order.p, cap};
        fm::fm_rank_sort_kernel<<<dim3((unsigned)n_users), dim3(fm::kBlock), 0, h->s>>>(s);
        GORSE_HIP_CHECK(hipGetLastError());
    }
    GORSE_HIP_CHECK(hipEventRecord(h->r_ev[1], h->s));
    GORSE_HIP_CHECK(hipStreamSynchronize(h->s));
    float ms = 0.0f;
    GORSE_HIP_CHECK(hipEventElapsedTime(&ms, h->r_ev[0], h->r_ev[1]));

    std::vector<float> tmp_scores;
    const float *host_scores = scores_out;
    if (total > 0 && (scores_out || (order_out && n_long > 0))) {
        float *dst = scores_out;
        if (!dst) {
            tmp_scores.resize((size_t)total);
            dst = tmp_scores.data();
            host_scores = dst;
        }
        GORSE_HIP_CHECK(hipMemcpy(dst, h->r_scores.p, (size_t)total * sizeof(float), hipMemcpyDeviceToHost));
    }
    if (order_out && total > 0) GORSE_TRY(fm::download_order(h, n_users, cand_indptr, cap, n_long > 0 ? host_scores : nullptr, order_out));
    h->rk_rows = total, h->rk_slices = h->r_plan.n_slices, h->rk_rounds = h->r_plan.rounds();
    h->rk_host_sorted = order_out ? n_long : 0;
    h->rk_ms = ms;
    return GORSE_OK;
}

extern "C" int32_t gorse_fm_rank_users(gorse_fm *h, int64_t n_users, const int64_t *user_indptr, const int32_t *user_indices,
                                       const float *user_values, const int32_t *user_lead, const int64_t *cand_indptr,
                                       const int32_t *cand, int32_t batch_size, const volatile int32_t *cancel, float *scores_out,
                                       int32_t *order_out) {
    if (!h) return fail(GORSE_ERR_INVALID, "handle is NULL");
    if (!h->cat) return fail(GORSE_ERR_INVALID, "no item catalogue (gorse_fm_set_items)");
    if (batch_size <= 0) return fail(GORSE_ERR_INVALID, "batch_size must be positive");
    if (n_users < 0 || n_users > INT32_MAX) return fail(GORSE_ERR_INVALID, "n_users must be in [0, 2^31)");
    if (n_users == 0) {
        h->rk_rows = h->rk_slices = h->rk_rounds = h->rk_host_sorted = 0;
        h->rk_ms = 0.0;
        return GORSE_OK;
    }
    GORSE_TRY(fm::check_side(h, n_users, user_indptr, user_indices, user_values, user_lead, "users"));
    GORSE_TRY(fm::check_pointer(cand_indptr, n_users, "cand_indptr"));
    const int64_t total = cand_indptr[n_users];
    if (total > INT32_MAX) return fail(GORSE_ERR_INVALID, "more than 2^31 - 1 candidates in one call: split the users");
    if (total > 0 && !cand) return fail(GORSE_ERR_INVALID, "cand is NULL");
    const fm::Catalogue &cat = *h->cat;
    for (int64_t e = 0; e < total; e++)
        if (cand[e] < 0 || cand[e] >= cat.n_items)
            return fail(GORSE_ERR_RANGE, "candidate %d at position %lld is outside the catalogue's [0,%lld)", cand[e], (long long)e,
                        (long long)cat.n_items);
    return rank_lists(h, n_users, user_indptr, user_indices, user_values, user_lead, cand_indptr, cand, nullptr, batch_size, cancel,
                      scores_out, order_out);
}

// what gorse_fm_rank_cand and gorse_fm_rank_cand_decayed ask of their handles and users before anything runs
static int32_t check_rank_cand(const gorse_fm *h, const gorse_cand *c, const char *who, const int64_t *user_indptr, const int32_t *user_indices,
                               const float *user_values, const int32_t *user_lead, int32_t batch_size) {
    if (!h || !c) return fail(GORSE_ERR_INVALID, "handle is NULL");
    if (!h->cat) return fail(GORSE_ERR_INVALID, "no item catalogue (gorse_fm_set_items)");
    if (batch_size <= 0) return fail(GORSE_ERR_INVALID, "batch_size must be positive");
    if (!c->pass.begun || !c->pass.finished) return fail(GORSE_ERR_INVALID, "%s: the chain has no finished pass (gorse_cand_finish)", who);
    if (c->device != h->device) return fail(GORSE_ERR_INVALID, "%s: the chain is on device %d, the ranker on device %d", who, c->device, h->device);
    if (c->n_items != h->cat->n_items)
        return fail(GORSE_ERR_INVALID, "%s: the chain has %lld items, the catalogue %lld", who, (long long)c->n_items,
                    (long long)h->cat->n_items);
    if (c->pass.n_queries == 0) return GORSE_OK;
    GORSE_TRY(fm::check_side(h, c->pass.n_queries, user_indptr, user_indices, user_values, user_lead, "users"));
    if (c->f_ptr_h.back() > INT32_MAX) return fail(GORSE_ERR_INVALID, "more than 2^31 - 1 candidates in one call: split the users");
    return GORSE_OK;
}

extern "C" int32_t gorse_fm_rank_cand(gorse_fm *h, gorse_cand *c, const int64_t *user_indptr, const int32_t *user_indices,
                                      const float *user_values, const int32_t *user_lead, int32_t batch_size,
                                      const volatile int32_t *cancel, float *scores_out, int32_t *order_out) {
    GORSE_TRY(check_rank_cand(h, c, "gorse_fm_rank_cand", user_indptr, user_indices, user_values, user_lead, batch_size));
    const int64_t n_users = c->pass.n_queries;
    if (n_users == 0) {
        h->rk_rows = h->rk_slices = h->rk_rounds = h->rk_host_sorted = 0;
        h->rk_ms = 0.0;
        return GORSE_OK;
    }
    // (the chain's items lie in [0, n_items): every stage's input was held against it)
    return rank_lists(h, n_users, user_indptr, user_indices, user_values, user_lead, c->f_ptr_h.data(), nullptr, c->f_item.p, batch_size, cancel,
                      scores_out, order_out);
}

// gorse_fm_rank_cand's scores, then the replacement decay and the sort of the decayed doubles (cand_replace.hip) on the same stream;
// lists past the device sort's cap by the host with the same order (cand_replace_plan.hpp)
extern "C" int32_t gorse_fm_rank_cand_decayed(gorse_fm *h, gorse_cand *c, const int64_t *user_indptr, const int32_t *user_indices,
                                              const float *user_values, const int32_t *user_lead, int32_t batch_size,
                                              const volatile int32_t *cancel, double positive_decay, double read_decay, float *scores_out,
                                              double *final_out, int32_t *order_out) {
    const char *who = "gorse_fm_rank_cand_decayed";
    GORSE_TRY(check_rank_cand(h, c, who, user_indptr, user_indices, user_values, user_lead, batch_size));
    std::string msg;
    const int32_t rc = cand::validate_decays(positive_decay, read_decay, &msg);
    if (rc != GORSE_OK) return fail(rc, "%s: %s", who, msg.c_str());
    const int64_t n_users = c->pass.n_queries;
    if (n_users == 0) {
        h->rk_rows = h->rk_slices = h->rk_rounds = h->rk_host_sorted = 0;
        h->rk_ms = 0.0;
        return GORSE_OK;
    }
    const int64_t *cptr = c->f_ptr_h.data();
    const int64_t total = cptr[n_users];
    const int32_t cap = fm::g_sort_cap > 0 ? fm::g_sort_cap : fm::kSortCap;
    int64_t n_long = 0;
    for (int64_t t = 0; t < n_users; t++) n_long += cptr[t + 1] - cptr[t] > cap;
    const bool fallback = order_out && n_long > 0;
    std::vector<float> tmp_scores;
    float *host_scores = scores_out;
    if (fallback && !host_scores && total > 0) {
        tmp_scores.resize((size_t)total);
        host_scores = tmp_scores.data();
    }
    GORSE_TRY(rank_lists(h, n_users, user_indptr, user_indices, user_values, user_lead, cptr, nullptr, c->f_item.p, batch_size, cancel,
                         host_scores, nullptr));
    if (total == 0) return GORSE_OK;
    GORSE_TRY(h->r_final.ensure((size_t)total));
    GORSE_TRY(h->r_order.ensure((size_t)total));
    GORSE_HIP_CHECK(hipEventRecord(h->r_ev[0], h->s));
    GORSE_TRY(cand_decay_sort(c, h->s, h->r_scores.p, positive_decay, read_decay, cap, h->r_final.p, h->r_order.p));
    GORSE_HIP_CHECK(hipEventRecord(h->r_ev[1], h->s));
    GORSE_HIP_CHECK(hipStreamSynchronize(h->s));
    float ms = 0.0f;
    GORSE_HIP_CHECK(hipEventElapsedTime(&ms, h->r_ev[0], h->r_ev[1]));
    h->rk_ms += ms;
    std::vector<double> tmp_final;
    double *host_final = final_out;
    if (fallback && !host_final) {
        tmp_final.resize((size_t)total);
        host_final = tmp_final.data();
    }
    if (host_final) GORSE_HIP_CHECK(hipMemcpy(host_final, h->r_final.p, (size_t)total * sizeof(double), hipMemcpyDeviceToHost));
    if (order_out) {
        GORSE_HIP_CHECK(hipMemcpy(order_out, h->r_order.p, (size_t)total * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (fallback)
            for (int64_t t = 0; t < n_users; t++) {
                const int64_t c0 = cptr[t], n = cptr[t + 1] - c0;
                if (n > cap) cand::decayed_positions(host_scores + c0, host_final + c0, n, order_out + c0);
            }
        h->rk_host_sorted = n_long;
    }
    return GORSE_OK;
}

extern "C" int32_t gorse_fm_rank_stats(gorse_fm *h, int64_t *rows, int64_t *slices, int64_t *rounds, int64_t *host_sorted,
                                       double *device_ms) {
    if (!h) return fail(GORSE_ERR_INVALID, "handle is NULL");
    if (rows) *rows = h->rk_rows;
    if (slices) *slices = h->rk_slices;
    if (rounds) *rounds = h->rk_rounds;
    if (host_sorted) *host_sorted = h->rk_host_sorted;
    if (device_ms) *device_ms = h->rk_ms;
    return GORSE_OK;
}

extern "C" int32_t gorse_hip_test_fm_rank_sort(gorse_fm *h, int64_t n_users, const int64_t *cand_indptr, const float *scores,
                                               int32_t *order_out) {
    if (!h || !scores || !order_out) return fail(GORSE_ERR_INVALID, "handle / scores / order_out is NULL");
    if (n_users <= 0 || n_users > INT32_MAX) return fail(GORSE_ERR_INVALID, "n_users must be in [1, 2^31)");
    GORSE_TRY(fm::check_pointer(cand_indptr, n_users, "cand_indptr"));
    const int64_t total = cand_indptr[n_users];
    if (total <= 0 || total > INT32_MAX) return fail(GORSE_ERR_INVALID, "between 1 and 2^31 - 1 scores");
    GORSE_HIP_CHECK(hipSetDevice(h->device));
    const int32_t cap = fm::g_sort_cap > 0 ? fm::g_sort_cap : fm::kSortCap;
    bool any_long = false;
    for (int64_t t = 0; t < n_users; t++) any_long = any_long || cand_indptr[t + 1] - cand_indptr[t] > cap;
    GORSE_TRY(fm::upload(h->r_cptr, cand_indptr, (size_t)n_users + 1));
    GORSE_TRY(fm::upload(h->r_scores, scores, (size_t)total));
    GORSE_TRY(h->r_order.ensure((size_t)total));
    fm::SortArgs s{h->r_cptr.p, h->r_scores.p, h->r_order.p, cap};
    fm::fm_rank_sort_kernel<<<dim3((unsigned)n_users), dim3(fm::kBlock), 0, h->s>>>(s);
    GORSE_HIP_CHECK(hipGetLastError());
    GORSE_HIP_CHECK(hipStreamSynchronize(h->s));
    return fm::download_order(h, n_users, cand_indptr, cap, any_long ? scores : nullptr, order_out);
}
