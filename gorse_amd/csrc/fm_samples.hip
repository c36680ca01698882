// fm_samples.hip -- training and evaluating the CTR model from (user, item) samples: the reference's own form of a CTR data set
// (model/ctr/data.go:152-267: one label row per user and per item, one embedding per item, and per sample only
// (Users[i], Items[i], Target[i]); Dataset.Get composes the row and looks the embedding up by item).
//
// gorse_fm_set_train_samples keeps the users' rows and three numbers per sample; the item side is the resident catalogue of
// gorse_fm_set_items, read in place.  gorse_fm_epoch (fm.hip) runs its one loop over the TrainSource in here:
//   fm_forward_kernel<G, NF, ComposedRows, kTrain>   the row composed on the device from the batch's user[] / item[]
//   att_{score,exp,enc}_kernel<ItemRows>             the branch over one batch whose row r reads row item[r] of the table
//   att_bwd_gx_items_kernel, att_grad_items_kernel   the two backward kernels that read x, through the same source
//   fm_accum_samples_kernel<G, NF>                   the accumulation over (row, value) lists (fm_samples_plan.hpp)
// -- each the arithmetic of the padded route's kernel (fm_internal.hpp, fm_train.hpp), so every bit equals what
// gorse_fm_set_train + gorse_fm_set_train_embeddings give on the materialised rows.  gorse_fm_set_test_samples keeps a test
// split the same way; gorse_fm_evaluate (fm_eval.hip) scores it through score_rounds<ComposedRows> and the catalogue's tables.
#include "fm_train.hpp"
#include "fm_samples_plan.hpp"

namespace gorse {
namespace fm {

template <int G, int NF>
__global__ __launch_bounds__(kBlock) void fm_accum_samples_kernel(AccArgs a, SampleEntries e) {
    fm_accum_body<G, NF>(a, e);
}

__global__ __launch_bounds__(kBlock) void att_bwd_gx_items_kernel(AttArgs a, ItemRows rows) { att_bwd_gx_body(a, rows); }

__global__ __launch_bounds__(kBlock) void att_grad_items_kernel(AttArgs a, ItemRows rows) { att_grad_body(a, rows); }

// ---- host side ----------------------------------------------------------------------------------------------------------------

// fn(k0, k1) on the batches [k0, k1), split over a few of the host's cores where there are enough batches
struct ThreadedBatches {
    template <class F>
    void operator()(int64_t nb, F fn) const {
        const int nt = (int)std::min<int64_t>(std::min(16u, std::max(1u, std::thread::hardware_concurrency())), nb / 16);
        if (nt < 2) {
            fn((int64_t)0, nb);
            return;
        }
        std::vector<std::thread> th;
        for (int t = 0; t < nt; t++) th.emplace_back([&, t] { fn(nb * t / nt, nb * (t + 1) / nt); });
        for (auto &x : th) x.join();
    }
};

struct SamplesTrain final : TrainSource {
    const float *targets(const gorse_fm *h) const override { return h->smp->tgt.p; }
    int32_t ready(const gorse_fm *h) const override {
        if (!h->cat) return fail(GORSE_ERR_INVALID, "the sample-form training set has no item catalogue (gorse_fm_set_items)");
        return GORSE_OK;
    }
    int32_t plan(gorse_fm *h, int32_t bs, int64_t *max_slots) const override {
        SampleSet &S = *h->smp;
        if (S.plan_bs != bs) {
            const Catalogue &c = *h->cat;
            const SideRows U{S.h_uptr.data(), S.h_uidx.data(), S.h_uval.data(), S.h_ulead.data()};
            const SideRows I{c.h_ptr.data(), c.h_idx.data(), c.h_val.data(), c.h_lead.data()};
            SamplePlan p;
            if (!plan_samples(U, I, S.h_user.data(), S.h_item.data(), S.n, bs, p, ThreadedBatches{}))
                return fail(GORSE_ERR_INVALID, "a batch of %d samples holds more than 2^31 - 1 nonzero entries", bs);
            S.plan_bs = 0;
            GORSE_TRY(upload(S.uniq, p.uniq.data(), p.uniq.size()));
            GORSE_TRY(upload(S.seg, p.seg.data(), p.seg.size()));
            GORSE_TRY(upload(S.row, p.row.data(), p.row.size()));
            GORSE_TRY(upload(S.val, p.val.data(), p.val.size()));
            S.uoff = std::move(p.uoff), S.eoff = std::move(p.eoff);
            S.max_slots = p.max_slots;
            S.plan_bs = bs;
        }
        *max_slots = S.max_slots;
        return GORSE_OK;
    }
    int32_t forward(gorse_fm *h, int64_t r0, int64_t nr) const override {
        const SampleSet &S = *h->smp;
        const Catalogue &c = *h->cat;
        ComposedRows src{};
        src.uptr = S.users.ptr.p, src.uidx = S.users.idx.p, src.uval = S.users.val.p, src.ulead = S.users.lead.p;
        src.iptr = c.ptr.p, src.iidx = c.idx.p, src.ival = c.val.p, src.ilead = c.lead.p;
        src.round(S.user.p, S.item.p, r0);
        return train_forward(h, src, S.tgt.p + r0, nr);
    }
    // the field's table is read in place: no per-batch copy of the embeddings
    AttArgs args(gorse_fm *h, int e, int64_t nr) const { return branch_args(h, e, h->cat->emb[e].p, nr, h->vx.p, true); }
    int32_t branch_forward(gorse_fm *h, int e, int64_t r0, int64_t nr) const override {
        return fm::branch_forward(h->s, args(h, e, nr), ItemRows{h->smp->item.p + r0});
    }
    int32_t branch_gx(gorse_fm *h, int e, int64_t r0, int64_t nr) const override {
        att_bwd_gx_items_kernel<<<dim3(row_grid(nr)), dim3(kBlock), 0, h->s>>>(args(h, e, nr), ItemRows{h->smp->item.p + r0});
        GORSE_HIP_CHECK(hipGetLastError());
        return GORSE_OK;
    }
    int32_t branch_grad(gorse_fm *h, int e, int64_t r0, int64_t nr) const override {
        const AttArgs a = args(h, e, nr);
        att_grad_items_kernel<<<grad_grid(a), dim3(kBlock), 0, h->s>>>(a, ItemRows{h->smp->item.p + r0});
        GORSE_HIP_CHECK(hipGetLastError());
        return GORSE_OK;
    }
    int32_t accum(gorse_fm *h, int64_t k, int64_t, int64_t nr, int64_t tag_hi) const override {
        const SampleSet &S = *h->smp;
        AccArgs a = accum_args(h, nr, tag_hi);
        const int64_t u0 = S.uoff[(size_t)k], e0 = S.eoff[(size_t)k];
        a.uniq = S.uniq.p + u0, a.seg = S.seg.p + u0 + k;  // every batch's offsets end with one more entry
        a.slot0 = 0, a.nslots = S.uoff[(size_t)k + 1] - u0;
        const SampleEntries ent{S.row.p + e0, S.val.p + e0};
        const int64_t grid = ceil_div(a.nslots * 64, kBlock) + 1;
        with_lanes(h->d, [&](auto G, auto NF) {
            fm_accum_samples_kernel<decltype(G)::value, decltype(NF)::value><<<dim3((unsigned)grid), dim3(kBlock), 0, h->s>>>(a, ent);
        });
        GORSE_HIP_CHECK(hipGetLastError());
        return GORSE_OK;
    }
};

const TrainSource &samples_source() {
    static const SamplesTrain src;
    return src;
}

// everything both calls refuse, before anything is touched
int32_t check_samples(const gorse_fm *h, int64_t n_users, const int64_t *uptr, const int32_t *uidx, const float *uval,
                      const int32_t *ulead, int64_t n, const int32_t *user, const int32_t *item, const float *target) {
    if (!h->cat) return fail(GORSE_ERR_INVALID, "no item catalogue (gorse_fm_set_items): samples index its rows");
    if (n > INT32_MAX) return fail(GORSE_ERR_INVALID, "n must be below 2^31");
    if (n_users < 0 || n_users > INT32_MAX) return fail(GORSE_ERR_INVALID, "n_users must be in [0, 2^31)");
    if (!user || !item || !target) return fail(GORSE_ERR_INVALID, "user / item / target is NULL");
    GORSE_TRY(check_side(h, n_users, uptr, uidx, uval, ulead, "users"));
    for (int64_t i = 0; i < n; i++) {
        if (user[i] < 0 || user[i] >= n_users)
            return fail(GORSE_ERR_RANGE, "user %d of sample %lld is outside [0,%lld)", user[i], (long long)i, (long long)n_users);
        if (item[i] < 0 || item[i] >= h->cat->n_items)
            return fail(GORSE_ERR_RANGE, "item %d of sample %lld is outside the catalogue's [0,%lld)", item[i], (long long)i,
                        (long long)h->cat->n_items);
    }
    return GORSE_OK;
}

int32_t upload_users(UserSide &u, int64_t n_users, const int64_t *uptr, const int32_t *uidx, const float *uval, const int32_t *ulead) {
    u.n_users = n_users;
    GORSE_TRY(upload(u.ptr, uptr, (size_t)n_users + 1));
    GORSE_TRY(upload(u.idx, uidx, (size_t)uptr[n_users]));
    GORSE_TRY(upload(u.val, uval, (size_t)uptr[n_users]));
    if (ulead) return upload(u.lead, ulead, (size_t)n_users);
    GORSE_TRY(u.lead.alloc((size_t)n_users));
    if (n_users) GORSE_HIP_CHECK(hipMemset(u.lead.p, 0, (size_t)n_users * sizeof(int32_t)));
    return GORSE_OK;
}

}  // namespace fm
}  // namespace gorse

using namespace gorse;

extern "C" int32_t gorse_fm_set_train_samples(gorse_fm *h, int64_t n_users, const int64_t *user_indptr, const int32_t *user_indices,
                                              const float *user_values, const int32_t *user_lead, int64_t n, const int32_t *user,
                                              const int32_t *item, const float *target) {
    if (!h) return fail(GORSE_ERR_INVALID, "handle is NULL");
    if (n <= 0) return fail(GORSE_ERR_INVALID, "the training set is empty");
    GORSE_TRY(fm::check_samples(h, n_users, user_indptr, user_indices, user_values, user_lead, n, user, item, target));
    GORSE_HIP_CHECK(hipSetDevice(h->device));
    const int64_t unnz = user_indptr[n_users];
    GORSE_TRY(fm::check_fits((double)(n_users + 1) * 8 + (double)n_users * 4 + (double)unnz * 8 + (double)n * 12, "training set"));
    // built beside the present set, which stays until the new one is complete
    std::unique_ptr<fm::SampleSet> S(new (std::nothrow) fm::SampleSet());
    if (!S) return fail(GORSE_ERR_NOMEM, "out of host memory");
    S->n = n;
    GORSE_TRY(fm::upload_users(S->users, n_users, user_indptr, user_indices, user_values, user_lead));
    GORSE_TRY(fm::upload(S->user, user, (size_t)n));
    GORSE_TRY(fm::upload(S->item, item, (size_t)n));
    GORSE_TRY(fm::upload(S->tgt, target, (size_t)n));
    S->h_uptr.assign(user_indptr, user_indptr + n_users + 1);
    S->h_uidx.assign(user_indices, user_indices + unnz);
    S->h_uval.assign(user_values, user_values + unnz);
    if (user_lead) S->h_ulead.assign(user_lead, user_lead + n_users);
    else S->h_ulead.assign((size_t)n_users, 0);
    S->h_user.assign(user, user + n);
    S->h_item.assign(item, item + n);
    GORSE_HIP_CHECK(hipStreamSynchronize(h->s));
    // the sample form replaces a padded set: its rows, its plan and its per-sample embeddings go
    for (auto *b : {&h->idx, &h->uniq, &h->seg, &h->pos}) b->release();
    for (auto *b : {&h->val, &h->tgt}) b->release();
    std::vector<int32_t>().swap(h->h_idx);
    std::vector<float>().swap(h->h_val);
    h->plan_bs = 0, h->width = 0;
    for (int k = 0; k < h->n_fields; k++) {
        h->fld[k].x.release();
        h->fld[k].have_x = false;
    }
    h->smp = std::move(S);
    h->n = n;
    h->smp_dropped = false;
    return GORSE_OK;
}

extern "C" int32_t gorse_fm_set_test_samples(gorse_fm *h, int64_t n_users, const int64_t *user_indptr, const int32_t *user_indices,
                                             const float *user_values, const int32_t *user_lead, int64_t n, const int32_t *user,
                                             const int32_t *item, const float *target) {
    if (!h) return fail(GORSE_ERR_INVALID, "handle is NULL");
    if (n < 0) return fail(GORSE_ERR_INVALID, "n must be in [0, 2^31)");
    GORSE_HIP_CHECK(hipSetDevice(h->device));
    if (n == 0) {
        GORSE_HIP_CHECK(hipStreamSynchronize(h->s));
        h->test.reset();
        h->test_dropped = false;
        return GORSE_OK;
    }
    GORSE_TRY(fm::check_samples(h, n_users, user_indptr, user_indices, user_values, user_lead, n, user, item, target));
    const int64_t unnz = user_indptr[n_users];
    GORSE_TRY(fm::check_fits((double)(n_users + 1) * 8 + (double)n_users * 4 + (double)unnz * 8 + (double)n * 16, "test split"));
    std::unique_ptr<fm::TestSplit> t(new (std::nothrow) fm::TestSplit());
    if (!t) return fail(GORSE_ERR_NOMEM, "out of host memory");
    t->n = n, t->samples = true;
    t->n_pos = fm::eval_partition(target, n, t->order);
    t->s_user.resize((size_t)n), t->s_item.resize((size_t)n);
    for (int64_t r = 0; r < n; r++) {
        t->s_user[(size_t)r] = user[t->order[(size_t)r]];
        t->s_item[(size_t)r] = item[t->order[(size_t)r]];
    }
    GORSE_TRY(fm::upload_users(t->users, n_users, user_indptr, user_indices, user_values, user_lead));
    GORSE_HIP_CHECK(hipStreamSynchronize(h->s));
    h->test = std::move(t);
    h->test_dropped = false;
    return GORSE_OK;
}
