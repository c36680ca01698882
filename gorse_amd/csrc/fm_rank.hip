// fm_rank.hip -- ranking many users' candidates by the CTR model from a resident item catalogue: the bulk form of the worker's
// per-user loop (worker/pipeline.go:451-499, rankByClickTroughRate -> BatchPredict, model/ctr/fm.go:180-229 -> cache.SortDocuments).
//
// gorse_fm_set_items keeps the item side on the device: the items' feature rows (one CSR), each row's count of leading entries,
// and one n_items x D bf16 embedding table per field.  gorse_fm_rank_users then composes every (user, candidate) row on the
// device in BatchPredict's order (fm.go:183-206), scores it with the chains of fm_forward_kernel and the attention branch's
// kernel bodies (fm_internal.hpp: the same code, so the same bits), and sorts every user's list on the device.
//
//   fm_rank_forward_kernel  one G-lane group per row: user lead | item lead | user rest | item rest, through the row's
//                           (user, item) descriptor; where a wave's rows all belong to one user the user's entries are read
//                           through the scalar unit.  Writes the FM logit, and vx when the model has fields.
//   att_*_slices_kernel     the branch's three forward launches over MANY slices: every row carries its slice's first row and
//                           length, the Softmax's maxima and sums are indexed by row0 + (local_r D + c) % len, and x is read in
//                           place from table[item[r]].
//   fm_rank_sort_kernel     one workgroup per user list of up to kSortCap entries: a bitonic sort of (key << 32 | position) in
//                           LDS.  The keys are unique, so the network's instability cannot show.
// A launch round covers whole slices of at most R rows in all, R from the scratch a row needs (maxD + 2 d + 2 floats) under
// kRoundBytes; the descriptors of all rounds are built on the host once and uploaded once.
#include "fm_internal.hpp"
#include "fm_rank_order.hpp"

namespace gorse {
namespace fm {

constexpr int64_t kRoundBytes = (int64_t)256 << 20;  // scratch of one launch round at most (unless one slice alone needs more)
constexpr int kSortCap = 4096;                       // entries of the longest list sorted on the device: 32 KB of LDS

// test hooks (gorse_hip_test_set_fm_rank): 0 = the library's choice
static int64_t g_round_rows = 0;
static int32_t g_sort_cap = 0;

struct RankFwdArgs {
    const int64_t *uptr;  // the call's users: CSR pointer, entries, leading entries per user
    const int32_t *uidx;
    const float *uval;
    const int32_t *ulead;
    const int64_t *iptr;  // the catalogue
    const int32_t *iidx;
    const float *ival;
    const int32_t *ilead;
    const int32_t *user, *item;  // per row of the round
    const float *V, *W, *B;
    int64_t nrows;
    int d;
    float *logit;  // nrows
    float *vx;     // nrows x d (VX only)
};

__device__ __forceinline__ int64_t first_lane64(int64_t v) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// entries [j0, j1) of a CSR join the row's chains in order; zero values are skipped as fm_forward_kernel skips them.
// UNIFORM: the range is the same in every lane of the wave (the caller checked), so index and value come through scalar loads.
template <int G, int NF, bool UNIFORM>
__device__ __forceinline__ void walk(const RankFwdArgs &a, const int32_t *idx, const float *val, int64_t j0, int64_t j1, int lane,
                                     float (&vx)[NF], float (&sq)[NF], float &lin) {
    if (UNIFORM) {
        j0 = first_lane64(j0);
        j1 = first_lane64(j1);
    }
    for (int64_t j = j0; j < j1; j++) {
        const float x = val[j];
        if (x == 0.0f) continue;
        fm_entry<G, NF>(a.V, a.W, a.d, lane, idx[j], x, vx, sq, lin);
    }
}

template <int G, int NF, bool VX>
__global__ __launch_bounds__(kBlock) void fm_rank_forward_kernel(RankFwdArgs a) {
    const int lane = threadIdx.x & (G - 1);
    const int64_t b = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / G;
    if (b >= a.nrows) return;  // whole groups leave together
    const int32_t u = a.user[b], c = a.item[b];
    const int64_t u0 = a.uptr[u], u1 = a.uptr[u + 1], um = u0 + a.ulead[u];
    const int64_t i0 = a.iptr[c], i1 = a.iptr[c + 1], im = i0 + a.ilead[c];
    // a user's rows are consecutive: most waves hold one user only
    const bool one_user = __all(u == __builtin_amdgcn_readfirstlane(u));
    float vx[NF], sq[NF];
#pragma unroll
    for (int k = 0; k < NF; k++) vx[k] = sq[k] = 0.0f;
    float lin = 0.0f;
    // BatchPredict's order (fm.go:183-206): user id, item id, user labels, item labels
    if (one_user)
        walk<G, NF, true>(a, a.uidx, a.uval, u0, um, lane, vx, sq, lin);
    else
        walk<G, NF, false>(a, a.uidx, a.uval, u0, um, lane, vx, sq, lin);
    walk<G, NF, false>(a, a.iidx, a.ival, i0, im, lane, vx, sq, lin);
    if (one_user)
        walk<G, NF, true>(a, a.uidx, a.uval, um, u1, lane, vx, sq, lin);
    else
        walk<G, NF, false>(a, a.uidx, a.uval, um, u1, lane, vx, sq, lin);
    walk<G, NF, false>(a, a.iidx, a.ival, im, i1, lane, vx, sq, lin);
    const float logit = fm_logit<G, NF>(vx, sq, lin, a.B);
    if (VX) {
#pragma unroll
        for (int k = 0; k < NF; k++) {
            const int f = lane + k * G;
            if (f < a.d) a.vx[b * a.d + f] = vx[k];
        }
    }
    if (lane == 0) a.logit[b] = logit;
}

__global__ __launch_bounds__(kBlock) void att_score_slices_kernel(AttArgs a, SliceRows rows) { att_score_body(a, rows); }
__global__ __launch_bounds__(kBlock) void att_exp_slices_kernel(AttArgs a, SliceRows rows) { att_exp_body(a, rows); }
__global__ __launch_bounds__(kBlock) void att_enc_slices_kernel(AttArgs a, SliceRows rows) { att_enc_body(a, rows); }

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

template <bool VX>
int32_t launch_rank_forward(gorse_fm *h, const RankFwdArgs &a) {
    const int G = lanes_for(h->d);
    const int64_t grid = ceil_div(a.nrows * G, kBlock);
    if (grid == 0) return GORSE_OK;
#define FM_RANK_FWD(g, nf) fm_rank_forward_kernel<g, nf, VX><<<dim3((unsigned)grid), dim3(kBlock), 0, h->s>>>(a)
    switch (G) {
        case 8: FM_RANK_FWD(8, 1); break;
        case 16: FM_RANK_FWD(16, 1); break;
        case 32: FM_RANK_FWD(32, 1); break;
        default:
            if (h->d > 64) FM_RANK_FWD(64, 2); else FM_RANK_FWD(64, 1);
    }
#undef FM_RANK_FWD
    GORSE_HIP_CHECK(hipGetLastError());
    return GORSE_OK;
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

template <typename T>
int32_t upload(DevBuf<T> &dst, const T *src, size_t n) {
    GORSE_TRY(dst.ensure(n));
    if (n) GORSE_HIP_CHECK(hipMemcpy(dst.p, src, n * sizeof(T), hipMemcpyHostToDevice));
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
        h->cat.reset();
        return GORSE_OK;
    }
    GORSE_TRY(fm::check_side(h, n_items, indptr, indices, values, lead, "items"));
    if (h->n_fields > 0) {
        if (!emb) return fail(GORSE_ERR_INVALID, "emb is NULL");
        for (int k = 0; k < h->n_fields; k++)
            if (!emb[k]) return fail(GORSE_ERR_INVALID, "emb[%d] is NULL", k);
    }
    // a catalogue larger than the device's memory is refused before anything is allocated
    const int64_t nnz = indptr[n_items];
    double bytes = (double)(n_items + 1) * 8 + (double)n_items * 4 + (double)nnz * 8;
    for (int k = 0; k < h->n_fields; k++) bytes += (double)n_items * h->fld[k].D * 2;
    size_t mem_free = 0, mem_total = 0;
    GORSE_HIP_CHECK(hipMemGetInfo(&mem_free, &mem_total));
    if (bytes > (double)mem_total)
        return fail(GORSE_ERR_NOMEM, "a catalogue of %.3g bytes does not fit the device's %zu", bytes, mem_total);
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
    GORSE_HIP_CHECK(hipStreamSynchronize(h->s));
    h->cat = std::move(c);
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
    GORSE_HIP_CHECK(hipSetDevice(h->device));

    // rows, slices (per user, batch_size rows each, the last one partial) and launch rounds (whole slices, at most R rows)
    int maxD = 0;
    for (int k = 0; k < h->n_fields; k++) maxD = std::max(maxD, h->fld[k].D);
    const int64_t row_floats = (int64_t)maxD + 2 * h->d + 2;
    int64_t R = fm::g_round_rows > 0 ? fm::g_round_rows : fm::kRoundBytes / (row_floats * (int64_t)sizeof(float));
    R = std::max<int64_t>(R, batch_size);
    const int32_t cap = fm::g_sort_cap > 0 ? fm::g_sort_cap : fm::kSortCap;
    std::vector<int32_t> desc((size_t)total * 4);
    int32_t *d_user = desc.data(), *d_item = d_user + total, *d_row0 = d_item + total, *d_len = d_row0 + total;
    std::vector<int64_t> round_begin{0};  // first row of every round, then total
    int64_t n_slices = 0, n_long = 0, max_round = 0;
    for (int64_t t = 0; t < n_users; t++) {
        const int64_t c0 = cand_indptr[t], c1 = cand_indptr[t + 1];
        if (c1 - c0 > cap) n_long++;
        for (int64_t s0 = c0; s0 < c1; s0 += batch_size) {
            const int64_t sn = std::min<int64_t>(batch_size, c1 - s0);
            if (s0 + sn - round_begin.back() > R) round_begin.push_back(s0);
            const int64_t local0 = s0 - round_begin.back();
            for (int64_t r = s0; r < s0 + sn; r++) {
                d_user[r] = (int32_t)t;
                d_item[r] = cand[r];
                d_row0[r] = (int32_t)local0;
                d_len[r] = (int32_t)sn;
            }
            n_slices++;
        }
    }
    round_begin.push_back(total);
    if (total == 0) round_begin.assign(1, 0);
    const int64_t n_rounds = (int64_t)round_begin.size() - 1;
    for (int64_t k = 0; k < n_rounds; k++) max_round = std::max(max_round, round_begin[(size_t)k + 1] - round_begin[(size_t)k]);

    // one upload of the users and the descriptors; scratch for the longest round
    std::vector<int32_t> zero_lead;
    if (!user_lead) zero_lead.assign((size_t)n_users, 0);
    GORSE_TRY(fm::upload(h->r_uptr, user_indptr, (size_t)n_users + 1));
    GORSE_TRY(fm::upload(h->r_uidx, user_indices, (size_t)user_indptr[n_users]));
    GORSE_TRY(fm::upload(h->r_uval, user_values, (size_t)user_indptr[n_users]));
    GORSE_TRY(fm::upload(h->r_ulead, user_lead ? user_lead : zero_lead.data(), (size_t)n_users));
    GORSE_TRY(fm::upload(h->r_cptr, cand_indptr, (size_t)n_users + 1));
    GORSE_TRY(fm::upload(h->r_desc, desc.data(), desc.size()));
    GORSE_TRY(h->r_scores.ensure((size_t)total));
    if (order_out) GORSE_TRY(h->r_order.ensure((size_t)total));
    if (h->n_fields > 0) {
        GORSE_TRY(h->r_vx.ensure((size_t)max_round * h->d));
        GORSE_TRY(h->r_h.ensure((size_t)max_round * h->d));
        GORSE_TRY(h->r_s.ensure((size_t)max_round * maxD));
        GORSE_TRY(h->r_rmax.ensure((size_t)max_round));
        GORSE_TRY(h->r_rsum.ensure((size_t)max_round));
    }
    for (auto &e : h->r_ev)
        if (!e) GORSE_HIP_CHECK(hipEventCreate(&e));

    const int32_t *v_user = h->r_desc.p, *v_item = v_user + total, *v_row0 = v_item + total, *v_len = v_row0 + total;
    GORSE_HIP_CHECK(hipEventRecord(h->r_ev[0], h->s));
    for (int64_t k = 0; k < n_rounds; k++) {
        if (cancel && *cancel) {
            GORSE_HIP_CHECK(hipStreamSynchronize(h->s));
            return fail(GORSE_ERR_CANCELLED, "cancelled");
        }
        const int64_t r0 = round_begin[(size_t)k], nr = round_begin[(size_t)k + 1] - r0;
        fm::RankFwdArgs f{};
        f.uptr = h->r_uptr.p, f.uidx = h->r_uidx.p, f.uval = h->r_uval.p, f.ulead = h->r_ulead.p;
        f.iptr = cat.ptr.p, f.iidx = cat.idx.p, f.ival = cat.val.p, f.ilead = cat.lead.p;
        f.user = v_user + r0, f.item = v_item + r0;
        f.V = h->V.p, f.W = h->W.p, f.B = h->B.p;
        f.nrows = nr, f.d = h->d;
        f.logit = h->r_scores.p + r0, f.vx = h->r_vx.p;
        if (h->n_fields == 0) {
            GORSE_TRY(fm::launch_rank_forward<false>(h, f));
            continue;
        }
        GORSE_TRY(fm::launch_rank_forward<true>(h, f));
        const fm::SliceRows rows{v_item + r0, v_row0 + r0, v_len + r0};
        const unsigned grid = fm::row_grid(nr);
        for (int e = 0; e < h->n_fields; e++) {
            const fm::Field &F = h->fld[e];
            fm::AttArgs a{};
            a.x = cat.emb[e].p;
            a.H = F.p.p + F.off[0], a.Wa = F.p.p + F.off[1], a.ba = F.p.p + F.off[2], a.We = F.p.p + F.off[3], a.be = F.p.p + F.off[4];
            a.nrows = nr, a.D = F.D, a.d = h->d;
            a.h = h->r_h.p, a.s = h->r_s.p, a.rmax = h->r_rmax.p, a.rsum = h->r_rsum.p;
            a.vx = h->r_vx.p, a.logit = h->r_scores.p + r0;
            fm::att_score_slices_kernel<<<dim3(grid), dim3(fm::kBlock), 0, h->s>>>(a, rows);
            fm::att_exp_slices_kernel<<<dim3(grid), dim3(fm::kBlock), 0, h->s>>>(a, rows);
            fm::att_enc_slices_kernel<<<dim3(grid), dim3(fm::kBlock), 0, h->s>>>(a, rows);
            GORSE_HIP_CHECK(hipGetLastError());
        }
    }
    if (cancel && *cancel) {
        GORSE_HIP_CHECK(hipStreamSynchronize(h->s));
        return fail(GORSE_ERR_CANCELLED, "cancelled");
    }
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
    h->rk_rows = total, h->rk_slices = n_slices, h->rk_rounds = n_rounds;
    h->rk_host_sorted = order_out ? n_long : 0;
    h->rk_ms = ms;
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
