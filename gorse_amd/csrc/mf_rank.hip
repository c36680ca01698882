// mf_rank.hip -- internalPredict (score) and Rank on the resident model, and the users' lists both Rank and Evaluate take.
// Reference: model/cf/model.go:190-203 (internalPredict), evaluator.go:162-169 (Rank), common/heap/filter.go:23-59 (TopKFilter).
// This is the literal route: one (user, item) pair per candidate, scored by mf_score_kernel, ranked one user per thread over a
// GoHeap in global memory.  mf_eval.hip and recommend.hip do the same work fused and are tested against it.
#include <algorithm>

#include "goheap.hpp"
#include "mf_internal.hpp"

using namespace gorse;

namespace {

// ---- internalPredict ---------------------------------------------------------------------
template <int NC>
__global__ __launch_bounds__(kBlock) void mf_score_kernel(const float *__restrict__ P, const float *__restrict__ Q,
                                                          const int32_t *__restrict__ us,
                                                          const int32_t *__restrict__ is, int64_t n, int d,
                                                          float *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & (kGroup - 1);
    const int gib = threadIdx.x / kGroup;
    const int64_t group = (int64_t)blockIdx.x * kGroupsPerBlock + gib;
    const int64_t ngroups = (int64_t)gridDim.x * kGroupsPerBlock;
    const VecShape vs(d);
    for (int64_t t = group; t < n; t += ngroups) {
        const int u = us[t], i = is[t];
        float r = 0.0f;
        if (u >= 0 && i >= 0) {
            const float *pu = P + (int64_t)u * d, *qi = Q + (int64_t)i * d;
            if constexpr (NC > 0) {
                float a[NC], b[NC];
#pragma unroll
                for (int c = 0; c < NC; c++) {
                    a[c] = pu[16 * c + lane];
                    b[c] = qi[16 * c + lane];
                }
                r = dot512_regs<NC>(a, b);
            } else {
                float *sa = smem + (size_t)gib * 2 * d, *sb = sa + d;
                for (int e = lane; e < d; e += kGroup) {
                    sa[e] = pu[e];
                    sb[e] = qi[e];
                }
                __builtin_amdgcn_wave_barrier();
                r = dot512_lds(sa, sb, vs, lane);
                __builtin_amdgcn_wave_barrier();
            }
        }
        if (lane == 0) out[t] = r;
    }
}

// ---- heap.TopKFilter per user over precomputed scores ------------------------------------------
__global__ void mf_rank_kernel(const int64_t *__restrict__ cand_ptr, const int32_t *__restrict__ cand,
                               const float *__restrict__ score, int64_t n_users, int topk, int32_t *heap_v,
                               float *heap_w, int32_t *__restrict__ rank_out, int32_t *__restrict__ rank_len) {
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_users) return;
    GoHeap<false> h(heap_v + t * (topk + 1), heap_w + t * (topk + 1));
    for (int64_t c = cand_ptr[t]; c < cand_ptr[t + 1]; c++) {
        h.push(cand[c], score[c]);
        if (h.n > topk) h.pop();
    }
    const int cnt = h.n;
    rank_len[t] = cnt;
    for (int k = 0; k < topk; k++) rank_out[t * topk + k] = -1;
    for (int k = cnt - 1; k >= 0; k--) {
        h.pop();  // root moved to position h.n
        rank_out[t * topk + k] = h.v[h.n];
    }
}

__global__ void expand_users_kernel(const int64_t *__restrict__ cand_ptr, const int32_t *__restrict__ users,
                                    int64_t n_users, int32_t *__restrict__ pair_u) {
    int64_t t = blockIdx.x;
    for (; t < n_users; t += gridDim.x)
        for (int64_t c = cand_ptr[t] + threadIdx.x; c < cand_ptr[t + 1]; c += blockDim.x) pair_u[c] = users[t];
}

}  // namespace

// score launcher shared with the rank path (device pointers)
int32_t gorse::mf_score_device(gorse_mf *h, const int32_t *us, const int32_t *is, int64_t n, float *out) {
    if (n == 0) return GORSE_OK;
    const int d = h->d;
    int64_t blocks = ceil_div(n, kGroupsPerBlock);
    if (blocks > 256 * 32) blocks = 256 * 32;
    const dim3 grid((unsigned)blocks), block(kBlock);
    const size_t lds = factor_row_in_registers(d) ? 0 : (size_t)kGroupsPerBlock * 2 * d * sizeof(float);
    with_factor_chunks(d, [&](auto nc) {
        mf_score_kernel<decltype(nc)::value><<<grid, block, lds, h->stream>>>(h->P.p, h->Q.p, us, is, n, d, out);
    });
    GORSE_HIP_CHECK(hipGetLastError());
    return GORSE_OK;
}

// ---- the users' lists ------------------------------------------------------------------------
int32_t gorse::upload_user_lists(gorse_mf *h, int64_t n_users, const int32_t *users, const int64_t *cand_indptr, const int32_t *cand,
                                 const int64_t *target_indptr, const int32_t *targets, UserLists *lists, int64_t *n_counted) {
    *lists = UserLists{};
    int64_t nc = 0, nt = 0, counted = 0;
    if (n_users > 0) {
        if (!users || !cand_indptr) return fail(GORSE_ERR_INVALID, "NULL argument");
        nc = cand_indptr[n_users];
        if (cand_indptr[0] != 0 || nc < 0 || (nc > 0 && !cand)) return fail(GORSE_ERR_INVALID, "bad candidate CSR");
        if (target_indptr) {
            nt = target_indptr[n_users];
            if (target_indptr[0] != 0 || nt < 0 || (nt > 0 && !targets)) return fail(GORSE_ERR_INVALID, "bad target CSR");
        }
        for (int64_t t = 0; t < n_users; t++) {
            if (users[t] < 0 || users[t] >= h->U) return fail(GORSE_ERR_RANGE, "user %d out of range", users[t]);
            if (cand_indptr[t + 1] < cand_indptr[t]) return fail(GORSE_ERR_INVALID, "cand_indptr not monotone");
            if (!target_indptr) continue;
            if (target_indptr[t + 1] < target_indptr[t]) return fail(GORSE_ERR_INVALID, "target_indptr not monotone");
            counted += target_indptr[t + 1] > target_indptr[t];
        }
        for (int64_t c = 0; c < nc; c++)
            if (cand[c] < 0 || cand[c] >= h->I) return fail(GORSE_ERR_RANGE, "candidate %d out of range", cand[c]);
    }
    if (n_counted) *n_counted = counted;
    GORSE_TRY(h->use());
    GORSE_TRY(mf_sync_streams(h));
    if (n_users == 0) return GORSE_OK;
    // their own buffer: the rank and the evaluation carve h->stage for their scratch
    Carver in;
    const size_t o_cptr = in.take((size_t)(n_users + 1) * 8), o_users = in.take((size_t)n_users * 4),
                 o_cand = in.take((size_t)std::max<int64_t>(nc, 1) * 4), o_tptr = in.take(target_indptr ? (size_t)(n_users + 1) * 8 : 0),
                 o_tgt = in.take(target_indptr ? (size_t)std::max<int64_t>(nt, 1) * 4 : 0);
    GORSE_TRY(h->rank_in.ensure(in.off));
    char *base = h->rank_in.p;
    GORSE_HIP_CHECK(hipMemcpyAsync(base + o_cptr, cand_indptr, (size_t)(n_users + 1) * 8, hipMemcpyHostToDevice, h->stream));
    GORSE_HIP_CHECK(hipMemcpyAsync(base + o_users, users, (size_t)n_users * 4, hipMemcpyHostToDevice, h->stream));
    if (nc > 0) GORSE_HIP_CHECK(hipMemcpyAsync(base + o_cand, cand, (size_t)nc * 4, hipMemcpyHostToDevice, h->stream));
    lists->n_users = n_users;
    lists->users = (const int32_t *)(base + o_users);
    lists->cand_ptr = (const int64_t *)(base + o_cptr);
    lists->cand = (const int32_t *)(base + o_cand);
    lists->n_cand = nc;
    if (target_indptr) {
        GORSE_HIP_CHECK(hipMemcpyAsync(base + o_tptr, target_indptr, (size_t)(n_users + 1) * 8, hipMemcpyHostToDevice, h->stream));
        if (nt > 0) GORSE_HIP_CHECK(hipMemcpyAsync(base + o_tgt, targets, (size_t)nt * 4, hipMemcpyHostToDevice, h->stream));
        lists->tgt_ptr = (const int64_t *)(base + o_tptr);
        lists->tgt = (const int32_t *)(base + o_tgt);
    }
    return GORSE_OK;
}

int32_t gorse::resident_user_lists(gorse_mf *h, UserLists *lists) {
    if (!h->ev_valid) return fail(GORSE_ERR_INVALID, "no resident candidate lists (gorse_mf_sample_user_negatives first)");
    *lists = UserLists{h->ev_users_n, h->ev_users.p, h->ev_cptr.p, h->ev_cand.p, h->ev_cand_n, h->ev_tptr.p, h->ev_tidx.p, true};
    return GORSE_OK;
}

// ---- Rank ------------------------------------------------------------------------------------
int32_t gorse::mf_rank_device(gorse_mf *h, const UserLists &L, int32_t topk, int32_t *rank_out, int32_t *rank_len) {
    const int64_t n_users = L.n_users, nc = L.n_cand;
    // scratch layout: pair_u | score | heap_v | heap_w | rank | len
    Carver sc;
    const size_t o_pu = sc.take((size_t)std::max<int64_t>(nc, 1) * 4), o_score = sc.take((size_t)std::max<int64_t>(nc, 1) * 4),
                 o_hv = sc.take((size_t)n_users * (topk + 1) * 4), o_hw = sc.take((size_t)n_users * (topk + 1) * 4),
                 o_rank = sc.take((size_t)n_users * topk * 4), o_len = sc.take((size_t)n_users * 4);
    GORSE_TRY(h->stage.ensure(sc.off));
    char *base = h->stage.p;
    int32_t *d_pu = (int32_t *)(base + o_pu);
    float *d_score = (float *)(base + o_score);
    int32_t *d_hv = (int32_t *)(base + o_hv);
    float *d_hw = (float *)(base + o_hw);
    int32_t *d_rank = (int32_t *)(base + o_rank), *d_len = (int32_t *)(base + o_len);
    if (nc > 0) {
        int64_t eb = n_users < 4096 ? n_users : 4096;
        expand_users_kernel<<<dim3((unsigned)eb), dim3(64), 0, h->stream>>>(L.cand_ptr, L.users, n_users, d_pu);
        GORSE_HIP_CHECK(hipGetLastError());
        GORSE_TRY(mf_score_device(h, d_pu, L.cand, nc, d_score));
    }
    mf_rank_kernel<<<dim3((unsigned)ceil_div(n_users, 64)), dim3(64), 0, h->stream>>>(L.cand_ptr, L.cand, d_score, n_users, topk, d_hv,
                                                                                     d_hw, d_rank, d_len);
    GORSE_HIP_CHECK(hipGetLastError());
    GORSE_HIP_CHECK(hipMemcpyAsync(rank_out, d_rank, (size_t)n_users * topk * 4, hipMemcpyDeviceToHost, h->stream));
    GORSE_HIP_CHECK(hipMemcpyAsync(rank_len, d_len, (size_t)n_users * 4, hipMemcpyDeviceToHost, h->stream));
    return GORSE_OK;
}

// ---- the entry points ------------------------------------------------------------------------
extern "C" int32_t gorse_mf_score(gorse_mf *h, const int32_t *u, const int32_t *items, int64_t n, float *out) {
    if (!h) return fail(GORSE_ERR_INVALID, "handle is NULL");
    if (n < 0 || (n > 0 && (!u || !items || !out))) return fail(GORSE_ERR_INVALID, "bad arguments");
    if (n == 0) return GORSE_OK;
    for (int64_t t = 0; t < n; t++)
        if (u[t] >= h->U || items[t] >= h->I)
            return fail(GORSE_ERR_RANGE, "pair %lld (%d,%d) out of range", (long long)t, u[t], items[t]);
    GORSE_TRY(h->use());
    GORSE_TRY(mf_sync_streams(h));
    size_t bytes = (size_t)n * (2 * sizeof(int32_t) + sizeof(float));
    GORSE_TRY(h->stage.ensure(bytes));
    int32_t *du = (int32_t *)h->stage.p, *di = du + n;
    float *dout = (float *)(di + n);
    GORSE_HIP_CHECK(hipMemcpyAsync(du, u, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    GORSE_HIP_CHECK(hipMemcpyAsync(di, items, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    GORSE_TRY(mf_score_device(h, du, di, n, dout));
    GORSE_HIP_CHECK(hipMemcpyAsync(out, dout, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    GORSE_HIP_CHECK(hipStreamSynchronize(h->stream));
    return GORSE_OK;
}

extern "C" int32_t gorse_mf_rank(gorse_mf *h, int64_t n_users, const int32_t *users, const int64_t *cand_indptr,
                                 const int32_t *cand, int32_t topk, int32_t *rank_out, int32_t *rank_len) {
    if (!h) return fail(GORSE_ERR_INVALID, "handle is NULL");
    if (n_users < 0 || topk <= 0) return fail(GORSE_ERR_INVALID, "n_users < 0 or topk <= 0");
    if (n_users == 0) return GORSE_OK;
    if (!rank_out || !rank_len) return fail(GORSE_ERR_INVALID, "NULL argument");
    UserLists lists;
    GORSE_TRY(upload_user_lists(h, n_users, users, cand_indptr, cand, nullptr, nullptr, &lists, nullptr));
    GORSE_TRY(mf_rank_device(h, lists, topk, rank_out, rank_len));
    GORSE_HIP_CHECK(hipStreamSynchronize(h->stream));
    return GORSE_OK;
}

extern "C" int32_t gorse_mf_rank_resident(gorse_mf *h, int32_t topk, int32_t *users_out, int32_t *rank_out, int32_t *rank_len) {
    if (!h) return fail(GORSE_ERR_INVALID, "handle is NULL");
    UserLists lists;
    GORSE_TRY(resident_user_lists(h, &lists));
    if (topk <= 0) return fail(GORSE_ERR_INVALID, "topk <= 0");
    if (lists.n_users == 0) return GORSE_OK;
    if (!rank_out || !rank_len) return fail(GORSE_ERR_INVALID, "NULL argument");
    GORSE_TRY(h->use());
    GORSE_TRY(mf_sync_streams(h));
    GORSE_TRY(mf_rank_device(h, lists, topk, rank_out, rank_len));
    if (users_out)
        GORSE_HIP_CHECK(hipMemcpyAsync(users_out, lists.users, (size_t)lists.n_users * 4, hipMemcpyDeviceToHost, h->stream));
    GORSE_HIP_CHECK(hipStreamSynchronize(h->stream));
    return GORSE_OK;
}
