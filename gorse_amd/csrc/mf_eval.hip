// mf_eval.hip -- cf.Evaluate's ranking AND metrics on the device (model/cf/evaluator.go:35-160).
// The route of mf_rank.hip (gorse_mf_rank / gorse_mf_rank_resident) writes one (user, item) pair per candidate, scores the pairs,
// ranks one user per thread over a heap in global memory and sends n_users x topK ranks to the host, which builds a set per
// user and walks the metrics.  Here one launch does all of it per user, and what crosses PCIe is six sums:
//   mf_eval_user_kernel<NC>  one 16-lane group per evaluated user (mf_score_kernel's layout and width dispatch, cf_device.hpp
//                            with_factor_chunks, so every score has gorse_mf_score's bits): p_u is loaded once, the
//                            candidates are scored a slice at a time into LDS, lane 0 pushes the slice in candidate order into the
//                            literal GoHeap<false> whose topK + 1 slots live in LDS (mf_rank_kernel's push / pop sequence, so ties
//                            fall as container/heap lets them), pops the rank list in place, the group marks the list's hits
//                            against the user's target row, and lane 0 walks the six metrics in the reference's operations and
//                            order (host/gorse_cf.hpp NDCG .. MRR) -> per_user[6][n_users], rows NDCG Precision Recall HR MAP MRR.
//   mf_eval_chain_kernel     the metrics' float32 running sums over the users IN USER ORDER (evaluator.go:60-66 with nJobs 1): one
//                            wave, the six chains side by side in six lanes, 64 users per load.  Serial by definition.
// 1 / log2f(i + 2) and the IDCG prefix sums come from two tables the host fills at run time with the libm the host mirror calls.
// No fast-math on this file: the divisions are the compiler's correctly rounded float division.
#include <algorithm>
#include <cmath>

#include "goheap.hpp"
#include "gorse_hip_test.h"
#include "mf_internal.hpp"

using namespace gorse;

namespace {

constexpr int kSlice = 64;  // candidates scored between two visits of the heap
constexpr int kAhead = 4;   // item rows a group loads before it reduces the first (register form)
constexpr int kMaxK = GORSE_MF_EVAL_MAX_TOPK;
constexpr int kMetrics = 6;

struct MfEvalArgs {
    const float *P, *Q;
    const int32_t *users;      // n_users user ids
    const int64_t *cand_ptr;   // n_users + 1
    const int32_t *cand;
    const int64_t *tgt_ptr;    // target rows: row users[t] (tgt_by_user) or row t
    const int32_t *tgt;
    const float *inv_log;      // 1 / log2f(i + 2), i < topk
    const float *idcg;         // idcg[n] = inv_log[0] + ... + inv_log[n - 1], added one after the other, n <= topk
    float *per_user;           // 6 x n_users
    int32_t *rank_out;         // n_users x topk padded with -1, or null
    int32_t *rank_len;         // n_users, or null
    int64_t n_users;
    int d, topk, tgt_by_user;
};

// floats per 16-lane group of the kernel's LDS: heap items | heap weights | slice scores | slice items | (LDS form) p_u | q_i
__host__ __device__ inline int group_floats(int topk, int d, bool lds_form) { return 2 * (topk + 1) + 2 * kSlice + (lds_form ? 2 * d : 0); }

// the group's lanes wrote LDS that other lanes of the group read next (one wave: its LDS operations complete in order)
__device__ __forceinline__ void group_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int NC>
__global__ __launch_bounds__(kBlock) void mf_eval_user_kernel(const MfEvalArgs A) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & (kGroup - 1);
    const int gib = threadIdx.x / kGroup;
    const int64_t t = (int64_t)blockIdx.x * kGroupsPerBlock + gib;
    if (t >= A.n_users) return;  // (no workgroup barrier below: a group only ever meets its own lanes)
    const int d = A.d, topk = A.topk;
    float *base = smem + (size_t)gib * group_floats(topk, d, NC == 0);
    int32_t *hv = reinterpret_cast<int32_t *>(base);
    float *hw = base + (topk + 1);
    float *sc = hw + (topk + 1);
    int32_t *ci = reinterpret_cast<int32_t *>(sc + kSlice);
    float *sa = sc + 2 * kSlice, *sb = sa + d;  // LDS form only
    const int u = A.users[t];
    const int64_t trow = A.tgt_by_user ? (int64_t)u : t;
    const int64_t t0 = A.tgt_ptr[trow];
    const int64_t nte = A.tgt_ptr[trow + 1] - t0;
    const int32_t *te = A.tgt + t0;
    if (nte <= 0) {  // evaluator.go:47: no target, no evaluation -- zeros, which the chain adds without effect
        if (lane < kMetrics) A.per_user[(int64_t)lane * A.n_users + t] = 0.0f;
        if (A.rank_out)
            for (int r = lane; r < topk; r += kGroup) A.rank_out[t * topk + r] = -1;
        if (A.rank_len && lane == 0) A.rank_len[t] = 0;
        return;
    }
    // ---- p_u, once
    const VecShape vs(d);
    const float *pu = A.P + (int64_t)(u >= 0 ? u : 0) * d;
    float a[NC > 0 ? NC : 1];
    if constexpr (NC > 0) {
#pragma unroll
        for (int c = 0; c < NC; c++) a[c] = pu[16 * c + lane];
    } else {
        for (int e = lane; e < d; e += kGroup) sa[e] = pu[e];
    }
    // ---- score a slice, feed the heap, slice after slice
    GoHeap<false> h(hv, hw);  // (lane 0's copy is the heap; the others never touch theirs)
    const int64_t c0 = A.cand_ptr[t], c1 = A.cand_ptr[t + 1];
    for (int64_t s0 = c0; s0 < c1; s0 += kSlice) {
        const int m = (int)(c1 - s0 < kSlice ? c1 - s0 : kSlice);
        for (int k = lane; k < m; k += kGroup) ci[k] = A.cand[s0 + k];
        group_sync();
        if constexpr (NC > 0) {
            // kAhead item rows on their way at a time (past the slice's end the step's first row again, not stored)
            for (int k0 = 0; k0 < m; k0 += kAhead) {
                float b[kAhead][NC];
                int it[kAhead];
#pragma unroll
                for (int j = 0; j < kAhead; j++) {
                    it[j] = ci[k0 + j < m ? k0 + j : k0];
                    const float *qi = A.Q + (int64_t)(it[j] >= 0 ? it[j] : 0) * d;
#pragma unroll
                    for (int c = 0; c < NC; c++) b[j][c] = qi[16 * c + lane];
                }
#pragma unroll
                for (int j = 0; j < kAhead; j++) {
                    const float r = dot512_regs<NC>(a, b[j]);
                    if (lane == 0 && k0 + j < m) sc[k0 + j] = (u >= 0 && it[j] >= 0) ? r : 0.0f;
                }
            }
        } else {
            for (int k = 0; k < m; k++) {
                const int i = ci[k];
                const float *qi = A.Q + (int64_t)(i >= 0 ? i : 0) * d;
                for (int e = lane; e < d; e += kGroup) sb[e] = qi[e];
                group_sync();
                const float r = dot512_lds(sa, sb, vs, lane);
                group_sync();
                if (lane == 0) sc[k] = (u >= 0 && i >= 0) ? r : 0.0f;
            }
        }
        if (lane == 0) {
            for (int k = 0; k < m; k++) {
                h.push(ci[k], sc[k]);
                if (h.n > topk) h.pop();
            }
        }
        group_sync();  // the next slice overwrites ci
    }
    // ---- the rank list, in place: every pop leaves the root just past the new end, so slot k ends up holding rank k
    int cnt = 0;
    if (lane == 0) {
        cnt = h.n;
        for (int k = cnt - 1; k >= 0; k--) h.pop();
    }
    cnt = __shfl(cnt, 0, kGroup);
    group_sync();
    // ---- hits (targetSet.Contains), the target set's cardinality
    for (int r = lane; r < cnt; r += kGroup) {
        const int32_t item = hv[r];
        hw[r] = row_has_linear(te, nte, item) ? 1.0f : 0.0f;
        if (A.rank_out) A.rank_out[t * topk + r] = item;
    }
    if (A.rank_out)
        for (int r = cnt + lane; r < topk; r += kGroup) A.rank_out[t * topk + r] = -1;
    int card = 0;
    for (int64_t k = lane; k < nte; k += kGroup) card += !row_has_linear(te, k, te[k]);
    card += __shfl_xor(card, 8, kGroup);
    card += __shfl_xor(card, 4, kGroup);
    card += __shfl_xor(card, 2, kGroup);
    card += __shfl_xor(card, 1, kGroup);
    group_sync();
    if (lane != 0) return;
    // ---- the six metrics (host/gorse_cf.hpp:517-555), float32, the reference's operations in its order
    float dcg = 0.0f, map_sum = 0.0f, mrr = 0.0f, hr = 0.0f;
    int hit = 0;
    for (int i = 0; i < cnt; i++) {
        if (hw[i] != 0.0f) {
            dcg += A.inv_log[i];
            hit++;
            map_sum += (float)hit / (float)(i + 1);
            if (hit == 1) {
                mrr = 1.0f / (float)(i + 1);
                hr = 1.0f;
            }
        }
    }
    const float idcg = A.idcg[card < cnt ? card : cnt];
    float *o = A.per_user + t;
    const int64_t n = A.n_users;
    o[0] = dcg / idcg;
    o[n] = (float)hit / (float)cnt;
    o[2 * n] = (float)hit / (float)card;
    o[3 * n] = hr;
    o[4 * n] = map_sum / (float)card;
    o[5 * n] = mrr;
    if (A.rank_len) A.rank_len[t] = cnt;
}

// sums[m] = per_user[m][0] + per_user[m][1] + ... in float32, user after user (evaluator.go:60-66 with nJobs 1): lane m of the one
// wave owns metric m's chain, so the six chains advance side by side; 64 users per load, staged through LDS so that a lane reads
// its own metric's row while the next 64 users are already on their way.  The tail's zeros add nothing: a sum is never -0.
constexpr int kChainRow = 68;  // floats per metric row in LDS: 64 + a shift of four banks per row, rows 16-byte aligned
__global__ __launch_bounds__(64) void mf_eval_chain_kernel(const float *__restrict__ pu, int64_t n, float *__restrict__ sums) {
    __shared__ __attribute__((aligned(16))) float buf[kMetrics][kChainRow];
    const int lane = threadIdx.x;
    float nx[kMetrics];
#pragma unroll
    for (int m = 0; m < kMetrics; m++) nx[m] = lane < n ? pu[(int64_t)m * n + lane] : 0.0f;
    float s = 0.0f;
    for (int64_t b = 0; b < n; b += 64) {
#pragma unroll
        for (int m = 0; m < kMetrics; m++) buf[m][lane] = nx[m];
        __syncthreads();
        const int64_t nb = b + 64 + lane;
#pragma unroll
        for (int m = 0; m < kMetrics; m++) nx[m] = nb < n ? pu[(int64_t)m * n + nb] : 0.0f;
        if (lane < kMetrics) {
#pragma unroll
            for (int j = 0; j < 64; j++) s = s + buf[lane][j];
        }
        __syncthreads();
    }
    if (lane < kMetrics) sums[lane] = s;
}

// the two tables, as the host mirror computes their entries (math32.Log2 -> log2f; evaluator.go:80-92)
void fill_tables(float *inv_log, float *idcg, int n) {
    volatile float two = 2.0f;  // (a run-time call of libm's log2f, never the compiler's own evaluation)
    idcg[0] = 0.0f;
    for (int i = 0; i < n; i++) {
        inv_log[i] = 1.0f / log2f((float)i + two);
        idcg[i + 1] = idcg[i] + inv_log[i];
    }
}

// a float32 counter that was incremented n times (count++, evaluator.go:59): it stops at 2^24
float float_count(int64_t n) { return (float)std::min<int64_t>(n, (int64_t)1 << 24); }

// Both entry points end here: lists on the device, everything validated.  n_counted = users with a target row.
int32_t evaluate_device(gorse_mf *h, const UserLists &L, int64_t n_counted, int32_t topk, float *sums, float *count, float *per_user,
                        int32_t *rank_out, int32_t *rank_len) {
    const int64_t n_users = L.n_users;
    h->mfe_users = n_counted;
    h->mfe_cands = L.n_cand;
    h->mfe_ms[0] = h->mfe_ms[1] = 0.0;
    if (n_users == 0) {
        for (int m = 0; m < kMetrics; m++) sums[m] = 0.0f;
        *count = 0.0f;
        return GORSE_OK;
    }
    if (!h->mfe_ev[2]) {
        std::vector<float> tab(2 * (size_t)kMaxK + 1);
        fill_tables(tab.data(), tab.data() + kMaxK, kMaxK);
        GORSE_TRY(h->mfe_tab.alloc(tab.size()));
        GORSE_HIP_CHECK(hipMemcpyAsync(h->mfe_tab.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, h->stream));
        GORSE_HIP_CHECK(hipStreamSynchronize(h->stream));  // tab is a host temporary
        for (auto &e : h->mfe_ev) GORSE_HIP_CHECK(hipEventCreate(&e));
    }
    // stage scratch (shared with score / rank / recommend; nothing of it outlives the call): per_user | sums | rank | len
    Carver sc;
    const size_t o_pu = sc.take((size_t)n_users * kMetrics * 4), o_sums = sc.take(kMetrics * 4),
                 o_rank = sc.take(rank_out ? (size_t)n_users * topk * 4 : 0), o_len = sc.take(rank_len ? (size_t)n_users * 4 : 0);
    GORSE_TRY(h->stage.ensure(sc.off));
    char *base = h->stage.p;
    float *d_pu = (float *)(base + o_pu), *d_sums = (float *)(base + o_sums);
    MfEvalArgs A;
    A.P = h->P.p, A.Q = h->Q.p;
    A.users = L.users, A.cand_ptr = L.cand_ptr, A.cand = L.cand, A.tgt_ptr = L.tgt_ptr, A.tgt = L.tgt;
    A.inv_log = h->mfe_tab.p, A.idcg = h->mfe_tab.p + kMaxK;
    A.per_user = d_pu;
    A.rank_out = rank_out ? (int32_t *)(base + o_rank) : nullptr;
    A.rank_len = rank_len ? (int32_t *)(base + o_len) : nullptr;
    A.n_users = n_users, A.d = h->d, A.topk = topk, A.tgt_by_user = L.tgt_by_user;
    const int d = h->d;
    const size_t lds = (size_t)kGroupsPerBlock * group_floats(topk, d, !factor_row_in_registers(d)) * sizeof(float);
    if (lds > 64 * 1024) return fail(GORSE_ERR_INVALID, "evaluate: %zu bytes of LDS for nFactors %d, topk %d", lds, d, topk);
    const dim3 grid((unsigned)ceil_div(n_users, kGroupsPerBlock));
    GORSE_HIP_CHECK(hipEventRecord(h->mfe_ev[0], h->stream));
    with_factor_chunks(d, [&](auto nc) { mf_eval_user_kernel<decltype(nc)::value><<<grid, dim3(kBlock), lds, h->stream>>>(A); });
    GORSE_HIP_CHECK(hipGetLastError());
    GORSE_HIP_CHECK(hipEventRecord(h->mfe_ev[1], h->stream));
    mf_eval_chain_kernel<<<dim3(1), dim3(64), 0, h->stream>>>(d_pu, n_users, d_sums);
    GORSE_HIP_CHECK(hipGetLastError());
    GORSE_HIP_CHECK(hipEventRecord(h->mfe_ev[2], h->stream));
    GORSE_HIP_CHECK(hipMemcpyAsync(sums, d_sums, kMetrics * 4, hipMemcpyDeviceToHost, h->stream));
    if (per_user) GORSE_HIP_CHECK(hipMemcpyAsync(per_user, d_pu, (size_t)n_users * kMetrics * 4, hipMemcpyDeviceToHost, h->stream));
    if (rank_out) GORSE_HIP_CHECK(hipMemcpyAsync(rank_out, A.rank_out, (size_t)n_users * topk * 4, hipMemcpyDeviceToHost, h->stream));
    if (rank_len) GORSE_HIP_CHECK(hipMemcpyAsync(rank_len, A.rank_len, (size_t)n_users * 4, hipMemcpyDeviceToHost, h->stream));
    GORSE_HIP_CHECK(hipStreamSynchronize(h->stream));
    *count = float_count(n_counted);
    float ms = 0.0f;
    GORSE_HIP_CHECK(hipEventElapsedTime(&ms, h->mfe_ev[0], h->mfe_ev[1]));
    h->mfe_ms[0] = ms;
    GORSE_HIP_CHECK(hipEventElapsedTime(&ms, h->mfe_ev[1], h->mfe_ev[2]));
    h->mfe_ms[1] = ms;
    return GORSE_OK;
}

int32_t check_topk(int32_t topk) {
    if (topk <= 0) return fail(GORSE_ERR_INVALID, "topk <= 0");
    if (topk > kMaxK) return fail(GORSE_ERR_INVALID, "topk %d > GORSE_MF_EVAL_MAX_TOPK (%d): rank on the device, metrics on the host", topk, kMaxK);
    return GORSE_OK;
}

}  // namespace

extern "C" int32_t gorse_mf_evaluate_resident(gorse_mf *h, int32_t topk, float *sums, float *count, float *per_user,
                                              int32_t *rank_out, int32_t *rank_len) {
    if (!h) return fail(GORSE_ERR_INVALID, "handle is NULL");
    UserLists lists;
    GORSE_TRY(resident_user_lists(h, &lists));
    GORSE_TRY(check_topk(topk));
    if (!sums || !count) return fail(GORSE_ERR_INVALID, "NULL argument");
    GORSE_TRY(h->use());
    GORSE_TRY(mf_sync_streams(h));
    return evaluate_device(h, lists, lists.n_users, topk, sums, count, per_user, rank_out, rank_len);
}

extern "C" int32_t gorse_mf_evaluate(gorse_mf *h, int64_t n_users, const int32_t *users, const int64_t *target_indptr,
                                     const int32_t *targets, const int64_t *cand_indptr, const int32_t *cand, int32_t topk,
                                     float *sums, float *count, float *per_user) {
    if (!h) return fail(GORSE_ERR_INVALID, "handle is NULL");
    if (n_users < 0) return fail(GORSE_ERR_INVALID, "n_users < 0");
    GORSE_TRY(check_topk(topk));
    if (!sums || !count) return fail(GORSE_ERR_INVALID, "NULL argument");
    if (n_users > 0 && !target_indptr) return fail(GORSE_ERR_INVALID, "NULL argument");
    UserLists lists;
    int64_t counted = 0;
    GORSE_TRY(upload_user_lists(h, n_users, users, cand_indptr, cand, target_indptr, targets, &lists, &counted));
    return evaluate_device(h, lists, counted, topk, sums, count, per_user, nullptr, nullptr);
}

extern "C" int32_t gorse_mf_evaluate_stats(gorse_mf *h, int64_t *users, int64_t *candidates, double *device_ms) {
    if (!h) return fail(GORSE_ERR_INVALID, "handle is NULL");
    if (users) *users = h->mfe_users;
    if (candidates) *candidates = h->mfe_cands;
    if (device_ms) *device_ms = h->mfe_ms[0] + h->mfe_ms[1];
    return GORSE_OK;
}

extern "C" int32_t gorse_hip_test_mf_evaluate_times(gorse_mf *h, double *ms2) {
    if (!h || !ms2) return fail(GORSE_ERR_INVALID, "NULL argument");
    ms2[0] = h->mfe_ms[0], ms2[1] = h->mfe_ms[1];
    return GORSE_OK;
}

extern "C" int32_t gorse_hip_test_mf_evaluate_tables(float *inv_log, float *idcg, int32_t n) {
    if (!inv_log || !idcg || n < 0 || n > kMaxK) return fail(GORSE_ERR_INVALID, "tables hold at most GORSE_MF_EVAL_MAX_TOPK entries");
    fill_tables(inv_log, idcg, n);
    return GORSE_OK;
}
