// recommend_sweep.hip -- gorse_mf_recommend's pilot-threshold schedule (gorse_mf_set_recommend_schedule(h, 1)).
// Schedule 0 (recommend.hip) learns a query's threshold while it walks the items: every item slice starts at -inf, a passing score
// costs binary searches and an append, a full buffer a compaction.  Here the threshold is known BEFORE the catalogue is swept:
//
//   1. Pilot (rec_sweep_score_kernel<NC, true> + rec_pilot_select_kernel).  Every stride-th item is scored for every query on the
//      matrix cores, in the reference's bits; one workgroup per query then drops the sampled items that are no candidates (item_ok by
//      a load, the training and seen rows by WALKING them: an entry that is a multiple of the stride clears its sample slot, no
//      search) and selects the kk-th best of the rest, kk = k + 1, by a four-pass radix select over the keys in LDS: tau.
//      Safe by construction: the sample's kk candidates at or above tau are candidates of the whole catalogue, so every score below
//      tau has kk candidates at or above it -- schedule 0's invariant.  A sample with fewer than kk candidates, or with a NaN
//      candidate, hands its query back.
//   2. Sweep (rec_sweep_score_kernel<NC, false>).  The same kernel over all items: a lane compares its 16 scores with its user's tau
//      and appends (item, score) of what is >= tau, or NaN, to the user's survivor list in global memory (count by atomic add, entries
//      by plain stores).  No exclusion here; about kk * stride survivors per query.  A count beyond the list's capacity hands the
//      query back.  The item slices of the grid share tau and the lists: nothing restarts.
//   3. Finish (rec_sweep_finish_kernel).  One workgroup per query: the survivors that are candidates (rec_candidate's searches, on
//      survivors only) ranked in LDS, the kk best kept, rec_finish_kernel's tie rule and result arrays.
// Handed-back queries are answered by schedule 0's rec_fast_kernel in a second launch (recommend.hip).
//
// Scores: recommend_mfma.hip's scheme.  One v_mfma_f32_32x32x1_2b_f32 advances the accumulator tiles of AVX lanes l and l + 8 by one
// fmaf step of the reference's chain over the chunks; the accumulators start at -0; the eight lane-pair tiles are added in
// group_tree16's pairing.  A lane holds 16 scores of ONE user (user lane & 31 of its wave, tile rows 4 (lane >> 5) + (r & 3) +
// 8 (r >> 2)), so the compare with tau is per lane and a pilot lane stores four runs of four consecutive sample slots.
// Work split: a workgroup of four waves keeps 128 users' factor rows stationary in registers (d / 2 per lane) and streams its item
// slice through LDS in tiles of 32 rows, double-buffered, one barrier per tile; a tile row is d + 1 words apart from the next.
#include "rec_internal.hpp"
#include "rec_sweep_plan.hpp"

using namespace gorse;
namespace rs = gorse::recsweep;

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x32 __attribute__((ext_vector_type(32)));

constexpr int kTile = rs::kTile;
constexpr int kQueries = rs::kQueries;
static_assert(kBlock == rs::kBlockThreads && kQueries == kRecMfmaQueries, "the plan is written for this workgroup");

__device__ __forceinline__ int sweep_user(const RecArgs &A, int64_t tq) {
    return tq < A.nq ? (A.users ? A.users[A.q0 + tq] : (int)(A.q0 + tq)) : -1;
}

// PILOT: virtual item j is item j * stride, its score goes to samp[query][j].  Otherwise: item j, compared with tau and appended.
template <int NC, bool PILOT>
__global__ __launch_bounds__(kBlock) void rec_sweep_score_kernel(const RecSweepArgs S) {
    constexpr int d = 16 * NC, QS = d + 1;
    constexpr int NV = kTile * d / 4;               // float4 of a tile
    constexpr int PT = (NV + kBlock - 1) / kBlock;  // of them per thread
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *tiles = smem;  // [2][kTile * QS]
    const RecArgs &A = S.R;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int col = lane & 31, hb = lane >> 5;  // the lane's user inside the wave; its block of the instruction = its half of the rows
    const int n = PILOT ? S.n_sample : A.I, stride = PILOT ? S.stride : 1;
    const int slice_len = PILOT ? S.pilot_slice_len : S.sweep_slice_len;
    const int i0 = blockIdx.y * slice_len, i1 = min(n, i0 + slice_len);
    if (i0 >= i1) return;
    const int64_t tq = (int64_t)blockIdx.x * kQueries + wv * 32 + col;
    const int u_lane = sweep_user(A, tq);
    const bool active = u_lane >= 0 && (PILOT || S.hb[tq] == 0);
    const float tau = (!PILOT && active) ? S.tau[tq] : 0.0f;

    float pf[8 * NC];  // pf[8 c + l] = P[u][16 c + l + 8 hb]
#pragma unroll
    for (int c = 0; c < NC; c++) {
        float4 lo = make_float4(0.f, 0.f, 0.f, 0.f), hi = lo;
        if (active) {
            const float4 *src = (const float4 *)(A.P + (int64_t)u_lane * d + 16 * c + 8 * hb);
            lo = src[0], hi = src[1];
        }
        pf[8 * c + 0] = lo.x, pf[8 * c + 1] = lo.y, pf[8 * c + 2] = lo.z, pf[8 * c + 3] = lo.w;
        pf[8 * c + 4] = hi.x, pf[8 * c + 5] = hi.y, pf[8 * c + 6] = hi.z, pf[8 * c + 7] = hi.w;
    }

    float4 rq[PT];
    auto gload = [&](int t0) {  // rows past the slice's end are zeros (scored, never kept)
#pragma unroll
        for (int e = 0; e < PT; e++) {
            const int x = tid + kBlock * e, row = x / (4 * NC), c4 = x % (4 * NC);
            rq[e] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (x < NV && t0 + row < i1) rq[e] = *(const float4 *)(A.Q + (int64_t)(t0 + row) * stride * d + 4 * c4);
        }
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int e = 0; e < PT; e++) {
            const int x = tid + kBlock * e, row = x / (4 * NC), c4 = x % (4 * NC);
            if (x < NV) {
                float *dst = tiles + buf * kTile * QS + row * QS + 4 * c4;
                dst[0] = rq[e].x, dst[1] = rq[e].y, dst[2] = rq[e].z, dst[3] = rq[e].w;
            }
        }
    };
    // AVX lanes l and l + 8 of the tile: the chain over the chunks, then the tree's first step.  The next lane pair's A operands are
    // fetched before the current chain is issued; the scheduling barrier keeps the eight chains from running side by side
    auto fetch = [&](float (&qa)[NC], const float *qrow, int l) {
#pragma unroll
        for (int c = 0; c < NC; c++) qa[c] = qrow[16 * c + l];
    };
    auto chain = [&](const float (&qa)[NC], int l) {
        f32x32 acc;
#pragma unroll
        for (int r = 0; r < 32; r++) acc[r] = -0.0f;
#pragma unroll
        for (int c = 0; c < NC; c++) acc = __builtin_amdgcn_mfma_f32_32x32x1f32(qa[c], pf[8 * c + l], acc, 0, 0, 0);
        f32x16 t;
#pragma unroll
        for (int r = 0; r < 16; r++) t[r] = acc[r] + acc[16 + r];
        __builtin_amdgcn_sched_barrier(0);
        return t;
    };

    gload(i0);
    lstore(0);
    __syncthreads();
    int p = 0;
    for (int t0 = i0; t0 < i1; t0 += kTile, p ^= 1) {
        const bool more = t0 + kTile < i1;
        if (more) gload(t0 + kTile);
        const float *qrow = tiles + p * kTile * QS + col * QS + 8 * hb;  // (the A fragment's row is the lane's ITEM lane & 31)
        float qa[NC], qn[NC];
        fetch(qa, qrow, 0);
        fetch(qn, qrow, 4);
        f32x16 t = chain(qa, 0);
        fetch(qa, qrow, 2);
        f32x16 s = t + chain(qn, 4);
        fetch(qn, qrow, 6);
        t = chain(qa, 2);
        fetch(qa, qrow, 1);
        s = s + (t + chain(qn, 6));
        fetch(qn, qrow, 5);
        t = chain(qa, 1);
        fetch(qa, qrow, 3);
        f32x16 o = t + chain(qn, 5);
        fetch(qn, qrow, 7);
        t = chain(qa, 3);
        o = o + (t + chain(qn, 7));
        s = s + o;
        if constexpr (PILOT) {
            // slots t0 .. t0 + 31 of the query's row exist: t0 is a multiple of the tile and the row is padded to whole tiles
            // and every lane stores, a query past the round's end or without a user too (samp has whole blocks of rows): a store under
            // `active` would let the compiler sink the tree's sums into that branch, behind all eight chains, 256 accumulators live
            float *dst = S.samp + tq * S.samp_ld + t0 + 4 * hb;
#pragma unroll
            for (int g = 0; g < 4; g++) *(float4 *)(dst + 8 * g) = make_float4(s[4 * g], s[4 * g + 1], s[4 * g + 2], s[4 * g + 3]);
        } else {
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int item = t0 + (r & 3) + 8 * (r >> 2) + 4 * hb;
                if (active && item < i1 && !(s[r] < tau)) {  // >= tau, or NaN
                    const int pos = atomicAdd(&S.cnt[tq], 1);
                    if (pos < S.cap) {
                        S.surv_i[tq * S.cap + pos] = item;
                        S.surv_s[tq * S.cap + pos] = s[r];
                    }
                }
            }
        }
        if (more) lstore(p ^ 1);
        __syncthreads();
    }
}

// One workgroup per query: tau = the kk-th best sampled candidate score, or the query handed back.
__global__ __launch_bounds__(kBlock) void rec_pilot_select_kernel(const RecSweepArgs S) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    uint32_t *keys = (uint32_t *)smem;  // [n_sample]
    int *hist = (int *)(keys + S.n_sample);  // [256]
    __shared__ int s_valid, s_nan, s_bin, s_rem;
    const RecArgs &A = S.R;
    const int64_t tq = blockIdx.x;
    const int tid = threadIdx.x, n = S.n_sample, stride = S.stride;
    const int u = sweep_user(A, tq);
    if (u < 0) {  // no answer needed: the sweep skips the query, the finish writes its empty row
        if (tid == 0) S.tau[tq] = INFINITY, S.hb[tq] = 0;
        return;
    }
    if (tid == 0) s_valid = 0, s_nan = 0;
    const float *row = S.samp + tq * S.samp_ld;
    for (int j = tid; j < n; j += kBlock) {
        const float s = row[j];
        keys[j] = A.item_ok[j * stride] == 0 ? 0u : (s != s ? rs::kKeyNaN : rs::score_key(__float_as_uint(s)));
    }
    __syncthreads();
    {   // the training and seen rows: an entry on the sample's grid clears its slot
        const int32_t *trow = A.uidx_sorted + A.uptr[u];
        const int64_t tn = A.uptr[u + 1] - A.uptr[u];
        for (int64_t e = tid; e < tn; e += kBlock)
            if (trow[e] % stride == 0) keys[trow[e] / stride] = 0u;
        if (A.sptr) {
            const int32_t *srow = A.seen + A.sptr[A.q0 + tq];
            const int64_t sn = A.sptr[A.q0 + tq + 1] - A.sptr[A.q0 + tq];
            for (int64_t e = tid; e < sn; e += kBlock)
                if (srow[e] % stride == 0) keys[srow[e] / stride] = 0u;
        }
    }
    __syncthreads();
    int valid = 0, nan = 0;
    for (int j = tid; j < n; j += kBlock) {
        valid += keys[j] != 0u;
        nan |= keys[j] == rs::kKeyNaN;
    }
    if (valid) atomicAdd(&s_valid, valid);
    if (nan) atomicOr(&s_nan, 1);
    __syncthreads();
    if (s_nan || s_valid < A.kk) {
        if (tid == 0) S.tau[tq] = INFINITY, S.hb[tq] = 1;
        return;
    }
    // the kk-th largest key, a byte per pass from the top: the histogram of the keys that share the bytes found so far
    uint32_t prefix = 0, mask = 0;
    int rem = A.kk;
    for (int shift = 24; shift >= 0; shift -= 8) {
        hist[tid] = 0;
        __syncthreads();
        for (int j = tid; j < n; j += kBlock)
            if ((keys[j] & mask) == prefix) atomicAdd(&hist[(keys[j] >> shift) & 255u], 1);
        __syncthreads();
        if (tid == 0) {
            int above = 0, b = 255;
            for (; b > 0 && above + hist[b] < rem; b--) above += hist[b];
            s_bin = b;
            s_rem = rem - above;
        }
        __syncthreads();
        prefix |= (uint32_t)s_bin << shift;
        mask |= 255u << shift;
        rem = s_rem;
        __syncthreads();
    }
    if (tid == 0) S.tau[tq] = __uint_as_float(rs::key_score_bits(prefix)), S.hb[tq] = 0;
}

// One workgroup per query: the survivors that are candidates, the kk best of them ranked, rec_finish_kernel's tie rule and outputs.
__global__ __launch_bounds__(kBlock) void rec_sweep_finish_kernel(const RecSweepArgs S, int32_t *__restrict__ res_items,
                                                                  float *__restrict__ res_scores, int32_t *__restrict__ res_cnt,
                                                                  int32_t *__restrict__ lit) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const RecArgs &A = S.R;
    const int kk = A.kk, k = A.k, cap = S.cap;
    float *es = smem;
    int32_t *ei = (int32_t *)(smem + cap);
    float *ts = smem + 2 * (size_t)cap;
    int32_t *ti = (int32_t *)(ts + kk);
    __shared__ int s_n, s_tie, s_back;
    const int64_t tq = blockIdx.x;
    const int tid = threadIdx.x;
    if (tid == 0) s_n = 0, s_tie = 0, s_back = S.hb[tq] != 0 || S.cnt[tq] > cap;
    __syncthreads();
    const int u = sweep_user(A, tq);
    if (!s_back) {
        const int c = S.cnt[tq];  // (0 for u < 0: the sweep skipped it)
        const int32_t *trow = nullptr, *srow = nullptr;
        int64_t tn = 0, sn = 0;
        if (u >= 0) {
            trow = A.uidx_sorted + A.uptr[u];
            tn = A.uptr[u + 1] - A.uptr[u];
            if (A.sptr) {
                srow = A.seen + A.sptr[A.q0 + tq];
                sn = A.sptr[A.q0 + tq + 1] - A.sptr[A.q0 + tq];
            }
        }
        for (int e = tid; e < c; e += kBlock) {
            const int32_t item = S.surv_i[tq * cap + e];
            const float s = S.surv_s[tq * cap + e];
            if (!rec_candidate(A.item_ok, trow, tn, srow, sn, item)) continue;
            if (s != s) {
                atomicOr(&s_tie, 1);
            } else {
                const int pos = atomicAdd(&s_n, 1);
                es[pos] = s;
                ei[pos] = item;
            }
        }
        __syncthreads();
        // (the pilot's kk candidates are among them; fewer would mean a list the sweep did not complete)
        if (tid == 0 && u >= 0 && s_n < kk && !s_tie) s_back = 1;
        __syncthreads();
    }
    if (s_back) {  // schedule 0 answers it and writes its row
        if (tid == 0) S.hb[tq] = 1, lit[tq] = 0, res_cnt[tq] = 0;
        return;
    }
    const int n = s_n, m = min(n, kk);
    for (int e = tid; e < n; e += kBlock) {
        const float s = es[e];
        int rank = 0;
        for (int j = 0; j < n; j++) {
            const float o = es[j];
            rank += (o > s || (o == s && j < e)) ? 1 : 0;
        }
        if (rank < m) {
            ts[rank] = s;
            ti[rank] = ei[e];
        }
    }
    __syncthreads();
    for (int r = tid; r + 1 < m; r += kBlock)
        if (ts[r] == ts[r + 1]) atomicOr(&s_tie, 1);
    __syncthreads();
    const int tie = s_tie;
    const int cntk = tie ? 0 : min(n, k);
    if (tid == 0) {
        lit[tq] = tie;
        res_cnt[tq] = cntk;
    }
    for (int r = tid; r < k; r += kBlock) {
        res_items[tq * k + r] = r < cntk ? ti[r] : -1;
        res_scores[tq * k + r] = r < cntk ? ts[r] : 0.0f;
    }
}

__global__ __launch_bounds__(kBlock) void rec_sweep_clear_kernel(int32_t *cnt, int64_t n) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t < n) cnt[t] = 0;
}

template <int NC>
int32_t launch(const RecSweepArgs &S, int32_t *res_items, float *res_scores, int32_t *res_cnt, int32_t *lit, hipStream_t stream) {
    constexpr size_t lds = (size_t)2 * kTile * (16 * NC + 1) * 4;
    const int64_t nq = S.R.nq;
    const unsigned blocks = (unsigned)ceil_div(nq, (int64_t)kQueries);
    GORSE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&rec_sweep_score_kernel<NC, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    GORSE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&rec_sweep_score_kernel<NC, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    GORSE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&rec_pilot_select_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)S.select_lds));
    GORSE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&rec_sweep_finish_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)S.finish_lds));
    rec_sweep_clear_kernel<<<dim3((unsigned)ceil_div(nq, (int64_t)kBlock)), dim3(kBlock), 0, stream>>>(S.cnt, nq);
    rec_sweep_score_kernel<NC, true><<<dim3(blocks, (unsigned)S.pilot_slices), dim3(kBlock), lds, stream>>>(S);
    rec_pilot_select_kernel<<<dim3((unsigned)nq), dim3(kBlock), S.select_lds, stream>>>(S);
    rec_sweep_score_kernel<NC, false><<<dim3(blocks, (unsigned)S.sweep_slices), dim3(kBlock), lds, stream>>>(S);
    rec_sweep_finish_kernel<<<dim3((unsigned)nq), dim3(kBlock), S.finish_lds, stream>>>(S, res_items, res_scores, res_cnt, lit);
    GORSE_HIP_CHECK(hipGetLastError());
    return GORSE_OK;
}

}  // namespace

namespace gorse {

int32_t rec_sweep_launch(const RecSweepArgs &S, int32_t *res_items, float *res_scores, int32_t *res_cnt, int32_t *lit, hipStream_t stream) {
    if (!rs::serves(S.R.d, S.R.k)) return fail(GORSE_ERR_INVALID, "the pilot schedule does not serve nFactors %d, k %d", S.R.d, S.R.k);
    if (S.select_lds > (size_t)rs::kLdsBytes || S.finish_lds > (size_t)rs::kLdsBytes) return fail(GORSE_ERR_INVALID, "pilot plan beyond LDS");
    switch (S.R.d / 16) {
#define GORSE_REC_NC(n) \
    case n: return launch<n>(S, res_items, res_scores, res_cnt, lit, stream);
        GORSE_REC_NC(1) GORSE_REC_NC(2) GORSE_REC_NC(3) GORSE_REC_NC(4) GORSE_REC_NC(5) GORSE_REC_NC(6) GORSE_REC_NC(7) GORSE_REC_NC(8)
        GORSE_REC_NC(9) GORSE_REC_NC(10) GORSE_REC_NC(11) GORSE_REC_NC(12) GORSE_REC_NC(13) GORSE_REC_NC(14) GORSE_REC_NC(15)
#undef GORSE_REC_NC
        default: return launch<16>(S, res_items, res_scores, res_cnt, lit, stream);
    }
}

}  // namespace gorse
