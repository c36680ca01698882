// recommend_mfma.hip -- gorse_mf_recommend's threshold search with the scores formed on the matrix cores (route 1).
// A second producer of exactly what rec_fast_kernel (recommend.hip) leaves behind: per (query, slice) the kk = k + 1 best candidates,
// sorted, in out_s / out_i / out_cnt, and nan_flag; rec_finish_kernel, the tie rule and the literal path follow unchanged.
//
// Scores.  The user x item score matrix is a GEMM, and the reference's _mm512_dot (cf_device.hpp dot512_regs) is, per AVX lane l, a
// product followed by an fmaf chain over the chunks 16 c + l, then group_tree16 over the 16 lane sums.  One
// v_mfma_f32_32x32x1_2b_f32 advances TWO accumulator tiles of 32 items x 32 users by one chain step each: its block 0 is AVX lane l,
// its block 1 AVX lane l + 8, with operands Q[item][16 c + l (+ 8)] and P[user][16 c + l (+ 8)].  The accumulators start at -0, so
// the first step fma(q, p, -0) is q * p in every bit (a -0 product included), and there is no padded step.  Checked on the device:
// the instruction chains as IEEE fmaf, subnormal products and sums included (tests/test_gpu_mf_recommend_matrix.py holds the bits).
// The lane tiles are then added element-wise in group_tree16's pairing -- (l, l + 8): the instruction's two blocks; (l, l + 4);
// (l, l + 2); (0, 1) -- walked depth-first (0, 4, 2, 6, 1, 5, 3, 7) so that at most three sums and one accumulator pair are live.
// Users lie on the tile's columns: a lane holds 16 scores of ONE user (user lane & 31, items 4 (lane >> 5) + (r & 3) + 8 (r >> 2))
// and that user's threshold.
//
// Work split.  A workgroup of four waves owns 128 queries (32 per wave, their factor rows stationary in registers as the B
// fragments: d / 2 registers per lane) and one item slice, whose rows of Q stream through LDS in tiles of 32 items, double-buffered:
// the next tile's global loads are issued before the current tile's MFMAs and stored to the other buffer behind them, one barrier
// per tile.  A tile row is 16 NC + 1 words apart from the next, so the 32 lanes of an A fragment read 32 different banks.
//
// Survivors.  A score passes on !(s <= thr) (thr = NaN until the first compaction).  The staging queue of a user has one slot per
// tile row: a passing score is stored at [row][user] and its bit set in the lane's own half of the user's row mask (the two lanes
// that share a user own disjoint rows, so nothing is claimed atomically and no queue can overflow: it is drained after every tile).
// After the tile's barrier each of the 16 sixteen-lane groups drains eight users: rec_candidate (a lane tests its own tile row, 16
// tests side by side), the NaN flag, the append to the (query, slice) buffer in global memory, rec_compact at cap, and the new
// threshold published in LDS.  The queues are double-buffered
// like the tiles, so the scoring of tile t + 1 runs against the drains of tile t with no second barrier: a scoring lane may read a
// threshold one drain old, which only admits more candidates.  The invariant is recommend.hip's: a score is dropped only when kk
// buffered candidates are >= it, so the result does not depend on the order in which survivors arrive.
#include "rec_internal.hpp"

using namespace gorse;

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x32 __attribute__((ext_vector_type(32)));

constexpr int kTile = 32;                // items per tile = rows of an accumulator tile
constexpr int kQueries = kRecMfmaQueries;

constexpr size_t rec_mfma_lds_bytes(int nc) {  // tiles | staged scores | row masks | thresholds | buffer counts | buffer halves
    return ((size_t)2 * kTile * (16 * nc + 1) + 2 * kTile * kQueries + 2 * 2 * kQueries + 3 * kQueries) * 4;
}

template <int NC>
__global__ __launch_bounds__(kBlock) void rec_mfma_kernel(const RecArgs A) {
    constexpr int d = 16 * NC, QS = d + 1;
    constexpr int NV = kTile * d / 4;              // float4 of a tile
    constexpr int PT = (NV + kBlock - 1) / kBlock;  // of them per thread
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *tiles = smem;                                            // [2][kTile * QS]
    float *stage = tiles + 2 * kTile * QS;                          // [2][kTile][kQueries]
    uint32_t *masks = (uint32_t *)(stage + 2 * kTile * kQueries);   // [2][kQueries][2]
    float *s_thr = (float *)(masks + 2 * 2 * kQueries);             // [kQueries]
    int *s_cnt = (int *)(s_thr + kQueries), *s_half = s_cnt + kQueries;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int col = lane & 31, hb = lane >> 5;  // the lane's user inside the wave; its block of the instruction = its half of the rows
    const int uw = wv * 32 + col;               // the lane's query inside the workgroup
    const int sl = blockIdx.y;
    const int i0 = sl * A.slice_len, i1 = min(A.I, i0 + A.slice_len);
    const int64_t qb = (int64_t)blockIdx.x * kQueries;

    auto user_of = [&](int64_t tq) { return tq < A.nq ? (A.users ? A.users[A.q0 + tq] : (int)(A.q0 + tq)) : -1; };
    const int u_lane = user_of(qb + uw);
    const bool active = u_lane >= 0;
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
    auto gload = [&](int t0) {  // rows past the slice's end are zeros (scored, never staged)
#pragma unroll
        for (int e = 0; e < PT; e++) {
            const int x = tid + kBlock * e, row = x / (4 * NC), c4 = x % (4 * NC);
            rq[e] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (x < NV && t0 + row < i1) rq[e] = *(const float4 *)(A.Q + (int64_t)(t0 + row) * d + 4 * c4);
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
    // AVX lanes l and l + 8 of every pair of the tile: the chain over the chunks, then the tree's first step.  The A operands of the
    // NEXT lane pair are fetched from LDS before the current pair's chain is issued, and a scheduling barrier after every chain keeps
    // the compiler from running the eight independent chains side by side (256 accumulator registers instead of 32).
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

    if (tid < kQueries) {
        s_thr[tid] = __int_as_float(0x7fc00000);  // NaN: !(s <= thr) holds for every s until the first compaction
        s_cnt[tid] = 0;
        s_half[tid] = 0;
    }
    gload(i0);
    lstore(0);
    __syncthreads();

    const int grp = tid / kGroup, gl = tid & (kGroup - 1);  // the drains' split: group grp owns queries 8 grp .. 8 grp + 7
    const int cap = A.cap, kk = A.kk;
    int p = 0;
    for (int t0 = i0; t0 < i1; t0 += kTile, p ^= 1) {
        const bool more = t0 + kTile < i1;
        if (more) gload(t0 + kTile);
        {   // ---- score the tile, stage what passes
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
            const float thr = s_thr[uw];
            const int nt = min(kTile, i1 - t0);
            float *st = stage + p * kTile * kQueries + uw;
            uint32_t m = 0;
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * hb;
                if (active && row < nt && !(s[r] <= thr)) {
                    st[row * kQueries] = s[r];
                    m |= 1u << r;
                }
            }
            masks[(p * kQueries + uw) * 2 + hb] = m;
        }
        if (more) lstore(p ^ 1);
        __syncthreads();
        // ---- drain: the group's eight users, one after the other; everything below is uniform inside the group
        for (int x = 0; x < 8; x++) {
            const int q = 8 * grp + x;
            const uint32_t m0 = masks[(p * kQueries + q) * 2], m1 = masks[(p * kQueries + q) * 2 + 1];
            if ((m0 | m1) == 0) continue;
            const int64_t tq = qb + q;
            const int u = user_of(tq);
            const int32_t *trow = A.uidx_sorted + A.uptr[u], *srow = nullptr;
            const int64_t tn = A.uptr[u + 1] - A.uptr[u];
            int64_t sn = 0;
            if (A.sptr) {
                srow = A.seen + A.sptr[A.q0 + tq];
                sn = A.sptr[A.q0 + tq + 1] - A.sptr[A.q0 + tq];
            }
            const int64_t slot = tq * A.slices + sl;
            float *bs = A.buf_s + slot * 2 * cap;
            int32_t *bi = A.buf_i + slot * 2 * cap;
            int cnt = s_cnt[q], half = s_half[q];
            float thr = s_thr[q];
            const float *st = stage + p * kTile * kQueries + q;
            // a lane tests its own tile row (two rounds of 16 rows), so sixteen candidate tests run side by side; the rows that
            // pass are then appended one after the other, uniformly in the group
            for (int h2 = 0; h2 < 2; h2++) {
                const int row = gl + 16 * h2, r = (row & 3) | ((row >> 3) << 2);  // (the row's lane half is bit 2, its register r)
                const bool staged = ((((row >> 2) & 1) ? m1 : m0) >> r) & 1u;
                const float s = staged ? st[row * kQueries] : 0.0f;
                // (s <= thr: the threshold may have risen since the score was staged)
                bool pass = staged && !(s <= thr) && rec_candidate(A.item_ok, trow, tn, srow, sn, t0 + row);
                if (pass && s != s) {
                    atomicOr(&A.nan_flag[tq], 1);
                    pass = false;
                }
                for (uint32_t todo = (uint32_t)(__ballot(pass) >> (kGroup * (grp & 3))) & 0xffffu; todo != 0; todo &= todo - 1) {
                    const int e = __ffs(todo) - 1;
                    const float se = __shfl(s, e, kGroup);
                    if (se <= thr) continue;
                    float *cs = bs + half * cap;
                    int32_t *ci = bi + half * cap;
                    if (gl == 0) {
                        cs[cnt] = se;
                        ci[cnt] = t0 + e + 16 * h2;
                    }
                    cnt++;
                    if (cnt == cap) {
                        __threadfence_block();
                        thr = rec_compact(cs, ci, cnt, bs + (half ^ 1) * cap, bi + (half ^ 1) * cap, kk, gl);
                        __threadfence_block();
                        half ^= 1;
                        cnt = kk;
                    }
                }
            }
            if (gl == 0) {
                s_cnt[q] = cnt;
                s_half[q] = half;
                s_thr[q] = thr;
            }
        }
    }
    // ---- the slice's kk best of every query, sorted (the group that appended them has them in view)
    for (int x = 0; x < 8; x++) {
        const int q = 8 * grp + x;
        const int64_t tq = qb + q;
        if (tq >= A.nq) break;
        const int64_t slot = tq * A.slices + sl;
        const int cnt = s_cnt[q], half = s_half[q];
        if (cnt > 0) {
            __threadfence_block();
            (void)rec_compact(A.buf_s + (slot * 2 + half) * cap, A.buf_i + (slot * 2 + half) * cap, cnt, A.out_s + slot * kk, A.out_i + slot * kk, kk, gl);
        }
        if (gl == 0) A.out_cnt[slot] = min(cnt, kk);
    }
}

template <int NC>
int32_t launch(const RecArgs &A, hipStream_t stream) {
    constexpr size_t lds = rec_mfma_lds_bytes(NC);
    GORSE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&rec_mfma_kernel<NC>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const dim3 grid((unsigned)ceil_div(A.nq, (int64_t)kQueries), (unsigned)A.slices);
    rec_mfma_kernel<NC><<<grid, dim3(kBlock), lds, stream>>>(A);
    GORSE_HIP_CHECK(hipGetLastError());
    return GORSE_OK;
}

}  // namespace

namespace gorse {

int32_t rec_mfma_launch(const RecArgs &A, hipStream_t stream) {
    if (!rec_mfma_serves(A.d)) return fail(GORSE_ERR_INVALID, "the matrix route does not serve nFactors %d", A.d);
    switch (A.d / 16) {
#define GORSE_REC_NC(n) \
    case n: return launch<n>(A, stream);
        GORSE_REC_NC(1) GORSE_REC_NC(2) GORSE_REC_NC(3) GORSE_REC_NC(4) GORSE_REC_NC(5) GORSE_REC_NC(6) GORSE_REC_NC(7) GORSE_REC_NC(8)
        GORSE_REC_NC(9) GORSE_REC_NC(10) GORSE_REC_NC(11) GORSE_REC_NC(12) GORSE_REC_NC(13) GORSE_REC_NC(14) GORSE_REC_NC(15)
#undef GORSE_REC_NC
        default: return launch<16>(A, stream);
    }
}

}  // namespace gorse
