// topk_deep.hip -- the DEEP form of path B's candidate sweep (topk_mfma.hip says what the path is and why it is exact): operands of
// 25 k-steps and more, which the register-resident sweep of topk_sweep.hip cannot hold (gorse_topk_set_deep_sweep).
//
// A GEMM-shaped kernel with a K-loop.  A workgroup of four waves owns 256 queries and walks the row tiles (128 rows); per tile it
// runs over the operand depth in K-slices of 64 bf16 values.  Both operands of a slice -- 128 row pieces and the block's 256 query
// pieces, 128 bytes each -- come into LDS by LDS-DMA (global_load_lds_dwordx4, 16-byte pieces XOR-swizzled by row on the source
// address and again on the read: ds_read_b128 is conflict-free); three slices are resident, so two are in flight behind the one
// being multiplied, across tile boundaries too.  The waves divide the QUERIES: a wave multiplies all 128 rows with its own 64
// queries, eight 32 x 32 blocks of v_mfma_f32_32x32x16_bf16 whose 128 accumulators per lane live in registers for the whole K-loop.
// A query's candidate list has therefore exactly one writer, as in topk_sweep_kernel, and compact_query (topk_compact.hpp) is that
// kernel's.  What the kernel leaves is the main sweep's non-symmetric, non-history contract: thresholds from f0 or -inf, margins
// from qmargin, (key, row) entries in two interleaved sub-lists of cbuf, ccnt / cflag / f_out at the end, tile_stride for the pilots,
// the per-row value of rscale (NaN: a masked row or a row past N) applied to every score.
//
// One barrier per slice: slice g is waited for (s_waitcnt vmcnt(kDmaPerSlice): everything but the slice behind it has landed;
// vector memory loads return in order), the barrier follows, and only then slice g + 2 is issued into the buffer slice g - 1 was
// read from -- every wave is past its reads of g - 1 when it reaches the barrier.  The DMA and its waits are inline assembly: a load
// or DMA builtin hipcc can see inside the loop makes it drain the memory counter in every iteration (topk_sweep.hip).  Accumulators
// are read only by instructions the compiler emits (it knows the MFMA's wait states; an asm statement gets none).
//
// Exactness.  topk_mfma_prepare's error coefficient bounds two summation orders of the same K' exact products (a bf16 x bf16
// product is exact in fp32): the reference's fp32 chain (gamma <= K' u) and the matrix core's (gamma <= 2 K' u, allowing
// truncating adders).  Nothing in that bound depends on HOW the K' products are grouped: any summation of K' terms, in any order
// and with a rounding (or truncation, 2 u) after every addition, has every term pass through at most K' - 1 additions, so its
// forward error is at most gamma'(K' - 1) sum |a_i b_i| <= 2 K' u |q| |x| to first order (Higham, Accuracy and Stability of
// Numerical Algorithms, 4.2; Cauchy-Schwarz).  An accumulation that spans K' / 16 chained MFMA instructions -- the accumulator
// rounded once per instruction or once per product -- is one such order.  The second-order factor 1 / (1 - 2 K' u) is 1.0006 at
// K' = 4608 and inside the 1.01 the coefficient is multiplied by; the zero padding adds exact zeros.  The coefficient is computed
// from the true d as for the shallow form; it needed no widening.
#include "topk_compact.hpp"
#include "topk_deep_plan.hpp"
#include "topk_mfma_internal.hpp"

using namespace gorse;
using namespace gorse::topk_deep_plan;

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float max3f(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }

// BIAS: the row value is added to the score (Euclidean), else multiplied (cosine's scale; 1 for -dot, where only its NaN matters)
template <bool BIAS>
__global__ __launch_bounds__(kThreads) void topk_deep_sweep_kernel(SweepParams p, int kpad) {
    constexpr int RB = kRows / 32, NCB = kQueriesPerWave / 32;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char *s_slice = smem;  // kBufs x (kRows + kQueries) pieces of 128 bytes: the A rows, then the B rows
    float *s_rs = reinterpret_cast<float *>(smem + kBufs * kSliceBytes);  // the row values of tile t at (t & 1) * kRows
    int *s_cnt = reinterpret_cast<int *>(s_rs + 2 * kRows);               // 2 per query: the interleaved sub-list lengths
    float *s_f = reinterpret_cast<float *>(s_cnt + 2 * kQueries);
    float *s_mg = s_f + kQueries;

    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t wgq0 = (int64_t)blockIdx.x * kQueries;
    for (int t = tid; t < kQueries; t += kThreads) {
        const int64_t q = wgq0 + t;
        s_cnt[2 * t] = 0;
        s_cnt[2 * t + 1] = 0;
        s_f[t] = q < p.nq ? (p.f0 ? p.f0[q] : -__builtin_inff()) : __builtin_inff();  // a query past nq collects nothing
        s_mg[t] = q < p.nq ? p.qmargin[q] : 0.0f;
    }
    const int S = kpad / kSlice;                                         // K-slices per tile
    const int64_t stride_rows = (int64_t)p.tile_stride * kRows;          // a pilot samples every tile_stride-th tile
    const int64_t NT = (p.N + stride_rows - 1) / stride_rows;
    const int64_t total = NT * S;                                        // slices this workgroup multiplies
    const unsigned row_bytes = (unsigned)kpad * 2u;

    // Piece c (16 bytes) of row r lives at piece c ^ swz(r) of the row's 128-byte LDS image: the 16 lanes of a ds_read_b128 group read
    // one piece column of 16 consecutive rows -- two rows per 256-byte bank row -- and the XOR spreads them over its 16 slots.
    auto swz = [](int row) -> int { return (row >> 1) & 7; };
    // DMA instruction i of this wave: 64 pieces = 8 consecutive rows of the slice's LDS image.  The lane's source offset from the
    // tile's (A) or the query block's (B) first byte of the slice is a 32-bit register computed once; the base is a 64-bit scalar.
    unsigned offA[kDmaA], offB[kDmaB];
#pragma unroll
    for (int i = 0; i < kDmaA; i++) {
        const int row = (w * kDmaA + i) * 8 + (lane >> 3), cs = lane & 7;
        offA[i] = (unsigned)row * row_bytes + (unsigned)((cs ^ swz(row)) << 4);
    }
#pragma unroll
    for (int i = 0; i < kDmaB; i++) {
        const int row = (w * kDmaB + i) * 8 + (lane >> 3), cs = lane & 7;  // = the query's place in the block
        int64_t q = wgq0 + row;
        if (q >= p.nq) q = p.nq - 1;  // clamped: its threshold is +inf
        offB[i] = (unsigned)(q - wgq0) * row_bytes + (unsigned)((cs ^ swz(row)) << 4);
    }
    const unsigned lds_slice = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)s_slice;
    const unsigned lds_rs = (unsigned)(uintptr_t)(__attribute__((address_space(3))) float *)s_rs;
    const unsigned char *Bblock = reinterpret_cast<const unsigned char *>(p.B) + wgq0 * (int64_t)row_bytes;

    // the next slice to issue: tile it, slice is of it, into buffer ibuf
    int64_t it = 0;
    int is = 0, ibuf = 0;
    auto issue = [&]() {
        const int64_t base_row = it * stride_rows;
        unsigned keep;
        // the tile's row values ride in front of its first slice (waves 0 and 1, 64 rows each): they have landed whenever that
        // slice has.  Padded with NaN past N (topk_mfma_prepare): no clamp.
        if (is == 0 && w < kRows / 64) {
            const float *src = p.rscale + base_row + w * 64 + lane;
            const unsigned dst = __builtin_amdgcn_readfirstlane(lds_rs + (unsigned)(((int)(it & 1)) * kRows + w * 64) * 4u);
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "v"(src), "s"(dst) : "memory");
        }
        const unsigned char *a0 = reinterpret_cast<const unsigned char *>(p.A) + base_row * (int64_t)row_bytes + is * kSliceRowBytes;
        const unsigned char *b0 = Bblock + is * kSliceRowBytes;
        const bool inside = base_row + kRows <= p.N;  // wave-uniform; else the last tile: its rows past N are clamped to row N - 1
        const int last = (int)(p.N - 1 - base_row);   // (their scores are discarded through the NaN row values)
#pragma unroll
        for (int i = 0; i < kDmaA; i++) {
            unsigned off = offA[i];
            if (!inside) {
                const int row = (w * kDmaA + i) * 8 + (lane >> 3), cs = lane & 7;
                off = (unsigned)(row < last ? row : last) * row_bytes + (unsigned)((cs ^ swz(row)) << 4);
            }
            const unsigned dst = __builtin_amdgcn_readfirstlane(lds_slice + (unsigned)ibuf * (unsigned)kSliceBytes + (unsigned)(w * kDmaA + i) * 1024u);
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "v"(off), "s"(a0), "s"(dst) : "memory");
        }
#pragma unroll
        for (int i = 0; i < kDmaB; i++) {
            const unsigned dst = __builtin_amdgcn_readfirstlane(lds_slice + (unsigned)ibuf * (unsigned)kSliceBytes +
                                                                (unsigned)(kRows * kSliceRowBytes) + (unsigned)(w * kDmaB + i) * 1024u);
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "v"(offB[i]), "s"(b0), "s"(dst) : "memory");
        }
        if (++is == S) is = 0, ++it;
        ibuf = ibuf + 1 == kBufs ? 0 : ibuf + 1;
    };

    __syncthreads();  // the per-query words are initialised
    float fth[NCB];
    int cnt[NCB];      // length of this lane's sub-list of its query (mirrored in s_cnt around a compaction)
    uint2 *mine[NCB];  // the lane's sub-list: slots 2 * c + (lane >> 5) of its query's list (see compact_query)
#pragma unroll
    for (int cb = 0; cb < NCB; cb++) {
        const int ql = w * kQueriesPerWave + cb * 32 + (lane & 31);
        fth[cb] = s_f[ql];
        cnt[cb] = 0;
        mine[cb] = p.cbuf + (wgq0 + ql) * kCap + (lane >> 5);
    }
    // the lane's read offsets inside a 32-row block of the slice image, one per k-step (swz(row) is the same in every block)
    unsigned foff[kSlice / 16];
#pragma unroll
    for (int ks = 0; ks < kSlice / 16; ks++) foff[ks] = (unsigned)((lane & 31) * kSliceRowBytes + (((ks * 2 + (lane >> 5)) ^ swz(lane & 31)) << 4));

    f32x16 acc[RB][NCB];
#pragma unroll
    for (int rb = 0; rb < RB; rb++)
#pragma unroll
        for (int cb = 0; cb < NCB; cb++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[rb][cb][r] = 0.0f;

    if (total > 0) issue();
    if (total > 1) issue();
    int64_t t = 0;  // the slice being multiplied: tile t, slice s of it, in buffer buf
    int s = 0, buf = 0;
    for (int64_t g = 0; g < total; g++) {
        // slice g has landed in every wave's share (one slice may stay in flight), then everyone is past slice g - 1
        if (g + 1 < total)
            asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(kDmaPerSlice) : "memory");
        else
            asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
        if (g + 2 < total) issue();
        const unsigned char *sa = s_slice + (size_t)buf * kSliceBytes;
        const unsigned char *sb = sa + kRows * kSliceRowBytes + (size_t)(w * kQueriesPerWave) * kSliceRowBytes;
#pragma unroll
        for (int ks = 0; ks < kSlice / 16; ks++) {
            bf16x8 b[NCB], a[RB];
#pragma unroll
            for (int cb = 0; cb < NCB; cb++) b[cb] = *reinterpret_cast<const bf16x8 *>(sb + cb * 32 * kSliceRowBytes + foff[ks]);
#pragma unroll
            for (int rb = 0; rb < RB; rb++) a[rb] = *reinterpret_cast<const bf16x8 *>(sa + rb * 32 * kSliceRowBytes + foff[ks]);
#pragma unroll
            for (int rb = 0; rb < RB; rb++)
#pragma unroll
                for (int cb = 0; cb < NCB; cb++) acc[rb][cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[rb], b[cb], acc[rb][cb], 0, 0, 0);
        }
        buf = buf + 1 == kBufs ? 0 : buf + 1;
        if (++s < S) continue;
        // ---- the tile's scores are complete.  C layout: a lane holds column (= query) lane & 31, rows (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
        const int64_t base_row = t * stride_rows;
        const float *rs = s_rs + ((int)(t & 1)) * kRows;
#pragma unroll
        for (int rb = 0; rb < RB; rb++) {
            float4 rv[4];
#pragma unroll
            for (int q4 = 0; q4 < 4; q4++) rv[q4] = reinterpret_cast<const float4 *>(rs + rb * 32)[2 * q4 + (lane >> 5)];
#pragma unroll
            for (int cb = 0; cb < NCB; cb++) {
                f32x16 &c = acc[rb][cb];
#pragma unroll
                for (int q4 = 0; q4 < 4; q4++) {
                    c[4 * q4 + 0] = BIAS ? c[4 * q4 + 0] + rv[q4].x : c[4 * q4 + 0] * rv[q4].x;
                    c[4 * q4 + 1] = BIAS ? c[4 * q4 + 1] + rv[q4].y : c[4 * q4 + 1] * rv[q4].y;
                    c[4 * q4 + 2] = BIAS ? c[4 * q4 + 2] + rv[q4].z : c[4 * q4 + 2] * rv[q4].z;
                    c[4 * q4 + 3] = BIAS ? c[4 * q4 + 3] + rv[q4].w : c[4 * q4 + 3] * rv[q4].w;
                }
                // the block's largest score of this query (the hardware maximum skips NaN; sixteen NaNs compare false)
                float m = max3f(c[0], c[1], c[2]);
#pragma unroll
                for (int r = 3; r < 15; r += 2) m = max3f(m, c[r], c[r + 1]);
                m = fmaxf(m, c[15]);
                const float f = fth[cb];  // +inf for a query past nq and for a flagged one
                if (__builtin_amdgcn_ballot_w64(m >= f) == 0) continue;
                // every lane appends to ITS OWN sub-list of the query (even / odd slots): a block adds at most 16 to one
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    if (c[r] >= f) {
                        const uint32_t row = (uint32_t)(base_row + rb * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5));
                        mine[cb][2 * cnt[cb]] = make_uint2(fkey(c[r]), row);
                        cnt[cb]++;
                    }
                }
                uint64_t need = __builtin_amdgcn_ballot_w64(cnt[cb] > p.compact_at);
                if (need) {
                    const int ql = w * kQueriesPerWave + cb * 32 + (lane & 31);
                    s_cnt[2 * ql + (lane >> 5)] = cnt[cb];
                    need = (need | (need >> 32)) & 0xffffffffull;  // either sub-list of a query
                    do {
                        const int l = __builtin_ctzll(need);
                        need &= need - 1;
                        const int qlc = w * kQueriesPerWave + cb * 32 + l;
                        compact_query<false>(p.cbuf + (wgq0 + qlc) * kCap, qlc, p.kth, s_cnt, s_f, s_mg, p.cflag + wgq0 + qlc);
                    } while (need);
                    cnt[cb] = s_cnt[2 * ql + (lane >> 5)];
                    fth[cb] = s_f[ql];
                }
            }
        }
#pragma unroll
        for (int rb = 0; rb < RB; rb++)
#pragma unroll
            for (int cb = 0; cb < NCB; cb++)
#pragma unroll
                for (int r = 0; r < 16; r++) acc[rb][cb][r] = 0.0f;
        s = 0, ++t;
    }
    // final threshold + compaction of every list this wave owns
#pragma unroll
    for (int cb = 0; cb < NCB; cb++) s_cnt[2 * (w * kQueriesPerWave + cb * 32 + (lane & 31)) + (lane >> 5)] = cnt[cb];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int l = 0; l < kQueriesPerWave; l++) {
        const int ql = w * kQueriesPerWave + l;
        if (wgq0 + ql >= p.nq) break;
        const int64_t qg = wgq0 + ql;
        if (s_f[ql] == __builtin_inff()) {  // flagged
            if (p.f_out && lane == 0) p.f_out[qg] = -__builtin_inff();
            continue;
        }
        compact_query<false>(p.cbuf + qg * kCap, ql, p.kth, s_cnt, s_f, s_mg, p.cflag + qg);
        if (lane == 0) {
            p.ccnt[qg] = s_cnt[2 * ql] + s_cnt[2 * ql + 1];  // packed by the final compaction: slots 0 .. count-1
            if (p.f_out) p.f_out[qg] = s_f[ql] == __builtin_inff() ? -__builtin_inff() : s_f[ql];
        }
    }
}

template <bool BIAS>
int32_t launch_deep(gorse_topk *h, const SweepParams &p) {
    const size_t lds = lds_bytes();
    GORSE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&topk_deep_sweep_kernel<BIAS>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    topk_deep_sweep_kernel<BIAS><<<dim3((unsigned)ceil_div(p.nq, kQueries)), dim3(kThreads), lds, h->stream>>>(p, h->kp * 16);
    GORSE_HIP_CHECK(hipGetLastError());
    return GORSE_OK;
}

}  // namespace

// the main or a pilot sweep of a deep handle (h->deep: operands of h->kp * 16 values, whole K-slices)
int32_t gorse::dispatch_deep_sweep(gorse_topk *h, const SweepParams &p) {
    if (p.nq <= 0) return GORSE_OK;
    if (h->kp * 16 % kSlice != 0 || h->kp * 16 < 2 * kSlice)  // (a tile's row values are issued two slices ahead: at least two per tile)
        return fail(GORSE_ERR_INVALID, "deep operand depth %d is not whole K-slices", h->kp * 16);
    return p.ep == EP_BIAS ? launch_deep<true>(h, p) : launch_deep<false>(h, p);
}
