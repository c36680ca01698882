// topk_deep_body.hpp -- the K-loop of the deep sweep of path B, shared by its two kernels' units: topk_deep.hip (the main / pilot
// form, 256 queries per workgroup; its head says how the loop works and why the sweep is exact) and topk_deep_hist.hip (the history
// form of the tie path, 128 queries per workgroup; rules in topk_deep_hist_plan.hpp).  One __device__ template; each unit's
// __global__ kernel is a call of it.
//
// HIST = false is the main sweep's non-symmetric, non-history contract.  HIST = true is the shallow history sweep's
// (topk_sweep_kernel<..., HIST>), in full:
//   grid.y = p.nslices row slices; slice y sweeps the tiles [NT_all * y / nslices, NT_all * (y + 1) / nslices) of kRows rows;
//   the per-query outputs (cbuf, ccnt, cflag, hbuf, hcnt, f_out) are slice-major, at y * nq + q;
//   a query starts from p.fwarm[y * nq + q] (trusted: tie_warm_kernel's bound) or, without fwarm, from -inf; f0 is not read;
//   compact_query<true>: what a raised threshold drops goes to the query's history in arrival order, the history's length lives in
//   LDS and reaches hcnt at the end, a history past kHistCap flags the query; a slice without tiles leaves its lists empty.
#pragma once
#include "topk_compact.hpp"
#include "topk_deep_hist_plan.hpp"
#include "topk_mfma_internal.hpp"

namespace gorse {
namespace topk_deep_body {
using namespace topk_deep_hist_plan;  // (and topk_deep_plan)

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float max3f(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }

// BIAS: the row value is added to the score (Euclidean), else multiplied (cosine's scale; 1 for -dot, where only its NaN matters)
template <bool BIAS, bool HIST>
__device__ __forceinline__ void deep_sweep_body(const SweepParams &p, int kpad) {
    constexpr int QPW = HIST ? kHistQueriesPerWave : kQueriesPerWave;  // queries per wave and per workgroup, a slice's LDS image,
    constexpr int QWG = HIST ? kHistQueries : kQueries;                // a wave's B instructions and the counted wait: the plan headers'
    constexpr size_t SLICEB = HIST ? kHistSliceBytes : kSliceBytes;
    constexpr int DMAB = HIST ? kHistDmaB : kDmaB;
    constexpr int PERSLICE = HIST ? kHistDmaPerSlice : kDmaPerSlice;
    constexpr int RB = kRows / 32, NCB = QPW / 32;
    static_assert(SLICEB == (size_t)(kRows + QWG) * kSliceRowBytes && PERSLICE == kDmaA + DMAB && DMAB * 8 == QPW, "the form's shape");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char *s_slice = smem;  // kBufs x (kRows + QWG) pieces of 128 bytes: the A rows, then the B rows
    float *s_rs = reinterpret_cast<float *>(smem + kBufs * SLICEB);  // the row values of tile t at (t & 1) * kRows
    int *s_cnt = reinterpret_cast<int *>(s_rs + 2 * kRows);          // 2 per query: the interleaved sub-list lengths
    float *s_f = reinterpret_cast<float *>(s_cnt + 2 * QWG);
    float *s_mg = s_f + QWG;
    int *s_hc = reinterpret_cast<int *>(s_mg + QWG);  // HIST: the history lengths

    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t wgq0 = (int64_t)blockIdx.x * QWG;
    const int64_t qslice = HIST ? (int64_t)blockIdx.y * p.nq : 0;  // this slice's rows of the per-query output arrays
    for (int t = tid; t < QWG; t += kThreads) {
        const int64_t q = wgq0 + t;
        s_cnt[2 * t] = 0;
        s_cnt[2 * t + 1] = 0;
        if (HIST) s_hc[t] = 0;
        if (HIST)
            s_f[t] = q < p.nq ? (p.fwarm ? p.fwarm[qslice + q] : -__builtin_inff()) : __builtin_inff();
        else
            s_f[t] = q < p.nq ? (p.f0 ? p.f0[q] : -__builtin_inff()) : __builtin_inff();  // a query past nq collects nothing
        s_mg[t] = q < p.nq ? p.qmargin[q] : 0.0f;
    }
    const int S = kpad / kSlice;                                         // K-slices per tile
    const int64_t stride_rows = (int64_t)p.tile_stride * kRows;          // a pilot samples every tile_stride-th tile
    const int64_t NT_all = (p.N + stride_rows - 1) / stride_rows;
    // HIST: this slice's tiles [T0, T1); else all of them
    const int64_t T0 = HIST ? NT_all * blockIdx.y / gridDim.y : 0, T1 = HIST ? NT_all * (blockIdx.y + 1) / gridDim.y : NT_all;
    const int64_t total = (T1 - T0) * S;                                 // slices this workgroup multiplies
    const unsigned row_bytes = (unsigned)kpad * 2u;

    // Piece c (16 bytes) of row r lives at piece c ^ swz(r) of the row's 128-byte LDS image: the 16 lanes of a ds_read_b128 group read
    // one piece column of 16 consecutive rows -- two rows per 256-byte bank row -- and the XOR spreads them over its 16 slots.
    auto swz = [](int row) -> int { return (row >> 1) & 7; };
    // DMA instruction i of this wave: 64 pieces = 8 consecutive rows of the slice's LDS image.  The lane's source offset from the
    // tile's (A) or the query block's (B) first byte of the slice is a 32-bit register computed once; the base is a 64-bit scalar.
    unsigned offA[kDmaA], offB[DMAB];
#pragma unroll
    for (int i = 0; i < kDmaA; i++) {
        const int row = (w * kDmaA + i) * 8 + (lane >> 3), cs = lane & 7;
        offA[i] = (unsigned)row * row_bytes + (unsigned)((cs ^ swz(row)) << 4);
    }
#pragma unroll
    for (int i = 0; i < DMAB; i++) {
        const int row = (w * DMAB + i) * 8 + (lane >> 3), cs = lane & 7;  // = the query's place in the block
        int64_t q = wgq0 + row;
        if (q >= p.nq) q = p.nq - 1;  // clamped: its threshold is +inf
        offB[i] = (unsigned)(q - wgq0) * row_bytes + (unsigned)((cs ^ swz(row)) << 4);
    }
    const unsigned lds_slice = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)s_slice;
    const unsigned lds_rs = (unsigned)(uintptr_t)(__attribute__((address_space(3))) float *)s_rs;
    const unsigned char *Bblock = reinterpret_cast<const unsigned char *>(p.B) + wgq0 * (int64_t)row_bytes;

    // the next slice to issue: tile it, slice is of it, into buffer ibuf
    int64_t it = T0;
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
            const unsigned dst = __builtin_amdgcn_readfirstlane(lds_slice + (unsigned)ibuf * (unsigned)SLICEB + (unsigned)(w * kDmaA + i) * 1024u);
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "v"(off), "s"(a0), "s"(dst) : "memory");
        }
#pragma unroll
        for (int i = 0; i < DMAB; i++) {
            const unsigned dst = __builtin_amdgcn_readfirstlane(lds_slice + (unsigned)ibuf * (unsigned)SLICEB +
                                                                (unsigned)(kRows * kSliceRowBytes) + (unsigned)(w * DMAB + i) * 1024u);
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "v"(offB[i]), "s"(b0), "s"(dst) : "memory");
        }
        if (++is == S) is = 0, ++it;
        ibuf = ibuf + 1 == kBufs ? 0 : ibuf + 1;
    };
    // the compaction of local query qlc of this workgroup (the wave that owns it calls)
    auto compact = [&](int qlc) {
        const int64_t qg = qslice + wgq0 + qlc;
        if constexpr (HIST)
            compact_query<true>(p.cbuf + qg * kCap, qlc, p.kth, s_cnt, s_f, s_mg, p.cflag + qg, p.hbuf + qg * kHistCap, s_hc, p.fwarm != nullptr);
        else
            compact_query<false>(p.cbuf + qg * kCap, qlc, p.kth, s_cnt, s_f, s_mg, p.cflag + qg);
    };

    __syncthreads();  // the per-query words are initialised
    float fth[NCB];
    int cnt[NCB];      // length of this lane's sub-list of its query (mirrored in s_cnt around a compaction)
    uint2 *mine[NCB];  // the lane's sub-list: slots 2 * c + (lane >> 5) of its query's list (see compact_query)
#pragma unroll
    for (int cb = 0; cb < NCB; cb++) {
        const int ql = w * QPW + cb * 32 + (lane & 31);
        fth[cb] = s_f[ql];
        cnt[cb] = 0;
        mine[cb] = p.cbuf + (qslice + wgq0 + ql) * kCap + (lane >> 5);
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
    int64_t t = T0;  // the slice being multiplied: tile t, slice s of it, in buffer buf
    int s = 0, buf = 0;
    for (int64_t g = 0; g < total; g++) {
        // slice g has landed in every wave's share (one slice may stay in flight), then everyone is past slice g - 1
        if (g + 1 < total)
            asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(PERSLICE) : "memory");
        else
            asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
        if (g + 2 < total) issue();
        const unsigned char *sa = s_slice + (size_t)buf * SLICEB;
        const unsigned char *sb = sa + kRows * kSliceRowBytes + (size_t)(w * QPW) * kSliceRowBytes;
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
                    const int ql = w * QPW + cb * 32 + (lane & 31);
                    s_cnt[2 * ql + (lane >> 5)] = cnt[cb];
                    need = (need | (need >> 32)) & 0xffffffffull;  // either sub-list of a query
                    do {
                        const int l = __builtin_ctzll(need);
                        need &= need - 1;
                        compact(w * QPW + cb * 32 + l);
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
    for (int cb = 0; cb < NCB; cb++) s_cnt[2 * (w * QPW + cb * 32 + (lane & 31)) + (lane >> 5)] = cnt[cb];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int l = 0; l < QPW; l++) {
        const int ql = w * QPW + l;
        if (wgq0 + ql >= p.nq) break;
        const int64_t qg = qslice + wgq0 + ql;
        if (s_f[ql] == __builtin_inff()) {  // flagged
            if (p.f_out && lane == 0) p.f_out[qg] = -__builtin_inff();
            continue;
        }
        compact(ql);
        if (lane == 0) {
            p.ccnt[qg] = s_cnt[2 * ql] + s_cnt[2 * ql + 1];  // packed by the final compaction: slots 0 .. count-1
            if (HIST) p.hcnt[qg] = s_hc[ql];
            if (p.f_out) p.f_out[qg] = s_f[ql] == __builtin_inff() ? -__builtin_inff() : s_f[ql];
        }
    }
}

}  // namespace topk_deep_body
}  // namespace gorse
