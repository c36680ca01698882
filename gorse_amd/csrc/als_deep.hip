// als_deep.hip -- the Deep form of an eALS half-sweep: the Gram form of als.hip (M = (1 - w) G + w S per row, one Gauss-Seidel
// sweep over it; model/cf/model.go:659-738) for 128 < nFactors <= 256, opt-in through gorse_mf_set_als_form(h, 1).
//
// A full M of 256 x 256 floats is 256 KB and a workgroup has 160 KB of LDS, so only the upper triangle of M's grid of 32 x 32 blocks is
// ever formed (als_deep_plan.hpp): 36 blocks at d = 256, 148.5 KB with the padded row stride, plus 3 KB of vectors.
//
//   G      one 256-thread workgroup per row (or per chunk of a long row).  The row's gathered factor rows go through a ring of two LDS
//          buffers of 32 rows inside the region that holds M afterwards, the next batch's loads in flight while the current one is
//          multiplied (64-bit gather addresses: factor matrices of any size; a column past d and an entry past the row's end are
//          zeros).  The NT blocks are dealt round-robin to the four waves -- block t to wave t mod 4, nine blocks = 144 accumulator
//          registers per lane at d = 256 -- and every block is accumulated by v_mfma_f32_32x32x2_f32: exact fp32 products, one
//          instruction per pair of gathered rows.  The wave that owns a diagonal block also keeps that block's column sums.
//   M      each wave writes (1 - w) G + w S for its blocks to LDS; S arrives packed the same way (below), so it is read coalesced.
//   sweep  Gauss-Seidel in blocks of 32 coordinates.  y = M p is kept in LDS.  For block b one wave runs the 32 dependent steps on the
//          diagonal block alone (a lane per coordinate: one fused step, one v_readlane, one fused update per step), leaving the 32
//          deltas in LDS; then all the threads of the blocks behind b add delta^T M[b, :] to their y -- a rank-32 update, in parallel.
//          In exact arithmetic this IS the coordinate sweep: y_j is not read before block j / 32's turn.  Row j of the symmetric M is
//          block row j / 32 from the diagonal on (rows of blocks) and block column j / 32 above it (columns of blocks, conflict-free
//          with the stride of 33).
//   S      the Gram of the other side: the same accumulation over chunks of 1024 rows with feedback, the chunks' partial triangles
//          added in chunk order by one thread per element.
//   long   a row above the plan's threshold: its chunks' partial triangles are added the same way, als_deep_long_kernel forms M
//          from the sum and sweeps.
// No atomics anywhere: every sum has one fixed order, two runs give the same bits.
#include <algorithm>
#include <type_traits>
#include <utility>

#include "als_deep_plan.hpp"
#include "mf_internal.hpp"

using namespace gorse;

namespace {

typedef float deep_f32x16 __attribute__((ext_vector_type(16)));

constexpr int deep_slots(int nb) { return (deep_nt(nb) + 3) / 4; }  // blocks per wave: slot s of wave W is block 4 s + W
// whether wave w multiplies column block b (as a row or a column operand of one of its blocks)
constexpr bool deep_wave_reads(int nb, int w, int b) {
    for (int t = w; t < deep_nt(nb); t += 4)
        if (deep_tile_bi(nb, t) == b || deep_tile_bj(nb, t) == b) return true;
    return false;
}
// f(integral_constant<int, 0>) .. f(integral_constant<int, N - 1>): a loop whose counter is a constant expression in its body
template <typename F, int... I>
__device__ __forceinline__ void deep_for_seq(F &&f, std::integer_sequence<int, I...>) {
    (f(std::integral_constant<int, I>{}), ...);
}
template <int N, typename F>
__device__ __forceinline__ void deep_for(F &&f) {
    deep_for_seq(f, std::make_integer_sequence<int, N>{});
}

// G and the column sums of entries idx[beg .. beg + n) of B into this wave's blocks; ends with a barrier (the ring is free again)
template <int NB, int W>
__device__ __forceinline__ void deep_gram(const float *__restrict__ B, const int32_t *__restrict__ idx, int64_t beg, int n, int d,
                                          float *ring, deep_f32x16 (&tl)[deep_slots(NB)], float (&cs)[deep_slots(NB)]) {
    constexpr int DW = 32 * NB, NT = deep_nt(NB), NS = deep_slots(NB);
    const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, col = lane & 31;
    const int ge = tid >> 5, gc = tid & 31;  // gather: entries ge, ge + 8, ge + 16, ge + 24 of the batch, column gc of every block
#pragma unroll
    for (int s = 0; s < NS; s++) {
        cs[s] = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; r++) tl[s][r] = 0.0f;
    }
    float g[4][NB];
    auto gather = [&](int e0) {
#pragma unroll
        for (int ps = 0; ps < 4; ps++) {
            const int e = e0 + ge + 8 * ps;
            if (e < n) {
                const float *row = B + (int64_t)idx[beg + e] * d;
#pragma unroll
                for (int b = 0; b < NB; b++) g[ps][b] = 32 * b + gc < d ? row[32 * b + gc] : 0.0f;
            } else {
#pragma unroll
                for (int b = 0; b < NB; b++) g[ps][b] = 0.0f;
            }
        }
    };
    if (n > 0) gather(0);
    int buf = 0;
    for (int e0 = 0; e0 < n; e0 += kDeepBatch) {
        float *sq = ring + buf * (kDeepBatch * DW);
#pragma unroll
        for (int ps = 0; ps < 4; ps++)
#pragma unroll
            for (int b = 0; b < NB; b++) sq[(ge + 8 * ps) * DW + 32 * b + gc] = g[ps][b];
        __syncthreads();  // (one barrier per batch: a buffer is rewritten two batches after it was read)
        if (e0 + kDeepBatch < n) gather(e0 + kDeepBatch);
        const int m = n - e0 < kDeepBatch ? n - e0 : kDeepBatch;
        const int pairs = (m + 1) >> 1;  // (an odd end: the last pair's second entry is a row of zeros)
        const float *mine = sq + half * DW + col;
#pragma unroll 2
        for (int p = 0; p < pairs; p++) {
            float fr[NB];
            deep_for<NB>([&](auto bc) {
                constexpr int b = decltype(bc)::value;
                fr[b] = deep_wave_reads(NB, W, b) ? mine[p * 2 * DW + 32 * b] : 0.0f;
            });
            deep_for<NS>([&](auto sc) {
                constexpr int s = decltype(sc)::value, t = 4 * s + W;
                if constexpr (t < NT) {
                    constexpr int bi = deep_tile_bi(NB, t), bj = deep_tile_bj(NB, t);
                    tl[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(fr[bi], fr[bj], tl[s], 0, 0, 0);
                    if constexpr (bi == bj) cs[s] += fr[bi];
                }
            });
        }
        buf ^= 1;
    }
    __syncthreads();
}

// this wave's blocks -> M = (1 - w) G + w S in LDS, the diagonal blocks' column sums -> ss.  Element r of a 32 x 32 accumulator is
// (row (r & 3) + 8 (r >> 2) + 4 (lane >> 5), column lane & 31).  Rows and columns past d are zeros of G (deep_gram) and of S (built
// the same way), so nothing is masked here.
template <int NB, int W>
__device__ __forceinline__ void deep_form(const deep_f32x16 (&tl)[deep_slots(NB)], const float (&cs)[deep_slots(NB)],
                                          const float *__restrict__ S, float w, float *sM, float *ss) {
    constexpr int NT = deep_nt(NB), NS = deep_slots(NB);
    const int lane = threadIdx.x & 63, half = lane >> 5, col = lane & 31;
    const float one_w = 1 - w;
    // (S's 144 load addresses are invariant across the kernel's row loop; formed from the pointer as written they are hoisted out of
    // it and held in registers beside the accumulators: an opaque copy forms them here, from one scalar base)
    const float *Sq = S;
    asm volatile("" : "+s"(Sq));
#pragma unroll
    for (int s = 0; s < NS; s++) {
        const int t = 4 * s + W;
        if (t < NT) {
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int i = (r & 3) + 8 * (r >> 2) + 4 * half;
                sM[t * kDeepTileLds + i * kDeepTileLd + col] = one_w * tl[s][r] + w * Sq[t * kDeepTileMem + i * 32 + col];
            }
            // (a block's sixteen loads of S at a time: left to itself the scheduler issues all 144 of a wave up front, beside the 144
            // accumulators they are added to -- 991 spilled registers at nFactors 256)
            __builtin_amdgcn_sched_barrier(0);
            if (deep_tile_bi(NB, t) == deep_tile_bj(NB, t)) {
                const float other = __shfl_xor(cs[s], 32, 64);
                if (lane < 32) ss[32 * deep_tile_bi(NB, t) + col] = cs[s] + other;
            }
        }
    }
}

// this wave's blocks and column sums -> the chunk's partial in global memory (dense blocks, then the 32 NB sums)
template <int NB, int W>
__device__ __forceinline__ void deep_store_partial(const deep_f32x16 (&tl)[deep_slots(NB)], const float (&cs)[deep_slots(NB)],
                                                   float *__restrict__ dst) {
    constexpr int NT = deep_nt(NB), NS = deep_slots(NB);
    const int lane = threadIdx.x & 63, half = lane >> 5, col = lane & 31;
#pragma unroll
    for (int s = 0; s < NS; s++) {
        const int t = 4 * s + W;
        if (t < NT) {
#pragma unroll
            for (int r = 0; r < 16; r++) dst[t * kDeepTileMem + ((r & 3) + 8 * (r >> 2) + 4 * half) * 32 + col] = tl[s][r];
            if (deep_tile_bi(NB, t) == deep_tile_bj(NB, t)) {
                const float other = __shfl_xor(cs[s], 32, 64);
                if (lane < 32) dst[NT * kDeepTileMem + 32 * deep_tile_bi(NB, t) + col] = cs[s] + other;
            }
        }
    }
}

template <int NB, int W, bool CHUNKS>
__device__ __forceinline__ void deep_item(const float *__restrict__ B, const int32_t *__restrict__ idx, int64_t beg, int n, int d,
                                          const float *__restrict__ S, float w, float *sM, float *ss, float *__restrict__ dst) {
    deep_f32x16 tl[deep_slots(NB)];
    float cs[deep_slots(NB)];
    deep_gram<NB, W>(B, idx, beg, n, d, sM, tl, cs);
    if (CHUNKS)
        deep_store_partial<NB, W>(tl, cs, dst);
    else
        deep_form<NB, W>(tl, cs, S, w, sM, ss);
}

// The Gauss-Seidel sweep of row `a` over M (LDS blocks, zero past d) and the column sums in sv[0 .. 32 NB) by the whole workgroup
// (256 threads).  M and the sums must be visible (a barrier behind their last write); ends with a barrier (M and sv are free again).
// With s the column sums and y = M p:  p_f' = (s_f - (y_f - p_f M_ff)) / (M_ff + reg) = base_f - y_f inv_f,  y += (p_f' - p_f) M[:, f].
template <int NB>
__device__ __forceinline__ void deep_sweep(float *__restrict__ a, int d, float reg, const float *sM, float *sv) {
    constexpr int DW = 32 * NB;
    float *ss = sv, *sp = sv + 256, *sy = sv + 512, *sdl = sv + 768;
    const int tid = threadIdx.x, bj = tid >> 5, jr = tid & 31;
    if (tid < DW) sp[tid] = tid < d ? a[tid] : 0.0f;
    __syncthreads();
    if (tid < DW) {  // y_j = sum_i M[i][j] p_i: column j of the blocks above the diagonal block, row j of those from it on
        float y = 0.0f;
#pragma unroll
        for (int bi = 0; bi < NB; bi++) {
            const bool above = bi <= bj;
            const float *tp = above ? sM + deep_tile(NB, bi, bj) * kDeepTileLds + jr : sM + deep_tile(NB, bj, bi) * kDeepTileLds + jr * kDeepTileLd;
            const int st = above ? kDeepTileLd : 1;
#pragma unroll 8
            for (int ir = 0; ir < 32; ir++) y = fmaf(tp[ir * st], sp[32 * bi + ir], y);
        }
        sy[tid] = y;
    }
    __syncthreads();
#pragma unroll 1
    for (int b = 0; b < NB; b++) {
        if (tid < 64) {  // the block's 32 dependent steps: lane r (and its twin r + 32) holds coordinate 32 b + r
            const float *td = sM + deep_tile(NB, b, b) * kDeepTileLds;
            const int r = tid & 31, k = 32 * b + r;
            const float diag = td[r * kDeepTileLd + r], p = sp[k];
            const float inv = k < d ? 1.0f / (diag + reg) : 0.0f;  // a padded coordinate (zero row and column of M) stays 0
            const float base = (ss[k] + p * diag) * inv, gk = base - p;
            float y = sy[k];
            int dm = 0;  // lane s: the bits of step s's delta
            deep_for<32>([&](auto sc) {
                constexpr int s = decltype(sc)::value;
                const float m = td[s * kDeepTileLd + r];
                const float dk = fmaf(-y, inv, gk);  // this lane's would-be step
                const int delta = __builtin_amdgcn_readlane(__float_as_int(dk), s);
                // (not `dm = r == s ? dk : dm`: the 32 compares' masks are invariant and would sit in scalar registers across the block loop)
                asm("v_writelane_b32 %0, %1, %2" : "+v"(dm) : "s"(delta), "n"(s));
                y = fmaf(__int_as_float(delta), m, y);
            });
            if (tid < 32) {
                sdl[r] = __int_as_float(dm);
                if (k < d) a[k] = p + __int_as_float(dm);
            }
        }
        __syncthreads();
        if (bj > b && tid < DW) {  // the blocks behind b take the 32 steps at once
            const float *tp = sM + deep_tile(NB, b, bj) * kDeepTileLds + jr;
            float y = sy[tid];
#pragma unroll 8
            for (int s = 0; s < 32; s++) y = fmaf(sdl[s], tp[s * kDeepTileLd], y);
            sy[tid] = y;
        }
        __syncthreads();
    }
}

// CHUNKS = false: the rows of `rows` (n_items of them), accumulated and solved.  CHUNKS = true: the chunks (chunk_beg / chunk_cnt,
// n_items of them) of the long rows -- or of the list of rows with feedback, for S -- each leaving its partial in `partial`.
template <int NB, bool CHUNKS>
__global__ __launch_bounds__(256) void als_deep_kernel(float *__restrict__ A, const float *__restrict__ B, const int64_t *__restrict__ ptr,
                                                       const int32_t *__restrict__ idx, const float *__restrict__ S,
                                                       const int32_t *__restrict__ rows, const int64_t *__restrict__ chunk_beg,
                                                       const int32_t *__restrict__ chunk_cnt, int64_t n_items, int d, float w, float reg,
                                                       float *__restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *sM = smem, *sv = smem + deep_nt(NB) * kDeepTileLds;
    for (int64_t t = blockIdx.x; t < n_items; t += gridDim.x) {
        int64_t u = 0, beg;
        int n;
        if (CHUNKS) {
            beg = chunk_beg[t];
            n = chunk_cnt[t];
        } else {
            u = rows[t];
            beg = ptr[u];
            n = (int)(ptr[u + 1] - beg);
        }
        float *dst = CHUNKS ? partial + t * deep_partial_stride(NB) : nullptr;
        switch (threadIdx.x >> 6) {  // wave-uniform; every branch meets the same barriers
        case 0: deep_item<NB, 0, CHUNKS>(B, idx, beg, n, d, S, w, sM, sv, dst); break;
        case 1: deep_item<NB, 1, CHUNKS>(B, idx, beg, n, d, S, w, sM, sv, dst); break;
        case 2: deep_item<NB, 2, CHUNKS>(B, idx, beg, n, d, S, w, sM, sv, dst); break;
        default: deep_item<NB, 3, CHUNKS>(B, idx, beg, n, d, S, w, sM, sv, dst); break;
        }
        if (!CHUNKS) {
            __syncthreads();
            deep_sweep<NB>(A + u * d, d, reg, sM, sv);
        }
    }
}

// the long rows: M from the row's added-up partial (als_deep_reduce_kernel), then the sweep
template <int NB>
__global__ __launch_bounds__(256) void als_deep_long_kernel(float *__restrict__ A, const float *__restrict__ S,
                                                            const int32_t *__restrict__ rows, int64_t n_rows, int d, float w, float reg,
                                                            const float *__restrict__ reduced) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *sM = smem, *sv = smem + deep_nt(NB) * kDeepTileLds;
    const float one_w = 1 - w;
    for (int64_t t = blockIdx.x; t < n_rows; t += gridDim.x) {
        const float *src = reduced + t * deep_partial_stride(NB);
        for (int e = threadIdx.x; e < (int)deep_packed(NB); e += 256)
            sM[(e >> 10) * kDeepTileLds + ((e >> 5) & 31) * kDeepTileLd + (e & 31)] = one_w * src[e] + w * S[e];
        if (threadIdx.x < 32 * NB) sv[threadIdx.x] = src[deep_packed(NB) + threadIdx.x];
        __syncthreads();
        deep_sweep<NB>(A + (int64_t)rows[t] * d, d, reg, sM, sv);
    }
}

// out[t][e] = the sum over row t's partials first[t] .. first[t] + nch[t] - 1 of element e < len, in that order, one thread per
// element with eight loads in flight (first == null: one row, partials 0 .. nch_all - 1 -- the S Gram; no partials: zeros)
__global__ __launch_bounds__(256) void als_deep_reduce_kernel(const float *__restrict__ partial, const int32_t *__restrict__ first,
                                                              const int32_t *__restrict__ nch, int64_t n_rows, int nch_all, int64_t stride,
                                                              int len, float *__restrict__ out, int64_t out_stride) {
    const int nb = (len + 255) / 256;
    for (int64_t b = blockIdx.x; b < n_rows * nb; b += gridDim.x) {
        const int64_t t = b / nb;
        const int e = (int)(b - t * nb) * 256 + threadIdx.x;
        if (e >= len) continue;
        const int nc = first ? nch[t] : nch_all;
        const float *src = partial + (int64_t)(first ? first[t] : 0) * stride + e;
        float acc = 0.0f;
        int c = 0;
        for (; c + 7 < nc; c += 8) {
            float x[8];
#pragma unroll
            for (int j = 0; j < 8; j++) x[j] = src[(int64_t)(c + j) * stride];
#pragma unroll
            for (int j = 0; j < 8; j++) acc += x[j];
        }
        for (; c < nc; c++) acc += src[(int64_t)c * stride];
        out[t * out_stride + e] = acc;
    }
}

struct DeepKernels {
    decltype(&als_deep_kernel<8, false>) row, chunk;
    decltype(&als_deep_long_kernel<8>) solve;
};
const DeepKernels &deep_kernels(int nb) {
#define DEEP(NB) {als_deep_kernel<NB, false>, als_deep_kernel<NB, true>, als_deep_long_kernel<NB>}
    static const DeepKernels table[] = {DEEP(5), DEEP(6), DEEP(7), DEEP(8)};  // 129..160, ..192, ..224, ..256
#undef DEEP
    return table[nb - 5];
}

template <typename K>
int32_t deep_launch(K kernel, int64_t items, int nb, hipStream_t st, float *A, const float *B, const int64_t *ptr, const int32_t *idx,
                    const float *S, const int32_t *rows, const int64_t *cbeg, const int32_t *ccnt, int d, float w, float reg,
                    float *partial) {
    // (dynamic LDS above 64 KB is allowed per device: asked for in front of every launch, as als.hip's allow_lds does)
    GORSE_HIP_CHECK(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)deep_lds_bytes(nb)));
    kernel<<<dim3((unsigned)std::min<int64_t>(items, 2048)), dim3(256), deep_lds_bytes(nb), st>>>(A, B, ptr, idx, S, rows, cbeg, ccnt, items,
                                                                                              d, w, reg, partial);
    GORSE_HIP_CHECK(hipGetLastError());
    return GORSE_OK;
}

int32_t deep_reduce(hipStream_t st, const float *partial, const int32_t *first, const int32_t *nch, int64_t n_rows, int nch_all,
                    int64_t stride, int len, float *out, int64_t out_stride) {
    const int64_t blocks = std::min<int64_t>(n_rows * ceil_div(len, 256), (int64_t)1 << 20);
    als_deep_reduce_kernel<<<dim3((unsigned)blocks), dim3(256), 0, st>>>(partial, first, nch, n_rows, nch_all, stride, len, out, out_stride);
    GORSE_HIP_CHECK(hipGetLastError());
    return GORSE_OK;
}

}  // namespace

namespace gorse {

// one half-sweep in the Deep form: S (packed) over ALL rows with feedback of the other side (plan 1 - side), then the rows of this
// handle's range of `side` (plan side: short rows whole, long rows by chunks, reduce and solve)
int32_t als_deep_half_epoch(gorse_mf *h, int side, float *A, const float *B, const int64_t *ptr, const int32_t *idx, float w, float reg) {
    const int d = h->d;
    if (!deep_serves(d)) return fail(GORSE_ERR_INVALID, "the Deep ALS form covers nFactors %d..%d (got %d)", kDeepMinD, kDeepMaxD, d);
    const int nb = deep_nb(d);
    const int64_t stride = deep_partial_stride(nb);
    const DeepKernels &k = deep_kernels(nb);
    const gorse_mf::AlsPlan &gp = h->als_plan[1 - side], &pl = h->als_plan[side];
    GORSE_TRY(h->gram.ensure(std::max<size_t>((size_t)d * d, (size_t)deep_packed(nb))));
    int tok = h->prof.begin(GORSE_PROF_ALS_GRAM, h->stream);
    if (gp.n_gchunks > 0) {
        GORSE_TRY(h->gram_partial.ensure((size_t)gp.n_gchunks * stride));
        GORSE_TRY(deep_launch(k.chunk, gp.n_gchunks, nb, h->stream, nullptr, B, nullptr, gp.fb_rows.p, nullptr, nullptr, gp.g_beg.p,
                              gp.g_cnt.p, d, 0.0f, 0.0f, h->gram_partial.p));
    }
    GORSE_TRY(deep_reduce(h->stream, h->gram_partial.p, nullptr, nullptr, 1, (int)gp.n_gchunks, stride, (int)deep_packed(nb), h->gram.p, 0));
    h->prof.end(tok, h->stream);
    tok = h->prof.begin(GORSE_PROF_ALS_SWEEP, h->stream);
    if (pl.n_short > 0)
        GORSE_TRY(deep_launch(k.row, pl.n_short, nb, h->stream, A, B, ptr, idx, h->gram.p, pl.short_rows.p, nullptr, nullptr, d, w, reg,
                              nullptr));
    if (pl.n_long > 0) {
        GORSE_TRY(h->als_partial.ensure((size_t)pl.n_chunks * stride));
        GORSE_TRY(h->als_reduced.ensure((size_t)pl.n_long * stride));
        GORSE_TRY(deep_launch(k.chunk, pl.n_chunks, nb, h->stream, nullptr, B, nullptr, idx, nullptr, nullptr, pl.chunk_beg.p, pl.chunk_cnt.p,
                              d, 0.0f, 0.0f, h->als_partial.p));
        GORSE_TRY(deep_reduce(h->stream, h->als_partial.p, pl.long_first.p, pl.long_nch.p, pl.n_long, 0, stride, (int)stride,
                              h->als_reduced.p, stride));
        GORSE_HIP_CHECK(hipFuncSetAttribute((const void *)k.solve, hipFuncAttributeMaxDynamicSharedMemorySize, (int)deep_lds_bytes(nb)));
        k.solve<<<dim3((unsigned)std::min<int64_t>(pl.n_long, 2048)), dim3(256), deep_lds_bytes(nb), h->stream>>>(
            A, h->gram.p, pl.long_rows.p, pl.n_long, d, w, reg, h->als_reduced.p);
        GORSE_HIP_CHECK(hipGetLastError());
    }
    h->prof.end(tok, h->stream);
    return GORSE_OK;
}

}  // namespace gorse
