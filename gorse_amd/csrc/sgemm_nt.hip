// sgemm_nt.hip -- floats.MM's NT case (C[i][j] = floats.Dot(A row i, B row j), C overwritten) on the fp32 matrix cores of gfx950.
// Reference: common/floats/mm.go:19-49 (the !transA && transB case), src/floats_avx512.c _mm512_dot.
//
// Bits.  Every element is dot512_lds's (cf_device.hpp): sixteen lane chains -- chain l is a[l] * b[l], then fmaf(a[16 c + l],
// b[16 c + l], acc_l) over the full chunks c = 1 .. nfull - 1 in order -- then group_tree16 over the sixteen lane sums, then the
// 8-lane tail (unfused products, group_tree8) where k % 16 >= 8, then the scalar tail as an fmaf chain in element order.  One
// v_mfma_f32_32x32x1_2b_f32 advances TWO lane chains of a 32 x 32 tile of C by one step: its block 0 is AVX lane l, its block 1
// AVX lane l + 8, with operands A[i][16 c + l (+ 8)] and B[j][16 c + l (+ 8)] (recommend_mfma.hip forms its scores the same way, and
// its tests hold the instruction to IEEE fmaf, subnormals included).  The accumulators start at -0, so the first step
// fma(a, b, -0) is a * b in every bit, a -0 product included; there is never a padded step (a +0 * +0 step would turn a -0 sum
// into +0): the last k block issues only the chunks that exist, and the k past the last full chunk never reach the MFMA.
//
// Work split.  The price of the bits is sixteen accumulators per element of C, so a wave with R accumulator registers owns 4 R
// elements.  The tile here is 32 x 32 per wave: all 256 AGPRs hold the eight accumulator pairs (lanes l and l + 8, l = 0 .. 7)
// across the whole k loop, one wave per SIMD.  The alternative, 16 x 32 in 128 AGPRs and two waves per SIMD, has no instruction that
// fits it: 32x32x1_2b needs 32 rows of both operands, and 16x16x1_4b moves the same two operand words per lane for half the
// multiply-adds, twice the LDS traffic per flop.  With 32 x 32 a chunk of 16 k is eight MFMAs (512 cycles of the matrix pipe) fed by
// sixteen operand words per lane; the eight MFMAs write eight different accumulator pairs, so they issue back to back.
// A workgroup is four waves, 2 x 2 wave tiles = 64 x 64 of C; registers allow one per CU.
//
// Operands.  A and B rows stream through LDS in k blocks of 128 (eight chunks), double-buffered (132 KB of the CU's 160: one
// workgroup per CU is what the registers allow anyway): the next block's global loads are issued before the current block's MFMAs
// and stored into the other buffer between the MFMAs of the block's last chunk, one barrier per block.  Every element of A and B is
// fetched from global memory once per workgroup tile.  An LDS row is 129 words apart from the next, so the 32 lanes of an operand
// fragment (32 rows, one k) read 32 different banks.  The loads are float4 where both base addresses and both leading dimensions
// keep every row on 16 bytes (WIDE), single words otherwise; rows past m / n are zeros on their way into LDS and are never stored;
// there is no re-layout copy and only the m x n view of C is written.  There is no short-k form: a k below one block runs the last
// block's path alone.
//
// Measured (scripts/bench_mm_nt.py, profiles/mm_nt_bench.json; profiles/mm_nt_pmc_SQ.txt): 81 TFLOP/s = 0.52 of the fp32 MFMA peak at
// 4096^3 against the NN kernel's 0.73, the matrix pipe 0.58 busy, the waves in s_waitcnt for 0.60 of their cycles and for LDS in
// 0.02 of them.  Blocks of 64 k instead of 128: 6 % slower.  The next chunk's LDS reads two behind each MFMA instead of ahead of the
// chunk, and the next block's global loads behind the MFMAs of chunk 0 instead of ahead of them: each within 4 %, not kept.  Rows 32
// floats further apart than 16 KB: the same time.  What the waves wait for is not separated further.
//
// Epilogue.  The eight pair tiles are added element-wise in group_tree16's pairing -- (l, l + 8): the instruction's two blocks;
// (l, l + 4); (l, l + 2); (0, 1).  The up to fifteen k behind the last full chunk are staged in LDS once (64 rows x 16 words of each
// operand) and added by the vector ALU: a lane holds sixteen elements of one column of C, so its B words are its own and its A
// words are broadcasts.
#include "cf_device.hpp"
#include "sgemm_internal.hpp"

using namespace gorse;

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x32 __attribute__((ext_vector_type(32)));

constexpr int kNtTile = 64;                  // rows of A and of B per workgroup
constexpr int kNtKB = 128;                   // k per LDS block
constexpr int kNtChunks = kNtKB / 16;        // 16-chunks per block
constexpr int kNtRow = kNtKB + 1;            // words from one LDS row to the next
constexpr int kNtOperand = kNtTile * kNtRow;  // words of one operand's block
constexpr int kNtTailRow = 17;
constexpr int kNtWords = kNtTile * kNtKB / kBlock;  // words of one operand's block per thread
constexpr size_t kNtLdsBytes = (size_t)2 * 2 * kNtOperand * sizeof(float);  // 132,096 of a CU's 160 KB: two buffers of two operands
static_assert(kNtKB % 64 == 0 && kNtWords % 8 == 0, "the load mapping takes a block in halves of 64 k; the stores go behind eight MFMAs");
static_assert(2 * kNtTile * kNtTailRow <= 2 * 2 * kNtOperand, "the tail staging reuses the block buffers");

template <bool WIDE>
__global__ __launch_bounds__(kBlock) void sgemm_nt_mfma_kernel(int m, int n, int k, int tiles_n, const float *__restrict__ a, int lda,
                                                               const float *__restrict__ b, int ldb, float *__restrict__ c, int ldc) {
    extern __shared__ __attribute__((aligned(16))) float smem[];  // [2][A block | B block]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int col = lane & 31, hb = lane >> 5;  // the lane's row of an operand fragment; its block of the instruction
    const int i0 = (int)(blockIdx.x / tiles_n) * kNtTile, j0 = (int)(blockIdx.x % tiles_n) * kNtTile;
    const int wi = 32 * (wv >> 1), wj = 32 * (wv & 1);
    const VecShape vs(k);
    const int kbody = 16 * vs.nfull;

    // a thread's kNtWords words of each operand block, in units of NW words (WIDE: a float4): unit e is row lr + RS (e % NR), words
    // lc + 64 (e / NR) ..; sixteen lanes (WIDE) or a wave read contiguous bytes of one row, and a wave's stores of one word index go
    // to 32 different LDS banks twice
    constexpr int NW = WIDE ? 4 : 1, NR = WIDE ? 4 : 16, RS = kNtTile / NR, NU = kNtWords / NW;
    const int lr = WIDE ? tid >> 4 : tid >> 6, lc = WIDE ? 4 * (tid & 15) : tid & 63;
    float ra[kNtWords], rb[kNtWords];
    auto gload = [&](int l0) {  // (kbody is a multiple of 16, lc of NW: a float4 lies inside the body or outside it)
#pragma unroll
        for (int e = 0; e < NU; e++) {
            const int ar = i0 + lr + RS * (e % NR), br = j0 + lr + RS * (e % NR), l = l0 + lc + 64 * (e / NR);
            const bool live = l < kbody;
            if constexpr (WIDE) {
                float4 va = make_float4(0.f, 0.f, 0.f, 0.f), vb = va;
                if (live && ar < m) va = *reinterpret_cast<const float4 *>(a + (int64_t)ar * lda + l);
                if (live && br < n) vb = *reinterpret_cast<const float4 *>(b + (int64_t)br * ldb + l);
                ra[4 * e] = va.x, ra[4 * e + 1] = va.y, ra[4 * e + 2] = va.z, ra[4 * e + 3] = va.w;
                rb[4 * e] = vb.x, rb[4 * e + 1] = vb.y, rb[4 * e + 2] = vb.z, rb[4 * e + 3] = vb.w;
            } else {
                ra[e] = live && ar < m ? a[(int64_t)ar * lda + l] : 0.0f;
                rb[e] = live && br < n ? b[(int64_t)br * ldb + l] : 0.0f;
            }
        }
    };
    auto lstore = [&](int buf, int first, int count) {  // the thread's words first .. first + count - 1 of each operand
        float *as = smem + buf * 2 * kNtOperand, *bs = as + kNtOperand;
#pragma unroll
        for (int x = first; x < first + count; x++) {
            const int e = x / NW, w = x % NW, at = (lr + RS * (e % NR)) * kNtRow + lc + 64 * (e / NR) + w;
            as[at] = ra[x];
            bs[at] = rb[x];
        }
    };

    f32x32 acc[8];  // acc[l]: AVX lanes l (registers 0 .. 15) and l + 8 (16 .. 31) of the wave's 32 x 32 elements
#pragma unroll
    for (int l = 0; l < 8; l++)
#pragma unroll
        for (int r = 0; r < 32; r++) acc[l][r] = -0.0f;
    // A chunk is chain step ch of all sixteen lanes: eight MFMAs.  The lane's fragment words are A[wi + col][16 ch + 8 hb + l] and
    // B[wj + col][16 ch + 8 hb + l], l = 0 .. 7.  The words of chunk ch + 1 are read from LDS BEFORE the MFMAs of chunk ch are issued
    // (two sets of fragment registers), and scheduling barriers keep the compiler from sinking each read to its use: with one wave
    // per SIMD nobody else covers an LDS round trip between two MFMAs.
    const float *frag_a = smem + (wi + col) * kNtRow + 8 * hb, *frag_b = smem + kNtOperand + (wj + col) * kNtRow + 8 * hb;
    float fa[2][8], fb[2][8];
    auto fetch = [&](int set, int buf, int ch) {
#pragma unroll
        for (int l = 0; l < 8; l++) {
            fa[set][l] = frag_a[buf * 2 * kNtOperand + 16 * ch + l];
            fb[set][l] = frag_b[buf * 2 * kNtOperand + 16 * ch + l];
        }
    };
    auto step = [&](int set, int l) { acc[l] = __builtin_amdgcn_mfma_f32_32x32x1f32(fa[set][l], fb[set][l], acc[l], 0, 0, 0); };

    const int nblk = (vs.nfull + kNtChunks - 1) / kNtChunks;
    gload(0);
    lstore(0, 0, kNtWords);
    __syncthreads();
    int p = 0;
    for (int blk = 0; blk + 1 < nblk; blk++, p ^= 1) {  // (a block with a successor is full)
        gload((blk + 1) * kNtKB);
        fetch(0, p, 0);
#pragma unroll
        for (int ch = 0; ch < kNtChunks; ch++) {
            if (ch + 1 < kNtChunks) fetch((ch + 1) & 1, p, ch + 1);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int l = 0; l < 8; l++) {
                step(ch & 1, l);
                if (ch + 1 == kNtChunks) {
                    // the next block goes into the other buffer (everybody left it before the barrier of the block before) between the
                    // block's last MFMAs: an eighth of the thread's words behind each, the stores issue while the matrix pipe works
                    lstore(p ^ 1, kNtWords / 8 * l, kNtWords / 8);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();
    }
    {   // the last block: only the chunks that exist, 1 .. kNtChunks
        const int nch = vs.nfull - kNtChunks * (nblk - 1);
        fetch(0, p, 0);
#pragma unroll
        for (int ch = 0; ch < kNtChunks; ch++) {
            if (ch < nch) {
                if (ch + 1 < nch) fetch((ch + 1) & 1, p, ch + 1);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int l = 0; l < 8; l++) step(ch & 1, l);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        __syncthreads();
    }

    // group_tree16 on whole tiles, depth-first: ((0 + 4) + (2 + 6)) + ((1 + 5) + (3 + 7)), each operand a pair sum l + (l + 8)
    float s[16];
#pragma unroll
    for (int r = 0; r < 16; r++) {
        float t[8];
#pragma unroll
        for (int l = 0; l < 8; l++) t[l] = acc[l][r] + acc[l][16 + r];
        s[r] = ((t[0] + t[4]) + (t[2] + t[6])) + ((t[1] + t[5]) + (t[3] + t[7]));
    }

    const int tl = k - kbody;  // 0 .. 15 words of every row behind the body
    if (tl > 0) {  // (the loop's last barrier is behind every fragment read: the buffers are free)
        float *ta = smem, *tb = smem + kNtTile * kNtTailRow;
#pragma unroll
        for (int e = 0; e < kNtTile * 16 / kBlock; e++) {
            const int x = tid + kBlock * e, row = x >> 4, w = x & 15;
            ta[row * kNtTailRow + w] = w < tl && i0 + row < m ? a[(int64_t)(i0 + row) * lda + kbody + w] : 0.0f;
            tb[row * kNtTailRow + w] = w < tl && j0 + row < n ? b[(int64_t)(j0 + row) * ldb + kbody + w] : 0.0f;
        }
        __syncthreads();
        const float *bt = tb + (wj + col) * kNtTailRow;
        const float *at = ta + (wi + 4 * hb) * kNtTailRow;  // element r of the lane: tile row 4 hb + (r & 3) + 8 (r >> 2)
        if (vs.has8) {  // eight unfused products in group_tree8's pairing: ((0 + 4) + (2 + 6)) + ((1 + 5) + (3 + 7))
            float b8[8];
#pragma unroll
            for (int e = 0; e < 8; e++) b8[e] = bt[e];
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const float *arow = at + ((r & 3) + 8 * (r >> 2)) * kNtTailRow;
                float q[8];
#pragma unroll
                for (int e = 0; e < 8; e++) q[e] = arow[e] * b8[e];
                s[r] += ((q[0] + q[4]) + (q[2] + q[6])) + ((q[1] + q[5]) + (q[3] + q[7]));
            }
        }
        for (int e = vs.tail0 - kbody; e < tl; e++) {  // the scalar tail, in element order
            const float bv = bt[e];
#pragma unroll
            for (int r = 0; r < 16; r++) s[r] = fmaf(at[((r & 3) + 8 * (r >> 2)) * kNtTailRow + e], bv, s[r]);
        }
    }

    const int cj = j0 + wj + col;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int ci = i0 + wi + 4 * hb + (r & 3) + 8 * (r >> 2);
        if (ci < m && cj < n) c[(int64_t)ci * ldc + cj] = s[r];
    }
}

template <bool WIDE>
int32_t launch(hipStream_t st, int m, int n, int k, const float *a, int lda, const float *b, int ldb, float *c, int ldc) {
    GORSE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&sgemm_nt_mfma_kernel<WIDE>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)kNtLdsBytes));
    const int64_t tiles_n = ceil_div(n, kNtTile), tiles = ceil_div(m, kNtTile) * tiles_n;
    sgemm_nt_mfma_kernel<WIDE><<<dim3((unsigned)tiles), dim3(kBlock), kNtLdsBytes, st>>>(m, n, k, (int)tiles_n, a, lda, b, ldb, c, ldc);
    GORSE_HIP_CHECK(hipGetLastError());
    return GORSE_OK;
}

}  // namespace

namespace gorse {

int32_t sgemm_nt_mfma_launch(hipStream_t st, int m, int n, int k, const float *a, int lda, const float *b, int ldb, float *c, int ldc) {
    if (!sgemm_nt_mfma_serves(m, n, k)) return fail(GORSE_ERR_INVALID, "the NT matrix-core kernel does not serve %d x %d x %d", m, n, k);
    // float4 loads only where every row of both operands starts on 16 bytes
    const bool wide = (((uintptr_t)a | (uintptr_t)b) & 15) == 0 && lda % 4 == 0 && ldb % 4 == 0;
    return wide ? launch<true>(st, m, n, k, a, lda, b, ldb, c, ldc) : launch<false>(st, m, n, k, a, lda, b, ldb, c, ldc);
}

}  // namespace gorse
