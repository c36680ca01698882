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
#include "topk_deep_body.hpp"

using namespace gorse;
using namespace gorse::topk_deep_plan;

namespace {

// the K-loop lives in topk_deep_body.hpp, which the history form (topk_deep_hist.hip) shares
// BIAS: the row value is added to the score (Euclidean), else multiplied (cosine's scale; 1 for -dot, where only its NaN matters)
template <bool BIAS>
__global__ __launch_bounds__(kThreads) void topk_deep_sweep_kernel(SweepParams p, int kpad) {
    topk_deep_body::deep_sweep_body<BIAS, false>(p, kpad);
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
