// topk_deep_hist.hip -- the HISTORY form of the deep sweep of path B (topk_mfma.hip says what the path is, topk_tie.hip what a
// history sweep is for): the first stage of the tie path of a deep handle (gorse_topk_set_deep_tie_replay), for operands of 25
// k-steps and more.  Without it the queries with equal distances among their k + 1 best go to the literal scan, one thread per query
// over all N rows.
//
// The K-loop is the main deep sweep's (topk_deep_body.hpp; topk_deep.hip's head describes it): four waves, one per SIMD, 128-row
// tiles, K-slices of 64 bf16 values brought in by global_load_lds_dwordx4 with the XOR swizzle on the source address and on the
// read, three slices resident, one barrier per slice, counted s_waitcnt vmcnt(n) in inline assembly, the tile's row values riding in
// front of its first slice, accumulators read only by compiler-emitted code, one writer per candidate list.  What it leaves is the
// shallow history sweep's contract in full (topk_sweep_kernel<..., HIST>; listed at the head of topk_deep_body.hpp), so SweepParams,
// compact_query<true>, tie_warm_kernel and everything behind them -- topk_tie_sort_kernel's join of the slices, the exact distances,
// the lane replay -- work against it unchanged.
//
// The shape differs from the main sweep's in one figure (topk_deep_hist_plan.hpp has the reasons and the constants): 128 queries per
// workgroup.  A wave owns one 32-query column block and all four 32-row blocks of the tile -- 64 accumulators per lane -- and row
// slices (grid.y) supply the parallelism a chunk of a few hundred flagged queries lacks.  The slice image is (128 + 128) x 128 B =
// 32 KB, three of them 96 KB; a wave issues 4 + 4 DMA instructions per slice, so vmcnt(8) leaves exactly one slice in flight.
//
// Exactness: topk_deep.hip's argument carries over as it stands -- the error bound does not depend on how the K' products are
// grouped, and this kernel groups them exactly as the main form does.
#include "topk_deep_body.hpp"

using namespace gorse;
using namespace gorse::topk_deep_hist_plan;

namespace {

// BIAS: the row value is added to the score (Euclidean), else multiplied (cosine's scale; 1 for -dot, where only its NaN matters)
template <bool BIAS>
__global__ __launch_bounds__(kThreads) void topk_deep_hist_kernel(SweepParams p, int kpad) {
    topk_deep_body::deep_sweep_body<BIAS, true>(p, kpad);
}

template <bool BIAS>
int32_t launch_deep_hist(gorse_topk *h, const SweepParams &p) {
    const size_t lds = hist_lds_bytes();
    GORSE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&topk_deep_hist_kernel<BIAS>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    topk_deep_hist_kernel<BIAS><<<dim3((unsigned)ceil_div(p.nq, kHistQueries), (unsigned)p.nslices), dim3(kThreads), lds, h->stream>>>(p, h->kp * 16);
    GORSE_HIP_CHECK(hipGetLastError());
    return GORSE_OK;
}

}  // namespace

// the history sweep of a deep handle: p.nslices row slices over the p.nq flagged queries of a replay chunk
int32_t gorse::dispatch_deep_hist_sweep(gorse_topk *h, const SweepParams &p) {
    if (p.nq <= 0) return GORSE_OK;
    if (h->kp * 16 % kSlice != 0 || h->kp * 16 < 2 * kSlice)  // (a tile's row values are issued two slices ahead: at least two per tile)
        return fail(GORSE_ERR_INVALID, "deep operand depth %d is not whole K-slices", h->kp * 16);
    if (p.nslices < 1 || p.nslices > kMaxSlicesFew || p.tile_stride != 1 || p.f0 || !p.hbuf || !p.hcnt)
        return fail(GORSE_ERR_INVALID, "not a history sweep's parameters (%d slices, tile stride %d)", p.nslices, p.tile_stride);
    return p.ep == EP_BIAS ? launch_deep_hist<true>(h, p) : launch_deep_hist<false>(h, p);
}
