// topk_internal.hpp -- the gorse_topk handle shared by topk.hip (path A: exact VALU scan + literal
// heaps) and topk_mfma.hip with its units topk_sweep / topk_rescore / topk_tie / topk_tri.hip (path B: bf16 MFMA candidate sweep + exact
// rescoring; topk_mfma_internal.hpp is what those units share).
#pragma once
#include "cf_device.hpp"

#define GORSE_PROF_TOPK_NCLASSES 6

namespace gorse {
struct TopkChunkState;  // topk_mfma_internal.hpp: what the stages of one chunk of an MFMA search share
}

struct gorse_topk {
    int device = 0;
    int64_t N = 0;
    int d = 0, dtype = 0, metric = 0;
    hipStream_t stream = nullptr;
    gorse::DevBuf<float> X;       // N x d fp32 (bf16 inputs are expanded by <<16, bfloats.go:32-38)
    gorse::DevBuf<uint16_t> Xb;   // N x d bf16 as given
    gorse::DevBuf<float> norm2;   // floats.Dot(x, x) per stored vector
    gorse::DevBuf<float> qbuf, qnorm, dist;
    gorse::DevBuf<int64_t> qidx;
    gorse::DevBuf<int32_t> out_idx, out_cnt, heap_v, scan_literal;
    gorse::DevBuf<float> out_dist, heap_w;
    // ---- path B (topk_mfma.hip and its units) ----
    bool mfma_ok = false;          // operands built and the data admits a rigorous error bound
    int kp = 0;                    // k-steps of 16 of the MFMA operands (KPAD = 16 * kp)
    float err_coef = 0.0f;         // |approx - reference| <= err_coef * |q| * |x| (dot of the operands)
    float max_norm = 0.0f;         // max_i sqrt(norm2[i])
    bool coarse_ok = false;        // cosine with nearly equal norms: block-level scale bound in the sweep
    float rs_min = 0.0f, rs_max = 0.0f;  // cosine: bounds of the row scales 1 / sqrt(norm2[i]) (the DMA sweeps' block bound)
    gorse::DevBuf<uint16_t> opA_own, opB_own;  // bf16 operand matrices N x KPAD (candidate / query roles)
    const uint16_t *opA = nullptr, *opB = nullptr;  // may alias Xb
    gorse::DevBuf<float> rscale;   // the sweep's per-row value: cosine 1 / sqrt(norm2[i]), Euclidean -norm2[i] / 2, -dot 1; N + kTopkRowPad
                                   // entries, the padding NaN (what the sweep's tiles read for the rows past N)
    gorse::DevBuf<uint16_t> opQ;   // query operands of the current chunk when they are not rows of opB
    gorse::DevBuf<float> qn2, qmargin, qf32;
    gorse::DevBuf<int64_t> qid;
    gorse::DevBuf<uint2> cbuf;     // per query: kCap (approx key, candidate index) entries
    gorse::DevBuf<int32_t> ccnt;
    gorse::DevBuf<uint8_t> cflag;
    gorse::DevBuf<int32_t> res_idx, res_cnt;
    gorse::DevBuf<float> res_dist;
    // tie replay (history sweep of the flagged queries + topk_tie_sort_kernel + topk_tie_replay_lane_kernel)
    gorse::DevBuf<int32_t> rp_pos, rp_ccnt, rp_hcnt, fl_pos;  // fl_*: the chunk's flagged queries, listed on the device (flag_compact_kernel)
    gorse::DevBuf<int64_t> fl_self;
    gorse::DevBuf<long long> fl_cnt;
    gorse::DevBuf<int64_t> rp_self;
    gorse::DevBuf<uint16_t> rp_op;
    gorse::DevBuf<float> rp_margin, rp_fslice;  // rp_fslice: final threshold of every (row slice, query) of a history sweep
    gorse::DevBuf<float> rp_fwarm;              // starting threshold of every (row slice, query) of a history sweep (tie_warm_kernel)
    gorse::DevBuf<uint2> rp_cbuf, rp_hbuf;
    gorse::DevBuf<uint8_t> rp_flag;
    gorse::DevBuf<int32_t> rp_sidx, rp_scount;
    gorse::DevBuf<float> rp_sdst;
    gorse::DevBuf<unsigned long long> sweep_prof;  // counters of the tie replay (GORSE_TEST_TOPK_REPLAY_COUNTERS, gorse_hip_test_get_sweep_profile)
    gorse::KernelProfile prof{GORSE_PROF_TOPK_NCLASSES};
    // gorse_topk_set_mask: rows with mask == 0 take no part in any search (as if they had never been added)
    gorse::DevBuf<uint8_t> mask;
    gorse::DevBuf<float> rscale_m;  // the sweep's per-row value (cosine scale / Euclidean bias / 1 for -dot) with NaN for masked rows
    bool has_mask = false;
    int64_t n_admissible = 0;
    bool bf16_order = false;  // GORSE_METRIC_EUCLIDEAN_BF16: metric is kept as GORSE_METRIC_EUCLIDEAN, the distance kernels get id 3
    int kernel_metric() const { return bf16_order ? 3 : metric; }
    int64_t n_fallback = 0, n_tie = 0, n_resweep = 0;  // of the last search: path A rows, tie replays, warm starts swept again
    gorse::DevBuf<float> f0, f1;                       // warm-start thresholds of a chunk (topk_mfma_search): pilot, pre-pilot
    // the symmetric all-pairs sweep (topk_sweep.hip, SYM): per query a foreign candidate list and its counter, the raw-score form
    // of the thresholds; last_sym: did the last search's (last chunk's) main sweep take the symmetric form
    gorse::DevBuf<uint2> fbuf;
    gorse::DevBuf<int32_t> fcnt;
    gorse::DevBuf<float> f0raw;
    gorse::DevBuf<unsigned long long> sym_stats;  // counters of the last symmetric search (gorse_hip_test_topk_sym_stats)
    bool last_sym = false;
    // the state of the search in progress (topk_mfma_internal.hpp: TopkChunkState): its stages run back to back in topk_mfma_search, call by call in the
    // triangle-sharded search (gorse_topk_tri_*), whose message buffers follow
    gorse::TopkChunkState *cstate = nullptr;
    gorse::TopkChunkState *chunk_state();
    gorse::DevBuf<int32_t> tri_counts, tri_in_counts;
    gorse::DevBuf<long long> tri_offsets;
    gorse::DevBuf<uint2> tri_entries, tri_in_entries;
    int64_t tri_packed_counts = 0, tri_packed_entries = 0;
    // test hook (gorse_hip_test_topk_scan_flags): the last block of the last call's scan -- its queries (0: the call did not scan),
    // whether the literal-only switch was on, and, where the host read the flags for the reroute (whose replay may scan again
    // and overwrite scan_literal), the flags as it read them
    int64_t scan_last_nq = 0;
    bool scan_last_literal_only = false, scan_flags_on_host = false;
    std::vector<int32_t> scan_flags_host;
    int32_t use() const {
        hipError_t e = hipSetDevice(device);
        if (e != hipSuccess) return gorse::fail(GORSE_ERR_HIP, "hipSetDevice(%d): %s", device, hipGetErrorString(e));
        return GORSE_OK;
    }
};

namespace gorse {
constexpr int64_t kTopkRowPad = 256;  // NaN entries behind the last row value: one tile of the sweep reaches at most 127 rows past N
// A NaN operand of a subtraction: the reference's vsubps / subss return it as it is (the first operand's when both are NaN);
// v_sub_f32 computes a + (-b) and hands back a NaN b with its sign flipped (measured on an MI355X: 1.0f - NaN(7fc00000) =
// ffc00000; sqrtf, products and quotients keep the sign).  NAN_SUB = true restores the operand.  The distance functions below run
// their plain form and, only when the result is a NaN, once more in this form: a finite pair pays one comparison.
template <bool NAN_SUB>
__device__ __forceinline__ float ref_sub(float a, float b) {
    const float v = a - b;
    if (NAN_SUB && v != v) return a != a ? a : (b != b ? b : v);
    return v;
}
// 1 - ab / (|q| |x|) of the cosine distance: a NaN quotient is the result
__device__ __forceinline__ float cosine_distance(float ab, float qq, float n2) {
    const float t = ab / (sqrtf(qq) * sqrtf(n2));
    const float r = 1.0f - t;
    return t != t ? t : r;
}

// floats.Euclidean (squared part) in AVX512 order for rows staged in LDS: floats_avx512.c:374-441
template <bool NAN_SUB = false>
__device__ __forceinline__ float euclid512_lds(const float *a, const float *b, const VecShape &vs, int lane) {
    float acc = 0.0f;
    for (int c = 0; c < vs.nfull; c++) {
        float v = ref_sub<NAN_SUB>(a[16 * c + lane], b[16 * c + lane]);
        v = v * v;
        acc = c == 0 ? v : v + acc;
    }
    float sum = group_tree16(acc);
    if (vs.has8) {
        int e = vs.nfull * 16 + (lane & 7);
        float v = ref_sub<NAN_SUB>(a[e], b[e]);
        sum += group_tree8(v * v);
    }
    for (int e = vs.tail0; e < vs.d; e++) {
        float v = ref_sub<NAN_SUB>(a[e], b[e]);
        sum = fmaf(v, v, sum);
    }
    return sqrtf(sum);
}

// bfloats.Euclidean (squared part) in the order of the reference's AVX512BW kernel (common/bfloats/src/bfloats_avx512.c:26-59 as
// shipped in bfloats_avx512.s, restated by the oracle's orc_bf16_euclidean): rows are the bf16 values expanded by << 16;
// sixteen partial sums with UNFUSED multiply + add, the partials added SEQUENTIALLY (a vaddss chain, not the shuffle tree of
// floats.Euclidean), the n % 16 tail one element at a time with a fused multiply-add.
template <bool NAN_SUB = false>
__device__ __forceinline__ float euclid_bf16_lds(const float *a, const float *b, int d, int lane) {
    const int nfull = d / 16;
    float acc = 0.0f;
    for (int c = 0; c < nfull; c++) {
        const float v = ref_sub<NAN_SUB>(a[16 * c + lane], b[16 * c + lane]);
        acc = acc + v * v;  // -ffp-contract=off: two roundings, as vmulps + vaddps
    }
    float sum = 0.0f;
    const int base = threadIdx.x & ~15;  // first lane of this 16-lane group inside its wave
#pragma unroll
    for (int l = 0; l < 16; l++) sum = sum + __shfl(acc, (base & 63) + l, 64);
    for (int e = 16 * nfull; e < d; e++) {
        const float v = ref_sub<NAN_SUB>(a[e], b[e]);
        sum = fmaf(v, v, sum);
    }
    return sqrtf(sum);
}
// the distance of `metric` (GORSE_METRIC_EUCLIDEAN or the kernels' own id 3 = bfloats order) for rows staged in LDS
constexpr int kMetricEuclidBf16 = 3;
__device__ __forceinline__ float euclid_any_lds(int metric, const float *a, const float *b, const VecShape &vs, int lane) {
    const float r = metric == kMetricEuclidBf16 ? euclid_bf16_lds(a, b, vs.d, lane) : euclid512_lds(a, b, vs, lane);
    if (r == r) return r;  // every lane of the 16-lane group holds the same total: the group takes the second run together
    return metric == kMetricEuclidBf16 ? euclid_bf16_lds<true>(a, b, vs.d, lane) : euclid512_lds<true>(a, b, vs, lane);
}

// Whoever takes a search's results where they lie: after each finished block (a chunk of the MFMA path, a block of the scan) the
// search hands over the block's device result arrays (m rows of stride k, and m counts) instead of copying them out.  q0 = the
// block's first query in the call's list.  The arrays are the handle's and are overwritten by the next block: what block() launches
// goes on `stream`, the search's own.
struct TopkBlockConsumer {
    virtual int32_t block(int64_t q0, int64_t m, const int32_t *idx, const float *dist, const int32_t *cnt, hipStream_t stream) = 0;

protected:
    ~TopkBlockConsumer() = default;
};

// topk.hip
int32_t topk_compute_norms(gorse_topk *h, const float *V, int64_t n, float *out);
// Stored rows src_host[0 .. nq) as query VECTORS (the row itself is not excluded, as gorse_topk_search_vector does not exclude it),
// prune0 = 0, under the current mask: the same search as the public call on those rows' vectors, gathered on the device from the
// index's fp32 image, every block's results handed to `consumer`.
int32_t topk_search_stored(gorse_topk *h, const int64_t *src_host, int64_t nq, int k, TopkBlockConsumer *consumer);
// path A on queries whose fp32 rows sit in h->qbuf (nq x d) [+ h->qnorm]; qidx_dev = exclusion ids or null (qidx_host: the same
// ids on the host).  Results land in h->out_idx / out_dist / out_cnt and, where given, in the host arrays.  Queries whose answer
// depends on the heap's history (ties among the k + 1 smallest distances, NaN) go to the MFMA path's tie replay where that is
// usable and `reroute` allows it, else to the literal heap kernel.
int32_t topk_scan_block(gorse_topk *h, int64_t nq, const int64_t *qidx_dev, const int64_t *qidx_host, int k, int prune0,
                        int32_t *idx_out, float *dist_out, int32_t *cnt_out, bool reroute = true, bool keep_on_device = false);
// keep_on_device: the rows a reroute answered are written back, so that h->out_* hold the whole block when the call returns
int64_t topk_scan_block_queries(const gorse_topk *h);
// topk_mfma.hip
int32_t topk_mfma_prepare(gorse_topk *h);  // at create: operands, scales, error bound
// Queries: stored vectors qid_host[0..nq) (exclude_self) or, when qid_host is NULL and qv_dev is given, nq fp32
// query vectors already on the device.  Host outputs may be NULL.
int32_t topk_mfma_search(gorse_topk *h, const int64_t *qid_host, int64_t q_contig_begin, const float *qv_dev,
                         int64_t nq, int k, int prune0, int32_t *idx_out, float *dist_out, int32_t *cnt_out,
                         TopkBlockConsumer *consumer = nullptr);
bool topk_mfma_usable(const gorse_topk *h, int64_t nq, int k);
void topk_mfma_release(gorse_topk *h);  // at destroy: the search state
extern int g_topk_variant;     // OR of the GORSE_TEST_TOPK_* switches (include/gorse_hip_test.h): every read names one; 0 in the product
extern int g_topk_force_path;  // 0 auto, 1 path A only, 2 path B whenever it is usable, 3 = 2 without the tie replay
}  // namespace gorse
