// topk_mfma.hip -- path B of the exact top-k: a bf16 MFMA candidate sweep followed by exact rescoring.
// Reference semantics: common/ann/bruteforce.go:39-83 (keep the k smallest distances, return them ascending),
// distances computed by floats.Dot in AVX512 order (common/floats/src/floats_avx512.c:306-367).
//
// The reference scores all N vectors per query one pair at a time.  Here the N x nq score matrix is produced
// by v_mfma_f32_32x32x16_bf16 tiles and never leaves the CU: every wave keeps the operands of its 32*NCB queries
// in registers for the whole sweep, candidate rows stream through LDS, and the epilogue only compares the 16
// scores a lane holds (all of ONE query: the C layout puts a query per column) against that query's running
// filter threshold.  Scores that pass are appended to a small per-query candidate list in HBM; when a list
// fills, its wave raises the threshold to (K-th best approximate score so far) - margin and compacts the list.
//
// Exactness: |approx - reference| <= delta_q for every pair of one query (delta_q from a forward error bound
// of both summation orders, see topk_mfma_prepare).  Any vector whose reference score is among the K best has an
// approximate score >= (final K-th best approximate score) - 2*delta_q >= every threshold used during the sweep,
// so it is in the list.  The list is then rescored in the reference's own arithmetic order and ranked; a query
// whose K+1 best exact distances are not all distinct (where the reference's result depends on container/heap
// mechanics), whose list overflowed, or that saw a NaN is handed to path A (topk.hip), which replays the
// reference's heaps literally.  Results are therefore identical to path A's, ties included.
//
// This unit is the path's driver: operand construction and the error bound (topk_mfma_prepare), and a search as chunks of queries,
// each through its stages -- operands and margins, pilot sweeps, the main sweep (topk_sweep.hip), rescoring (topk_rescore.hip), the
// tie path for what that leaves undecided (topk_tie.hip), the literal scan (topk.hip) for what THAT leaves.  topk_tri.hip runs the
// same stages call by call; topk_mfma_internal.hpp is what the units share, topk_plan.hpp the rules the host decides by.
#include "topk_mfma_internal.hpp"

using namespace gorse;

namespace gorse {
int g_topk_force_path = 0;
int g_topk_variant = 0;  // OR of the GORSE_TEST_TOPK_* switches (include/gorse_hip_test.h)
}

namespace {

// ---- operand construction ------------------------------------------------------------------------------
__device__ __forceinline__ uint16_t bf16_rne(float x) {
    uint32_t b = __float_as_uint(x);
    b += 0x7fffu + ((b >> 16) & 1u);
    return (uint16_t)(b >> 16);
}
__device__ __forceinline__ float bf16_f32(uint16_t h) { return __uint_as_float((uint32_t)h << 16); }

// fp32 rows -> [hi | lo | hi] (role 0, candidates) or [hi | hi | lo] (role 1, queries), zero padded to kpad:
// sum over the operand = hi.hi + lo.hi + hi.lo, the three leading terms of the split product.
__global__ void split_f32_kernel(const float *__restrict__ X, int64_t n, int d, int kpad, int role,
                                 uint16_t *__restrict__ out) {
    const int64_t total = n * kpad;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = t / kpad;
        const int e = (int)(t % kpad);
        uint16_t v = 0;
        if (e < 3 * d) {
            const int part = e / d, j = e % d;
            const float x = X[row * d + j];
            const uint16_t hi = bf16_rne(x);
            const bool want_lo = role == 0 ? part == 1 : part == 2;
            v = want_lo ? bf16_rne(x - bf16_f32(hi)) : hi;
        }
        out[t] = v;
    }
}
// bf16 rows (or fp32 rows that hold bf16 values exactly) -> zero padded bf16 operand rows
__global__ void pad_bf16_kernel(const uint16_t *__restrict__ Xb, const float *__restrict__ Xf, int64_t n, int d,
                                int kpad, uint16_t *__restrict__ out) {
    const int64_t total = n * kpad;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = t / kpad;
        const int e = (int)(t % kpad);
        uint16_t v = 0;
        if (e < d) v = Xb ? Xb[row * d + e] : (uint16_t)(__float_as_uint(Xf[row * d + e]) >> 16);
        out[t] = v;
    }
}
__global__ void rscale_kernel(const float *__restrict__ norm2, int64_t n, float *__restrict__ out) {
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x)
        out[t] = 1.0f / sqrtf(norm2[t]);
}
// gather operand rows / norms of stored vectors for an id list
__global__ void gather_queries_kernel(const uint16_t *__restrict__ opB, const float *__restrict__ norm2,
                                      const int64_t *__restrict__ qid, int64_t nq, int kpad,
                                      uint16_t *__restrict__ opQ, float *__restrict__ qn2) {
    const int64_t t = blockIdx.x;
    const int64_t src = qid[t];
    const uint4 *s = reinterpret_cast<const uint4 *>(opB + src * kpad);
    uint4 *o = reinterpret_cast<uint4 *>(opQ + t * kpad);
    for (int e = threadIdx.x; e < kpad / 8; e += blockDim.x) o[e] = s[e];
    if (threadIdx.x == 0) qn2[t] = norm2[src];
}
// Euclidean: score = q.x - |x|^2 / 2 stands for (|q|^2 - d^2) / 2 with d = the reference's floats.Euclidean.  Its error
// against that quantity: the dot product's (coef |q| |x|), the fp32 norm in the bias (d u |x|^2 / 2) and the
// reference's own rounding of the sum of squares and the square root ((d + 8) u (|q| + |x|)^2 / 2); margin = 2 x that.
__global__ void margin_euclid_kernel(const float *__restrict__ qn2, int64_t nq, float coef, float xmax, float du,
                                     float *__restrict__ out) {
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < nq; t += (int64_t)gridDim.x * blockDim.x) {
        const float qn = sqrtf(qn2[t]);
        const float u = 5.9604645e-8f;  // 2^-24; the + 4u also covers the rounding of the bias addition itself
        const float delta = coef * qn * xmax + 0.5f * (du + 4.0f * u) * xmax * xmax + 0.5f * (du + 8.0f * u) * (qn + xmax) * (qn + xmax);
        out[t] = 2.0f * delta * 1.01f + 1e-30f;
    }
}
__global__ void bias_kernel(const float *__restrict__ norm2, int64_t n, float *__restrict__ out) {
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x)
        out[t] = -0.5f * norm2[t];
}
__global__ void margin_kernel(const float *__restrict__ qn2, int64_t nq, float coef, float other,
                              float *__restrict__ out) {
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < nq; t += (int64_t)gridDim.x * blockDim.x)
        out[t] = 2.0f * coef * sqrtf(qn2[t]) * other * 1.001f + 1e-30f;
}

// SYM: the pilot's thresholds as the main sweep's foreign side uses them.  A query the pilot could not give a threshold (-inf)
// would make every column of every block a foreign candidate: it gets +inf instead -- nothing is collected for it, neither by
// its own workgroup nor by the others -- and the flag that sends it to the tie path's sweep from -inf.  raw = the form the
// RAWF test compares raw scores with (topk_sweep_kernel's raw_threshold), or null.
__global__ void sym_thresholds_kernel(float *__restrict__ f0, float *__restrict__ raw, uint8_t *__restrict__ cflag, int64_t n,
                                      float rs_min, float rs_max, unsigned long long *__restrict__ stats) {
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
        float f = f0[t];
        if (f == -__builtin_inff()) {
            f = __builtin_inff();
            f0[t] = f;
            cflag[t] = 2;
        }
        if (raw) {
            const float q = f / (f > 0.0f ? rs_max : rs_min);
            raw[t] = fabsf(q) == __builtin_inff() ? q : q - fabsf(q) * 2.4e-7f;
        }
    }
}

__global__ void pilot_unset_count_kernel(const float *__restrict__ f0, int64_t n, unsigned long long *__restrict__ stats) {
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x)
        if (f0[t] == -__builtin_inff()) {
            atomicAdd(stats + 0, 1ull);  // the search's total
            atomicAdd(stats + 4, 1ull);  // this chunk's
        }
}

__global__ void fill_kernel(float *__restrict__ out, int64_t n, float v) {
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) out[t] = v;
}

}  // namespace

namespace gorse {

bool topk_mfma_usable(const gorse_topk *h, int64_t nq, int k) {
    if (!h->mfma_ok || g_topk_force_path == 1) return false;
    if (k + 1 > kMaxKth) return false;
    // Below ~800 queries the scan (path A: distances in the reference's order, select_fast_kernel) is faster: 0.12 ms per query at
    // N = 1M, against the ~40-100 ms one or two workgroups need to sweep a million rows on their own (profiles/
    // r02_v / r02_w_probe_query_latency.txt: 64 queries 7.4 ms on the scan, 41 ms on the sweep; 512 queries 96 ms on the sweep).
    return g_topk_force_path >= 2 || nq >= kMinSweepQueries;
}

int32_t topk_mfma_prepare(gorse_topk *h) {
    h->mfma_ok = false;
    if (h->metric != GORSE_METRIC_NEG_DOT && h->metric != GORSE_METRIC_COSINE && h->metric != GORSE_METRIC_EUCLIDEAN)
        return GORSE_OK;
    const int64_t N = h->N;
    const int d = h->d;
    const bool bf = h->dtype == GORSE_DTYPE_BF16;
    const int kp = operand_depth(bf, d);
    if (kp == 0) return GORSE_OK;  // too deep for register-resident query operands: path A
    // the error bound needs finite norms (and non-zero ones for cosine, whose reference distance is then NaN)
    std::vector<float> n2((size_t)N);
    GORSE_HIP_CHECK(hipMemcpyAsync(n2.data(), h->norm2.p, (size_t)N * 4, hipMemcpyDeviceToHost, h->stream));
    GORSE_HIP_CHECK(hipStreamSynchronize(h->stream));
    float mx = 0.0f;
    for (float v : n2) {
        if (!(v == v) || std::isinf(v)) return GORSE_OK;
        if (h->metric == GORSE_METRIC_COSINE && !(v > 0.0f)) return GORSE_OK;
        mx = std::max(mx, v);
    }
    h->max_norm = std::sqrt(mx) * 1.0001f;
    {   // cosine: row scales within 2 % of each other -> the block-level bound loses nothing (topk_sweep_kernel)
        float mn2 = std::numeric_limits<float>::infinity();
        for (float v : n2) mn2 = std::min(mn2, v);
        h->coarse_ok = h->metric == GORSE_METRIC_COSINE && mn2 > 0.0f && std::sqrt(mx / mn2) <= 1.02f;
        if (h->metric == GORSE_METRIC_COSINE && mn2 > 0.0f) {  // bounds of 1 / sqrtf(norm2[i]) as the device rounds it
            h->rs_min = (1.0f / std::sqrt(mx)) * (1.0f - 1e-6f);
            h->rs_max = (1.0f / std::sqrt(mn2)) * (1.0f + 1e-6f);
        }
    }
    h->kp = kp;
    const int kpad = kp * 16;
    // forward error of two different summation orders of the same K' exact products (the reference's fp32
    // chain, gamma <= K' u, and the MFMA's, gamma <= 2 K' u allowing truncating adders), plus the fp32 roundings
    // of the cosine formula; fp32 inputs add the dropped lo.lo / residual terms of the RNE split (3 * 2^-16).
    const double u = std::ldexp(1.0, -24);
    double coef = bf ? (3.0 * d + 64.0) * u : (9.0 * d + 64.0) * u + 3.2 * std::ldexp(1.0, -16);
    coef += 16.0 * u;
    h->err_coef = (float)(coef * 1.01);
    if (bf && d == kpad) {
        h->opA = h->opB = h->Xb.p;
    } else {
        GORSE_TRY(h->opA_own.alloc((size_t)N * kpad));
        if (bf) {
            pad_bf16_kernel<<<dim3(2048), dim3(256), 0, h->stream>>>(h->Xb.p, nullptr, N, d, kpad, h->opA_own.p);
            h->opA = h->opB = h->opA_own.p;
        } else {
            GORSE_TRY(h->opB_own.alloc((size_t)N * kpad));
            split_f32_kernel<<<dim3(2048), dim3(256), 0, h->stream>>>(h->X.p, N, d, kpad, 0, h->opA_own.p);
            split_f32_kernel<<<dim3(2048), dim3(256), 0, h->stream>>>(h->X.p, N, d, kpad, 1, h->opB_own.p);
            h->opA = h->opA_own.p;
            h->opB = h->opB_own.p;
        }
        GORSE_HIP_CHECK(hipGetLastError());
    }
    // the per-row value of the sweep's epilogue: cosine 1 / |x|, Euclidean -|x|^2 / 2 (added), -dot 1; kTopkRowPad NaN entries
    // behind it -- a tile of the sweep reaches past N, and a NaN value keeps those rows out of every list
    GORSE_TRY(h->rscale.alloc((size_t)N + kTopkRowPad));
    if (h->metric == GORSE_METRIC_EUCLIDEAN)
        bias_kernel<<<dim3(1024), dim3(256), 0, h->stream>>>(h->norm2.p, N, h->rscale.p);
    else if (h->metric == GORSE_METRIC_COSINE)
        rscale_kernel<<<dim3(1024), dim3(256), 0, h->stream>>>(h->norm2.p, N, h->rscale.p);
    else
        fill_kernel<<<dim3(1024), dim3(256), 0, h->stream>>>(h->rscale.p, N, 1.0f);
    fill_kernel<<<dim3(1), dim3(256), 0, h->stream>>>(h->rscale.p + N, kTopkRowPad, __builtin_nanf(""));
    GORSE_HIP_CHECK(hipGetLastError());
    GORSE_HIP_CHECK(hipStreamSynchronize(h->stream));
    h->mfma_ok = true;
    return GORSE_OK;
}

// the per-query arrays of a sweep restricted to the queries [lo, lo + n) (a pilot over one rank's slice)
static SweepParams slice_params(const SweepParams &sp, int64_t lo, int64_t n, int kpad) {
    SweepParams p = sp;
    p.B = sp.B + lo * (int64_t)kpad;
    p.qmargin = sp.qmargin + lo;
    p.cbuf = sp.cbuf + lo * kCap;
    p.ccnt = sp.ccnt + lo;
    p.cflag = sp.cflag + lo;
    if (sp.f0) p.f0 = sp.f0 + lo;
    p.nq = n;
    return p;
}

int32_t search_setup(gorse_topk *h, ChunkState &cs, const int64_t *qid_host, int64_t q_contig_begin, const float *qv_dev, int64_t nq,
                     int k, int prune0) {
    const int d = h->d, kpad = h->kp * 16;
    cs = ChunkState();
    cs.nq = nq, cs.qid_host = qid_host, cs.q_contig_begin = q_contig_begin, cs.qv_dev = qv_dev, cs.k = k, cs.prune0 = prune0;
    cs.by_vector = qv_dev != nullptr;
    cs.contiguous = !cs.by_vector && qid_host == nullptr;
    const bool exclude_self = !cs.by_vector;
    cs.kth = k + (exclude_self ? 1 : 0);
    // with a mask the query's own row may or may not be admissible: the larger count only sends a query whose list comes out
    // one short (fewer than k admissible rows in all) to path A
    const int64_t admissible = h->has_mask ? h->n_admissible : h->N - (exclude_self ? 1 : 0);
    cs.expect = std::min<int64_t>(k, admissible);
    cs.euclid = h->metric == GORSE_METRIC_EUCLIDEAN;
    cs.other = h->metric == GORSE_METRIC_COSINE ? 1.0f : h->max_norm;
    const int64_t mb = std::min(nq, kChunkQ);
    cs.mb = mb;
    GORSE_TRY(h->cbuf.ensure((size_t)mb * kCap));
    GORSE_TRY(h->ccnt.ensure((size_t)mb));
    GORSE_TRY(h->cflag.ensure((size_t)mb));
    GORSE_TRY(h->qmargin.ensure((size_t)mb));
    GORSE_TRY(h->res_idx.ensure((size_t)mb * k));
    GORSE_TRY(h->res_dist.ensure((size_t)mb * k));
    GORSE_TRY(h->res_cnt.ensure((size_t)mb));
    if (!cs.contiguous) {
        GORSE_TRY(h->opQ.ensure((size_t)mb * kpad));
        GORSE_TRY(h->qn2.ensure((size_t)mb));
    }
    if (qid_host) GORSE_TRY(h->qid.ensure((size_t)mb));
    (void)d;
    h->n_fallback = 0;
    h->n_tie = 0;
    h->n_resweep = 0;
    return GORSE_OK;
}

// stage A: the chunk's query operands, margins and the main sweep's parameters (cs.sp); decides whether the sweep is warm-started
int32_t chunk_prepare(gorse_topk *h, ChunkState &cs) {
    const uint16_t *Bop;
    const float *qn2;
    const float *Qf = nullptr;
    const int64_t m = cs.m, c0 = cs.c0, q_contig_begin = cs.q_contig_begin;
    const int64_t *qid_host = cs.qid_host;
    const float *qv_dev = cs.qv_dev;
    const int d = h->d, kpad = h->kp * 16, kth = cs.kth;
    const bool contiguous = cs.contiguous, euclid = cs.euclid;
    const float other = cs.other;
    if (contiguous) {
        Bop = h->opB + (q_contig_begin + c0) * kpad;
        qn2 = h->norm2.p + q_contig_begin + c0;
    } else if (qid_host) {
        GORSE_HIP_CHECK(hipMemcpyAsync(h->qid.p, qid_host + c0, (size_t)m * 8, hipMemcpyHostToDevice, h->stream));
        gather_queries_kernel<<<dim3((unsigned)m), dim3(64), 0, h->stream>>>(h->opB, h->norm2.p, h->qid.p, m, kpad,
                                                                            h->opQ.p, h->qn2.p);
        GORSE_HIP_CHECK(hipGetLastError());
        Bop = h->opQ.p;
        qn2 = h->qn2.p;
    } else {
        Qf = qv_dev + c0 * d;
        if (h->dtype == GORSE_DTYPE_BF16)
            pad_bf16_kernel<<<dim3(1024), dim3(256), 0, h->stream>>>(nullptr, Qf, m, d, kpad, h->opQ.p);
        else
            split_f32_kernel<<<dim3(1024), dim3(256), 0, h->stream>>>(Qf, m, d, kpad, 1, h->opQ.p);
        GORSE_HIP_CHECK(hipGetLastError());
        GORSE_TRY(topk_compute_norms(h, Qf, m, h->qn2.p));
        Bop = h->opQ.p;
        qn2 = h->qn2.p;
    }
    if (euclid)
        margin_euclid_kernel<<<dim3((unsigned)std::min<int64_t>(ceil_div(m, 256), 1024)), dim3(256), 0, h->stream>>>(
            qn2, m, h->err_coef, h->max_norm, (float)(d * 5.9604645e-8), h->qmargin.p);
    else
        margin_kernel<<<dim3((unsigned)std::min<int64_t>(ceil_div(m, 256), 1024)), dim3(256), 0, h->stream>>>(
            qn2, m, h->err_coef, other, h->qmargin.p);
    GORSE_HIP_CHECK(hipGetLastError());
    GORSE_HIP_CHECK(hipMemsetAsync(h->cflag.p, 0, (size_t)m, h->stream));
    SweepParams &sp = cs.sp;
    sp.A = h->opA;
    sp.B = Bop;
    sp.rscale = h->has_mask ? h->rscale_m.p : h->rscale.p;
    sp.qmargin = h->qmargin.p;
    sp.cbuf = h->cbuf.p;
    sp.ccnt = h->ccnt.p;
    sp.cflag = h->cflag.p;
    sp.hbuf = nullptr;
    sp.hcnt = nullptr;
    // epilogue: Euclidean adds its bias to every score; cosine multiplies every score by the row scale unless the scales
    // lie within 2 % of each other (then the block's largest raw score times the extreme scale bounds the block and
    // rows are scaled only behind that test; COARSE_OFF / COARSE_ON: off / on whatever the norms); -dot has the value 1
    // (NaN for a masked row), which the block test never needs
    const bool cos_coarse = (g_topk_variant & GORSE_TEST_TOPK_COARSE_OFF) ? false : ((g_topk_variant & GORSE_TEST_TOPK_COARSE_ON) ? true : h->coarse_ok);
    sp.ep = euclid ? EP_BIAS : (h->metric == GORSE_METRIC_COSINE ? (cos_coarse ? EP_COARSE : EP_SCALE) : EP_COARSE);
    sp.compact_at = kCompactSubAt;
    sp.prof = nullptr;
    if (g_topk_variant & GORSE_TEST_TOPK_REPLAY_COUNTERS) {
        GORSE_TRY(h->sweep_prof.ensure(16));
        GORSE_HIP_CHECK(hipMemsetAsync(h->sweep_prof.p, 0, 16 * sizeof(unsigned long long), h->stream));
        sp.prof = h->sweep_prof.p;
    }
    sp.N = h->N;
    sp.nq = m;
    sp.kth = kth;
    sp.f0 = nullptr, sp.f_out = nullptr, sp.tile_stride = 1;
    sp.nslices = 1;
    // bounds of the per-row value for the DMA sweeps' block test: the cosine scales; without them (a masked -dot index:
    // the value is 1 or NaN) the bound is the score itself
    sp.rs_min = h->metric == GORSE_METRIC_COSINE ? h->rs_min : 1.0f;
    sp.rs_max = h->metric == GORSE_METRIC_COSINE ? h->rs_max : 1.0f;
    sp.sym_q0 = 0;
    sp.frow = sp.frow_raw = nullptr;
    sp.fbuf = nullptr;
    sp.fcnt = nullptr;
    sp.sym_stats = nullptr;
    sp.sym_rank = 0, sp.sym_world = 1, sp.sym_slices = 1;
    sp.fwarm = nullptr;
    cs.warm = warm_start(g_topk_variant, kth, h->N);  // pilot sweeps propose the thresholds the main sweep starts from (topk_plan.hpp)
    cs.Bop = Bop, cs.qn2 = qn2, cs.Qf = Qf;
    return GORSE_OK;
}

// stage B: the pilot sweeps (see topk_plan.hpp's comment on the warm start) over the queries [lo, hi) of the chunk: their thresholds
// land in h->f0[lo .. hi)
int32_t chunk_pilots(gorse_topk *h, ChunkState &cs, int64_t lo, int64_t hi) {
    if (hi <= lo) return GORSE_OK;
    SweepParams p2 = slice_params(cs.sp, lo, hi - lo, h->kp * 16);
    p2.kth = (g_topk_variant & GORSE_TEST_TOPK_PILOT_KTH2) ? 2 : pilot_kth(cs.kth, kPilotStride);
    p2.tile_stride = kPilotStride;
    p2.f_out = h->f0.p + lo;
    if (two_pilots(g_topk_variant, h->N)) {  // a 1/256 sample proposes the 1/16 sample's thresholds first
        SweepParams p1 = p2;
        p1.kth = pilot_kth(p2.kth, 16);
        p1.tile_stride = kPilotStride * 16;
        p1.f_out = h->f1.p + lo;
        GORSE_TRY(dispatch_sweep(h, p1, false));
        GORSE_HIP_CHECK(hipMemsetAsync(h->cflag.p + lo, 0, (size_t)(hi - lo), h->stream));
        p2.f0 = h->f1.p + lo;
    }
    GORSE_TRY(dispatch_sweep(h, p2, false));
    GORSE_HIP_CHECK(hipMemsetAsync(h->cflag.p + lo, 0, (size_t)(hi - lo), h->stream));  // a pilot's flags say nothing about the query
    return GORSE_OK;
}

// stage C: the main sweep -- symmetric where the call allows it (cs.sym says which form ran)
int32_t chunk_main(gorse_topk *h, ChunkState &cs) {
    const int64_t m = cs.m;
    SweepParams &sp = cs.sp;
    if (cs.warm) sp.f0 = h->f0.p;
    // the symmetric form (topk_sweep_kernel, SYM) where the queries are a contiguous range of the stored rows that sym_eligible accepts
    const int64_t sym_q0 = cs.q_contig_begin + cs.c0;
    bool sym = cs.warm && cs.contiguous && sym_eligible(g_topk_variant, h->kp, cs.kth, h->N, sym_q0, m);
    if (cs.warm) {
        // sym_stats[0..3]: the counters of the whole search (every chunk adds to them); [4]: THIS chunk's queries without a pilot
        // threshold -- cleared per chunk, so that a chunk that was not eligible for the symmetric form leaves nothing behind for the
        // next one's decision (round 5 took a difference against a host copy that only symmetric chunks updated)
        GORSE_TRY(h->sym_stats.ensure(8));
        if (cs.c0 == 0) GORSE_HIP_CHECK(hipMemsetAsync(h->sym_stats.p, 0, 8 * sizeof(unsigned long long), h->stream));
        else GORSE_HIP_CHECK(hipMemsetAsync(h->sym_stats.p + 4, 0, sizeof(unsigned long long), h->stream));
        pilot_unset_count_kernel<<<dim3((unsigned)std::min<int64_t>(ceil_div(m, 256), 1024)), dim3(256), 0, h->stream>>>(h->f0.p, m, h->sym_stats.p);
        GORSE_HIP_CHECK(hipGetLastError());
    }
    if (sym && cs.tri_world == 1) {
        // A query the pilot left without a threshold costs the symmetric form a sweep of its own (the tie path's), the square form
        // only a cold start: where the pilot fails for many (rows sorted so that the systematic sample misleads it -- the
        // Euclidean case of test_warm_started_sweep_returns_the_same_rows), the square sweep is the better one.  One 8-byte read
        // behind the pilots.
        unsigned long long unset = 0;
        GORSE_HIP_CHECK(hipMemcpyAsync(&unset, h->sym_stats.p + 4, sizeof(unset), hipMemcpyDeviceToHost, h->stream));
        GORSE_HIP_CHECK(hipStreamSynchronize(h->stream));
        if ((int64_t)unset * 32 > m && cs.tri_world == 1) sym = false;
    }
    h->last_sym = sym;
    if (sym) {
        GORSE_TRY(h->fbuf.ensure((size_t)cs.mb * kCapF));
        GORSE_TRY(h->fcnt.ensure((size_t)cs.mb));
        const bool rawf = sp.ep == EP_COARSE;
        if (rawf) GORSE_TRY(h->f0raw.ensure((size_t)cs.mb));
        GORSE_HIP_CHECK(hipMemsetAsync(h->fcnt.p, 0, (size_t)m * 4, h->stream));
        sym_thresholds_kernel<<<dim3((unsigned)std::min<int64_t>(ceil_div(m, 256), 1024)), dim3(256), 0, h->stream>>>(
            h->f0.p, rawf ? h->f0raw.p : nullptr, h->cflag.p, m, sp.rs_min, sp.rs_max, h->sym_stats.p);
        GORSE_HIP_CHECK(hipGetLastError());
        sp.sym_q0 = sym_q0;
        sp.frow = h->f0.p;
        sp.frow_raw = rawf ? h->f0raw.p : nullptr;
        sp.fbuf = h->fbuf.p;
        sp.fcnt = h->fcnt.p;
        sp.sym_stats = h->sym_stats.p;
        sp.f_out = h->f1.p;  // the thresholds the workgroups end with: topk_rescore_kernel's verification reads them
        sp.sym_rank = cs.tri_rank, sp.sym_world = cs.tri_world;
        sp.sym_slices = cs.sym_slices;
        if (cs.sym_slices > 1)  // (slice 0's flags were cleared by chunk_prepare and may carry sym_thresholds_kernel's 2)
            GORSE_HIP_CHECK(hipMemsetAsync(h->cflag.p + cs.mb, 0, (size_t)(cs.sym_slices - 1) * cs.mb, h->stream));
    }
    GORSE_TRY(dispatch_sweep(h, sp, false, sym));
    cs.sym = sym;
    return GORSE_OK;
}

// flagged positions [at, at + n) of the chunk's list (h->fl_pos) to the host
static int32_t fetch_flagged(gorse_topk *h, int64_t at, int64_t n, std::vector<int64_t> &out) {
    std::vector<int32_t> tmp((size_t)n);
    GORSE_HIP_CHECK(hipMemcpyAsync(tmp.data(), h->fl_pos.p + at, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
    GORSE_HIP_CHECK(hipStreamSynchronize(h->stream));
    for (int32_t v : tmp) out.push_back(v);
    return GORSE_OK;
}

// stage D2: history sweep + literal heap replay (topk_tie.hip) for the n_flagged queries the rescoring listed, kReplayChunk at a
// time; rest = the positions of those it leaves undecided
static int32_t tie_path(gorse_topk *h, const ChunkState &cs, int64_t n_flagged, std::vector<int64_t> &rest) {
    if (n_flagged <= 0) return GORSE_OK;
    // (with a mask the replay's gap arithmetic -- which counts the rows between two recorded ones -- would count masked
    // rows too: those queries take the literal scan, which skips masked rows)
    if (g_topk_force_path == 3 || h->has_mask) return fetch_flagged(h, 0, n_flagged, rest);
    std::vector<uint8_t> f2;
    for (int64_t f0 = 0; f0 < n_flagged; f0 += kReplayChunk) {
        const int64_t m2 = std::min<int64_t>(kReplayChunk, n_flagged - f0);
        GORSE_TRY(tie_replay_chunk(h, cs, f0, m2, f2));
        int64_t undecided = 0;
        for (int64_t r = 0; r < m2; r++) undecided += f2[r] != 0;
        h->n_tie += m2 - undecided;
        if (undecided > 0) {  // rare: their positions come to the host now
            std::vector<int64_t> at;
            GORSE_TRY(fetch_flagged(h, f0, m2, at));
            for (int64_t r = 0; r < m2; r++)
                if (f2[r]) rest.push_back(at[(size_t)r]);
        }
    }
    return GORSE_OK;
}

// stage D3: whatever is left replays the reference literally over all N vectors (path A); its rows go into
// the chunk's device result arrays like everybody else's
static int32_t scan_rest(gorse_topk *h, const ChunkState &cs, const std::vector<int64_t> &rest) {
    if (rest.empty()) return GORSE_OK;
    const int d = h->d, k = cs.k, prune0 = cs.prune0;
    const bool by_vector = cs.by_vector;
    const float *qn2 = cs.qn2, *Qf = cs.Qf;
    auto stored_id = [&](int64_t t) -> int64_t {
        return by_vector ? -1 : (cs.qid_host ? cs.qid_host[cs.c0 + t] : cs.q_contig_begin + cs.c0 + t);
    };
    h->n_fallback += (int64_t)rest.size();
    const int64_t bq = topk_scan_block_queries(h);
    std::vector<int64_t> ids((size_t)std::min<int64_t>(bq, (int64_t)rest.size()));
    std::vector<int32_t> ti((size_t)ids.size() * k), tc(ids.size());
    std::vector<float> td((size_t)ids.size() * k);
    GORSE_TRY(h->qbuf.ensure(ids.size() * (size_t)d));
    GORSE_TRY(h->qnorm.ensure(ids.size()));
    GORSE_TRY(h->qidx.ensure(ids.size()));
    for (size_t f0 = 0; f0 < rest.size(); f0 += (size_t)bq) {
        const int64_t fm = std::min<int64_t>(bq, (int64_t)(rest.size() - f0));
        for (int64_t r = 0; r < fm; r++) {
            const int64_t t = rest[f0 + r];
            ids[r] = stored_id(t);
            const float *src = by_vector ? Qf + t * d : h->X.p + ids[r] * d;
            GORSE_HIP_CHECK(hipMemcpyAsync(h->qbuf.p + r * d, src, (size_t)d * 4, hipMemcpyDeviceToDevice, h->stream));
            GORSE_HIP_CHECK(hipMemcpyAsync(h->qnorm.p + r, qn2 + t, 4, hipMemcpyDeviceToDevice, h->stream));
        }
        const int64_t *excl = nullptr;
        if (!by_vector) {
            GORSE_HIP_CHECK(hipMemcpyAsync(h->qidx.p, ids.data(), (size_t)fm * 8, hipMemcpyHostToDevice, h->stream));
            excl = h->qidx.p;
        }
        GORSE_TRY(topk_scan_block(h, fm, excl, by_vector ? nullptr : ids.data(), k, prune0, ti.data(), td.data(), tc.data(),
                                  /*reroute=*/false));  // these queries come FROM the replay: the literal kernel ends it
        for (int64_t r = 0; r < fm; r++) {
            const int64_t t = rest[f0 + r];
            GORSE_HIP_CHECK(hipMemcpyAsync(h->res_idx.p + t * k, ti.data() + r * k, (size_t)k * 4, hipMemcpyHostToDevice, h->stream));
            GORSE_HIP_CHECK(hipMemcpyAsync(h->res_dist.p + t * k, td.data() + r * k, (size_t)k * 4, hipMemcpyHostToDevice, h->stream));
            GORSE_HIP_CHECK(hipMemcpyAsync(h->res_cnt.p + t, tc.data() + r, 4, hipMemcpyHostToDevice, h->stream));
        }
        GORSE_HIP_CHECK(hipStreamSynchronize(h->stream));
    }
    return GORSE_OK;
}

// stage D: exact rescoring of the lists, the tie path for what that leaves undecided, the literal scan for what THAT leaves; the
// chunk's rows end up in h->res_idx / res_dist / res_cnt (a triangle shard: the rows of the queries this rank owns)
int32_t chunk_finish(gorse_topk *h, ChunkState &cs) {
    int64_t n_flagged = 0;
    GORSE_TRY(rescore_chunk(h, cs, &n_flagged));
    std::vector<int64_t> rest;
    GORSE_TRY(tie_path(h, cs, n_flagged, rest));
    return scan_rest(h, cs, rest);
}

int32_t topk_mfma_search(gorse_topk *h, const int64_t *qid_host, int64_t q_contig_begin, const float *qv_dev,
                         int64_t nq, int k, int prune0, int32_t *idx_out, float *dist_out, int32_t *cnt_out,
                         TopkBlockConsumer *consumer) {
    ChunkState &cs = *h->chunk_state();
    GORSE_TRY(search_setup(h, cs, qid_host, q_contig_begin, qv_dev, nq, k, prune0));
    for (int64_t c0 = 0; c0 < nq; c0 += kChunkQ) {
        const int64_t m = std::min(kChunkQ, nq - c0);
        cs.c0 = c0, cs.m = m;
        GORSE_TRY(chunk_prepare(h, cs));
        int tok = h->prof.begin(GORSE_PROF_TOPK_SWEEP, h->stream);
        if (cs.warm) {
            GORSE_TRY(h->f0.ensure((size_t)cs.mb));
            GORSE_TRY(h->f1.ensure((size_t)cs.mb));
            GORSE_TRY(chunk_pilots(h, cs, 0, m));
        }
        GORSE_TRY(chunk_main(h, cs));
        h->last_sym = cs.sym;
        // The queries whose warm start failed its verification carry flag 2: topk_rescore_kernel leaves flagged queries alone
        // and stage 2 of chunk_finish (history sweep from -inf + literal replay) answers them together with the tie queries -- a sweep
        // of their own would cost one workgroup a full pass over the rows (48 ms for 86 queries, profiles/r02_h_*).
        h->prof.end(tok, h->stream);
        GORSE_TRY(chunk_finish(h, cs));
        if (consumer) GORSE_TRY(consumer->block(c0, m, h->res_idx.p, h->res_dist.p, h->res_cnt.p, h->stream));
        if (idx_out)
            GORSE_HIP_CHECK(hipMemcpyAsync(idx_out + c0 * k, h->res_idx.p, (size_t)m * k * 4, hipMemcpyDeviceToHost, h->stream));
        if (dist_out)
            GORSE_HIP_CHECK(hipMemcpyAsync(dist_out + c0 * k, h->res_dist.p, (size_t)m * k * 4, hipMemcpyDeviceToHost, h->stream));
        if (cnt_out)
            GORSE_HIP_CHECK(hipMemcpyAsync(cnt_out + c0, h->res_cnt.p, (size_t)m * 4, hipMemcpyDeviceToHost, h->stream));
        GORSE_HIP_CHECK(hipStreamSynchronize(h->stream));
    }
    return GORSE_OK;
}

void topk_mfma_release(gorse_topk *h) {
    delete h->cstate;
    h->cstate = nullptr;
}

}  // namespace gorse

gorse::TopkChunkState *gorse_topk::chunk_state() {
    if (!cstate) cstate = new gorse::TopkChunkState();
    return cstate;
}
