// sq.hip -- gorse_sq: the scalar-quantised (int8) exact top-k index (include/gorse_hip.h, "scalar-quantised index").
// A stored row is a row of int8 codes (padded with zero codes to whole K steps, sq_plan.hpp) and three fp32 constants: its scale, the
// squared norm and the norm of the dequantised row.  The inner product of two code rows is an exact int32; the reported score is a
// fixed chain of rounded fp32 operations on it, so every path below returns the same bits.
//
//   1. Encode (sq_encode_kernel): one wave per row.  max |x| by a shuffle reduction, the scale by one division, a code by one division
//      and rint, four codes packed per dword, the sum of squares by v_dot4_i32_i8.  Stored rows and search_vector's queries alike.
//   2. Pilot (sq_sweep_kernel<NS, true> + sq_pilot_select_kernel): every stride-th stored row is scored for every query on the int8
//      matrix cores; one workgroup per query then selects the kk-th best admissible sampled score by a four-pass radix select over
//      the keys in LDS: tau (kk = k, or k + 1 when the query's own row is left out).  The sample's kk rows at or above tau are rows
//      of the index, so the k best rows all score >= tau.  A query with fewer than kk admissible samples is handed to the scan.
//   3. Sweep (sq_sweep_kernel<NS, false>): a workgroup of four waves keeps 128 queries' code rows stationary in registers as B
//      fragments (4 VGPRs per K step) and streams its slice of the stored rows through LDS tiles, double-buffered, one barrier per
//      tile.  v_mfma_i32_32x32x32_i8 over the K steps; a lane then holds 16 dot products of ONE query (column lane & 31, rows
//      4 (lane >> 5) + (r & 3) + 8 (r >> 2)), forms the 16 reported scores and appends the keys of those >= tau to the query's list
//      in global memory.  A masked row and a row past N carry a NaN scale in the tile's constants and never pass.  A list that
//      overflows hands its query back.
//   4. Select (sq_select_kernel): one workgroup per query sorts the survivors' 64-bit keys in LDS (descending score, ascending row)
//      and writes the first k.
//   5. Scan (sq_scan_kernel): one workgroup per query, the query's codes in LDS, a thread per stored row with v_dot4_i32_i8, and a
//      running selection: keys above the k-th best so far go to an LDS buffer that is sorted and cut to k whenever it fills.
//      Right alone for every legal input; it answers what the plan does not give to the sweep, and every handed-back query.
// Key of a pair: rank_keys.hpp's score_ord in the upper word (-0 counts as +0), (2^31 - 1 - row) << 1 below it and the sign of a
// zero score in bit 0, so that the score's own bits come back.  No real key is 0: that is padding.
#include "common.hpp"
#include "rank_keys.hpp"
#include "sq_plan.hpp"

using namespace gorse;

namespace {

constexpr int kBlock = sq::kBlockThreads;
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));
typedef unsigned long long u64;

enum { kProfEncode = GORSE_PROF_SQ_ENCODE, kProfPilot = GORSE_PROF_SQ_PILOT, kProfSweep = GORSE_PROF_SQ_SWEEP,
       kProfSelect = GORSE_PROF_SQ_SELECT, kProfScan = GORSE_PROF_SQ_SCAN, kProfClasses = GORSE_PROF_SQ_NCLASSES };

int g_force_path = 0, g_cap_hint = 0;  // gorse_hip_test_set_sq

// one side of a search: code rows and their constants
struct SqRows {
    const int8_t *codes;
    const float *scale, *sn, *rn;
};

struct SqArgs {
    SqRows X, Q;
    const uint8_t *mask;  // or NULL
    int64_t N, nq;        // stored rows; queries of this launch
    int64_t self0;        // stored row of query 0 when own rows are left out, else -1
    int32_t dp, metric, k, kk;
    // sweep
    int32_t stride, n_sample, samp_ld, cap, pilot_slice_len, sweep_slice_len;
    float *samp, *tau;
    int32_t *cnt;
    uint8_t *hb;
    u64 *surv;
    // results (device), rows of this launch's queries
    int32_t *idx_out, *cnt_out;
    float *score_out;
    const int32_t *list;  // scan: the queries to answer, or NULL = all
};

__device__ __forceinline__ float sq_score(int metric, int t, float sx, float snx, float rnx, float sq_, float snq, float rnq) {
    const float p = ((float)t * sx) * sq_;
    if (metric == GORSE_METRIC_NEG_DOT) return p;
    if (metric == GORSE_METRIC_COSINE) {
        const float den = rnq * rnx;
        return den == 0.0f ? -1.0f : p / den - 1.0f;
    }
    return -sqrtf(fmaxf((snq + snx) - (p + p), 0.0f));
}

__device__ __forceinline__ u64 sq_key(float score, int row) {
    return ((u64)rank::score_ord(score) << 32) | (u64)(((0x7fffffffu - (uint32_t)row) << 1) | (rank::f2u(score) == 0x80000000u ? 1u : 0u));
}
__device__ __forceinline__ int sq_key_row(u64 key) { return (int)(0x7fffffffu - ((uint32_t)key >> 1)); }
__device__ __forceinline__ float sq_key_score(u64 key) { return (key & 1) ? -0.0f : rank::key_score(key); }

// descending bitonic sort of n keys in LDS, n a power of two; every thread of the workgroup calls it
__device__ void sort_desc(u64 *a, int n, int tid) {
    for (int size = 2; size <= n; size <<= 1)
        for (int j = size >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int t = tid; t < (n >> 1); t += kBlock) {
                const int lo = ((t / j) * 2 * j) + (t % j), hi = lo + j;
                const bool desc = (lo & size) == 0;
                const u64 x = a[lo], y = a[hi];
                if ((x < y) == desc) a[lo] = y, a[hi] = x;
            }
        }
    __syncthreads();
}

// the first m keys of a sorted list as a result row, padded to k
__device__ void write_row(const SqArgs &A, int64_t q, const u64 *keys, int m, int tid) {
    for (int r = tid; r < A.k; r += kBlock) {
        A.idx_out[q * A.k + r] = r < m ? sq_key_row(keys[r]) : -1;
        A.score_out[q * A.k + r] = r < m ? sq_key_score(keys[r]) : -INFINITY;
    }
    if (tid == 0) A.cnt_out[q] = m;
}

// ---- 1. encode ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void sq_encode_kernel(const float *__restrict__ X, int64_t rows, int d, int dp, int8_t *codes,
                                                           float *scale, float *sn, float *rn, int32_t *err) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float *x = X + row * d;
    float a = 0.0f;
    bool bad = false;
    for (int j = lane; j < d; j += 64) {
        const float v = x[j];
        bad = bad || !(fabsf(v) <= 3.402823466e38f);
        a = fmaxf(a, fabsf(v));
    }
    for (int o = 32; o > 0; o >>= 1) a = fmaxf(a, __shfl_xor(a, o));
    const float s = a / 127.0f;
    int n = 0;
    uint32_t *dst = (uint32_t *)(codes + row * dp);
    for (int w = lane; w < dp / 4; w += 64) {
        uint32_t pk = 0;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const int j = 4 * w + e;
            int c = 0;
            if (j < d && s > 0.0f && !bad) c = (int)rintf(x[j] / s);
            pk |= (uint32_t)(c & 255) << (8 * e);
        }
        n = __builtin_amdgcn_sdot4((int)pk, (int)pk, n, false);
        dst[w] = pk;
    }
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
    const float snr = (s * s) * (float)n;
    bad = bad || !(fabsf(snr) <= 3.402823466e38f);
    if (__any(bad) && lane == 0) atomicOr(err, 1);
    if (lane == 0) scale[row] = s, sn[row] = snr, rn[row] = sqrtf(snr);
}

// ---- 2./3. pilot and sweep -------------------------------------------------------------------------------------------------
// PILOT: virtual row j is stored row j * stride and its score goes to samp[query][j].  Otherwise: row j, compared with tau, appended.
template <int NS, bool PILOT>
__global__ __launch_bounds__(kBlock) void sq_sweep_kernel(const SqArgs A) {
    constexpr int dp = NS * sq::kKStep, LS = dp + sq::kPadRow, R = sq::tile_rows(NS);
    constexpr int NV = R * dp / 16;                 // 16-byte pieces of a tile
    constexpr int PT = (NV + kBlock - 1) / kBlock;  // of them per thread
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char *tiles = smem;                                 // [2][R * LS]
    float *consts = (float *)(smem + (size_t)2 * R * LS);        // [2][3][R]: scale (NaN = no such row) | sn | rn
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, col = lane & 31, hb = lane >> 5;
    const int64_t n = PILOT ? A.n_sample : A.N;
    const int64_t stride = PILOT ? A.stride : 1;
    const int64_t slice_len = PILOT ? A.pilot_slice_len : A.sweep_slice_len;
    const int64_t i0 = blockIdx.y * slice_len, i1 = min(n, i0 + slice_len);
    if (i0 >= i1) return;
    const int64_t tq = (int64_t)blockIdx.x * sq::kQueries + wv * 32 + col;
    const bool active = tq < A.nq && (PILOT || A.hb[tq] == 0);
    const float tau = (!PILOT && active) ? A.tau[tq] : 0.0f;
    float sq_ = 0.0f, snq = 0.0f, rnq = 0.0f;
    i32x4 bq[NS];
#pragma unroll
    for (int s = 0; s < NS; s++) bq[s] = i32x4{0, 0, 0, 0};
    if (active) {
        sq_ = A.Q.scale[tq], snq = A.Q.sn[tq], rnq = A.Q.rn[tq];
#pragma unroll
        for (int s = 0; s < NS; s++) bq[s] = *(const i32x4 *)(A.Q.codes + tq * dp + 32 * s + 16 * hb);
    }

    i32x4 rq[PT];
    float rc0 = 0.f, rc1 = 0.f, rc2 = 0.f;
    auto gload = [&](int64_t t0) {  // rows past the slice's end are zero codes under a NaN scale
#pragma unroll
        for (int e = 0; e < PT; e++) {
            const int x = tid + kBlock * e, row = x / (2 * NS), c = x % (2 * NS);
            rq[e] = i32x4{0, 0, 0, 0};
            if (x < NV && t0 + row < i1) rq[e] = *(const i32x4 *)(A.X.codes + (t0 + row) * stride * dp + 16 * c);
        }
        if (tid < R) {
            const int64_t r = (t0 + tid) * stride;
            const bool ok = t0 + tid < i1 && (PILOT || !A.mask || A.mask[r] != 0);
            rc0 = ok ? A.X.scale[r] : __builtin_nanf("");
            rc1 = ok ? A.X.sn[r] : 0.0f;
            rc2 = ok ? A.X.rn[r] : 0.0f;
        }
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int e = 0; e < PT; e++) {
            const int x = tid + kBlock * e, row = x / (2 * NS), c = x % (2 * NS);
            if (x < NV) *(i32x4 *)(tiles + (size_t)buf * R * LS + row * LS + 16 * c) = rq[e];
        }
        if (tid < R) {
            float *cb = consts + buf * 3 * R;
            cb[tid] = rc0, cb[R + tid] = rc1, cb[2 * R + tid] = rc2;
        }
    };

    gload(i0);
    lstore(0);
    __syncthreads();
    int p = 0;
    for (int64_t t0 = i0; t0 < i1; t0 += R, p ^= 1) {
        const bool more = t0 + R < i1;
        if (more) gload(t0 + R);
        const unsigned char *tile = tiles + (size_t)p * R * LS;
        const float *cb = consts + p * 3 * R;
        for (int sub = 0; sub < R / 32 && t0 + 32 * sub < i1; sub++) {
            // the A fragment's row is the lane's STORED row lane & 31 of the sub-tile, the B fragment's column its query
            const unsigned char *arow = tile + (32 * sub + col) * LS + 16 * hb;
            i32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; r++) acc[r] = 0;
#pragma unroll
            for (int s = 0; s < NS; s++) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(*(const i32x4 *)(arow + 32 * s), bq[s], acc, 0, 0, 0);
            float sc[16];
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int lr = 32 * sub + (r & 3) + 8 * (r >> 2) + 4 * hb;
                sc[r] = sq_score(A.metric, acc[r], cb[lr], cb[R + lr], cb[2 * R + lr], sq_, snq, rnq);
            }
            if constexpr (PILOT) {
                // every lane stores, a query past the launch's end too: samp has whole workgroups of rows, each padded to whole tiles
                float *dst = A.samp + tq * A.samp_ld + t0 + 32 * sub + 4 * hb;
#pragma unroll
                for (int g = 0; g < 4; g++) *(float4 *)(dst + 8 * g) = make_float4(sc[4 * g], sc[4 * g + 1], sc[4 * g + 2], sc[4 * g + 3]);
            } else {
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int lr = 32 * sub + (r & 3) + 8 * (r >> 2) + 4 * hb;
                    const float sx = cb[lr];
                    if (active && sx == sx && sc[r] >= tau) {
                        const int pos = atomicAdd(&A.cnt[tq], 1);
                        if (pos < A.cap) A.surv[tq * A.cap + pos] = sq_key(sc[r], (int)(t0 + lr));
                    }
                }
            }
        }
        if (more) lstore(p ^ 1);
        __syncthreads();
    }
}

// One workgroup per query: tau = the kk-th best admissible sampled score, or the query handed back.
__global__ __launch_bounds__(kBlock) void sq_pilot_select_kernel(const SqArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t *keys = (uint32_t *)smem;      // [n_sample]
    int *hist = (int *)(keys + A.n_sample);  // [256]
    __shared__ int s_valid, s_bin, s_rem;
    const int64_t tq = blockIdx.x;
    const int tid = threadIdx.x, n = A.n_sample;
    const int64_t self = A.self0 >= 0 ? A.self0 + tq : -1;
    if (tid == 0) s_valid = 0;
    __syncthreads();
    const float *row = A.samp + tq * A.samp_ld;
    int valid = 0;
    for (int j = tid; j < n; j += kBlock) {
        const int64_t r = (int64_t)j * A.stride;
        const bool ok = r != self && (!A.mask || A.mask[r] != 0);
        keys[j] = ok ? rank::score_ord(row[j]) : 0u;
        valid += ok;
    }
    if (valid) atomicAdd(&s_valid, valid);
    __syncthreads();
    if (s_valid < A.kk) {
        if (tid == 0) A.tau[tq] = INFINITY, A.hb[tq] = 1;
        return;
    }
    // the kk-th largest key, a byte per pass from the top: the histogram of the keys that share the bytes found so far
    uint32_t prefix = 0, mask = 0;
    int rem = A.kk;
    for (int shift = 24; shift >= 0; shift -= 8) {
        hist[tid] = 0;
        __syncthreads();
        for (int j = tid; j < n; j += kBlock)
            if (keys[j] != 0u && (keys[j] & mask) == prefix) atomicAdd(&hist[(keys[j] >> shift) & 255u], 1);
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
    if (tid == 0) A.tau[tq] = rank::key_score((u64)prefix << 32), A.hb[tq] = 0;
}

// ---- 4. select -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void sq_select_kernel(const SqArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u64 *keys = (u64 *)smem;
    __shared__ int s_n;
    const int64_t tq = blockIdx.x;
    const int tid = threadIdx.x;
    const int c = A.cnt[tq];
    if (A.hb[tq] != 0 || c > A.cap) {  // the scan answers it and writes its row
        if (tid == 0) A.hb[tq] = 1;
        return;
    }
    if (tid == 0) s_n = 0;
    __syncthreads();
    const int64_t self = A.self0 >= 0 ? A.self0 + tq : -1;
    int P = 1;
    while (P < c) P <<= 1;
    int kept = 0;
    for (int e = tid; e < P; e += kBlock) {
        u64 key = e < c ? A.surv[tq * A.cap + e] : 0;
        if (key != 0 && sq_key_row(key) == self) key = 0;
        keys[e] = key;
        kept += key != 0;
    }
    if (kept) atomicAdd(&s_n, kept);
    sort_desc(keys, P, tid);
    write_row(A, tq, keys, min(s_n, A.k), tid);
}

// ---- 5. scan ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void sq_scan_kernel(const SqArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u64 *buf = (u64 *)smem;                                     // [kScanBuf]
    const i32x4 *qc = (const i32x4 *)(smem + sq::kScanBuf * 8);  // [dp / 16]
    __shared__ int s_cnt;
    __shared__ u64 s_thr;
    const int tid = threadIdx.x;
    const int64_t q = A.list ? A.list[blockIdx.x] : blockIdx.x;
    const int64_t self = A.self0 >= 0 ? A.self0 + q : -1;
    const int nv = A.dp / 16;
    for (int w = tid; w < nv; w += kBlock) ((i32x4 *)qc)[w] = *(const i32x4 *)(A.Q.codes + q * A.dp + 16 * w);
    if (tid == 0) s_cnt = 0, s_thr = 0;
    const float sq_ = A.Q.scale[q], snq = A.Q.sn[q], rnq = A.Q.rn[q];
    __syncthreads();
    auto cut = [&]() {  // the buffer sorted and cut to its k best; every thread calls it
        const int c = s_cnt;
        for (int e = c + tid; e < sq::kScanBuf; e += kBlock) buf[e] = 0;
        sort_desc(buf, sq::kScanBuf, tid);
        if (tid == 0) {
            s_cnt = min(c, A.k);
            if (c >= A.k) s_thr = buf[A.k - 1];
        }
        __syncthreads();
    };
    for (int64_t base = 0; base < A.N; base += kBlock) {
        const int64_t r = base + tid;
        if (r < A.N && r != self && (!A.mask || A.mask[r] != 0)) {
            const i32x4 *xc = (const i32x4 *)(A.X.codes + r * A.dp);
            int t = 0;
            for (int w = 0; w < nv; w++) {
                const i32x4 x = xc[w], y = qc[w];
                t = __builtin_amdgcn_sdot4(x[0], y[0], t, false);
                t = __builtin_amdgcn_sdot4(x[1], y[1], t, false);
                t = __builtin_amdgcn_sdot4(x[2], y[2], t, false);
                t = __builtin_amdgcn_sdot4(x[3], y[3], t, false);
            }
            const u64 key = sq_key(sq_score(A.metric, t, A.X.scale[r], A.X.sn[r], A.X.rn[r], sq_, snq, rnq), (int)r);
            if (key > s_thr) buf[atomicAdd(&s_cnt, 1)] = key;  // at most kBlock more than the bound below
        }
        __syncthreads();
        const bool full = s_cnt > sq::kScanBuf - kBlock;
        __syncthreads();  // every thread has read the count before the next step adds to it
        if (full) cut();
    }
    cut();
    write_row(A, q, buf, s_cnt, tid);
}

__global__ __launch_bounds__(kBlock) void sq_clear_kernel(int32_t *cnt, uint8_t *hb, int64_t n) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t < n) cnt[t] = 0, hb[t] = 0;
}

}  // namespace

struct gorse_sq {
    int device = 0;
    hipStream_t stream = nullptr;
    int64_t N = 0;
    int32_t d = 0, dp = 0, metric = 0;
    DevBuf<int8_t> codes, qcodes;
    DevBuf<float> scale, sn, rn, qconst, stage, samp, tau, score_out;
    DevBuf<uint8_t> mask, hb;
    DevBuf<int32_t> err, cnt, idx_out, cnt_out, list;
    DevBuf<u64> surv;
    bool has_mask = false;
    KernelProfile prof{kProfClasses};
    int64_t n_sweep = 0, n_scan = 0, n_handed_back = 0;
    int32_t use() {
        GORSE_HIP_CHECK(hipSetDevice(device));
        return GORSE_OK;
    }
};

namespace {

// rows x d floats on the host -> code rows and constants on the device; GORSE_ERR_INVALID for a row that cannot be encoded
int32_t encode(gorse_sq *h, const float *X, int64_t rows, int8_t *codes, float *scale, float *sn, float *rn) {
    const int64_t per = std::max<int64_t>(1, ((int64_t)1 << 26) / h->d);
    GORSE_TRY(h->stage.ensure((size_t)(std::min(per, rows) * h->d)));
    GORSE_TRY(h->err.ensure(1));
    GORSE_HIP_CHECK(hipMemsetAsync(h->err.p, 0, 4, h->stream));
    for (int64_t r0 = 0; r0 < rows; r0 += per) {
        const int64_t m = std::min(per, rows - r0);
        GORSE_HIP_CHECK(hipMemcpyAsync(h->stage.p, X + r0 * h->d, (size_t)(m * h->d) * 4, hipMemcpyHostToDevice, h->stream));
        const int tok = h->prof.begin(kProfEncode, h->stream);
        sq_encode_kernel<<<dim3((unsigned)ceil_div(m, kBlock / 64)), dim3(kBlock), 0, h->stream>>>(
            h->stage.p, m, h->d, h->dp, codes + r0 * h->dp, scale + r0, sn + r0, rn + r0, h->err.p);
        h->prof.end(tok, h->stream);
        GORSE_HIP_CHECK(hipGetLastError());
        GORSE_HIP_CHECK(hipStreamSynchronize(h->stream));  // the staging buffer is filled again
    }
    int32_t err = 0;
    GORSE_HIP_CHECK(hipMemcpy(&err, h->err.p, 4, hipMemcpyDeviceToHost));
    if (err) return fail(GORSE_ERR_INVALID, "a row holds a non-finite value, or its squared norm is not finite");
    return GORSE_OK;
}

template <int NS>
int32_t launch_sweep(gorse_sq *h, const SqArgs &A, const sq::Plan &P) {
    const size_t lds = sq::sweep_lds(NS);
    GORSE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&sq_sweep_kernel<NS, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    GORSE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&sq_sweep_kernel<NS, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const unsigned blocks = (unsigned)ceil_div(A.nq, (int64_t)sq::kQueries);
    sq_clear_kernel<<<dim3((unsigned)ceil_div(A.nq, (int64_t)kBlock)), dim3(kBlock), 0, h->stream>>>(A.cnt, A.hb, A.nq);
    int tok = h->prof.begin(kProfPilot, h->stream);
    sq_sweep_kernel<NS, true><<<dim3(blocks, (unsigned)P.pilot_slices), dim3(kBlock), lds, h->stream>>>(A);
    sq_pilot_select_kernel<<<dim3((unsigned)A.nq), dim3(kBlock), P.pilot_lds, h->stream>>>(A);
    h->prof.end(tok, h->stream);
    tok = h->prof.begin(kProfSweep, h->stream);
    sq_sweep_kernel<NS, false><<<dim3(blocks, (unsigned)P.sweep_slices), dim3(kBlock), lds, h->stream>>>(A);
    h->prof.end(tok, h->stream);
    tok = h->prof.begin(kProfSelect, h->stream);
    sq_select_kernel<<<dim3((unsigned)A.nq), dim3(kBlock), P.select_lds, h->stream>>>(A);
    h->prof.end(tok, h->stream);
    GORSE_HIP_CHECK(hipGetLastError());
    return GORSE_OK;
}

int32_t launch_scan(gorse_sq *h, const SqArgs &A, int64_t n) {
    if (n == 0) return GORSE_OK;
    const int tok = h->prof.begin(kProfScan, h->stream);
    sq_scan_kernel<<<dim3((unsigned)n), dim3(kBlock), (size_t)sq::kScanBuf * 8 + (size_t)A.dp, h->stream>>>(A);
    h->prof.end(tok, h->stream);
    GORSE_HIP_CHECK(hipGetLastError());
    return GORSE_OK;
}

// nq queries (code rows and constants on the device) against the index; results to the host
int32_t search(gorse_sq *h, const SqRows &Q, int64_t nq, int64_t self0, int32_t k, int32_t *idx_out, float *score_out, int32_t *count_out) {
    const int32_t kk = k + (self0 >= 0 ? 1 : 0);
    GORSE_TRY(h->idx_out.ensure((size_t)(nq * k)));
    GORSE_TRY(h->score_out.ensure((size_t)(nq * k)));
    GORSE_TRY(h->cnt_out.ensure((size_t)nq));
    SqArgs A{};
    A.X = SqRows{h->codes.p, h->scale.p, h->sn.p, h->rn.p};
    A.mask = h->has_mask ? h->mask.p : nullptr;
    A.N = h->N, A.dp = h->dp, A.metric = h->metric, A.k = k, A.kk = kk;
    h->n_sweep = h->n_scan = h->n_handed_back = 0;
    std::vector<int32_t> back;
    if (sq::choose(g_force_path, nq, h->N, h->d, k, kk) == sq::kSweep) {
        const sq::Plan P = sq::make_plan(h->N, h->d, kk, nq, g_cap_hint);
        if (P.pilot_lds > (size_t)160 * 1024 || P.select_lds > (size_t)160 * 1024) return fail(GORSE_ERR_INVALID, "sweep plan beyond LDS");
        GORSE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&sq_pilot_select_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)P.pilot_lds));
        GORSE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&sq_select_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)P.select_lds));
        GORSE_TRY(h->samp.ensure((size_t)P.chunk * (size_t)P.samp_ld));
        GORSE_TRY(h->surv.ensure((size_t)P.chunk * (size_t)P.cap));
        GORSE_TRY(h->tau.ensure((size_t)P.chunk));
        GORSE_TRY(h->cnt.ensure((size_t)P.chunk));
        GORSE_TRY(h->hb.ensure((size_t)nq));
        A.stride = P.stride, A.n_sample = P.n_sample, A.samp_ld = P.samp_ld, A.cap = P.cap;
        A.pilot_slice_len = P.pilot_slice_len, A.sweep_slice_len = P.sweep_slice_len;
        A.samp = h->samp.p, A.tau = h->tau.p, A.cnt = h->cnt.p, A.surv = h->surv.p;
        for (int64_t q0 = 0; q0 < nq; q0 += P.chunk) {
            A.nq = std::min(P.chunk, nq - q0);
            A.Q = SqRows{Q.codes + q0 * h->dp, Q.scale + q0, Q.sn + q0, Q.rn + q0};
            A.self0 = self0 >= 0 ? self0 + q0 : -1;
            A.hb = h->hb.p + q0;
            A.idx_out = h->idx_out.p + q0 * k, A.score_out = h->score_out.p + q0 * k, A.cnt_out = h->cnt_out.p + q0;
            switch (P.steps) {
#define GORSE_SQ_NS(n) \
    case n: GORSE_TRY(launch_sweep<n>(h, A, P)); break;
                GORSE_SQ_NS(1) GORSE_SQ_NS(2) GORSE_SQ_NS(3) GORSE_SQ_NS(4) GORSE_SQ_NS(6) GORSE_SQ_NS(8) GORSE_SQ_NS(12) GORSE_SQ_NS(16)
                GORSE_SQ_NS(24) GORSE_SQ_NS(32)
#undef GORSE_SQ_NS
                default: return fail(GORSE_ERR_INVALID, "no sweep for %d K steps", P.steps);
            }
        }
        std::vector<uint8_t> hb((size_t)nq);
        GORSE_HIP_CHECK(hipMemcpyAsync(hb.data(), h->hb.p, (size_t)nq, hipMemcpyDeviceToHost, h->stream));
        GORSE_HIP_CHECK(hipStreamSynchronize(h->stream));
        for (int64_t t = 0; t < nq; t++)
            if (hb[(size_t)t]) back.push_back((int32_t)t);
        h->n_handed_back = (int64_t)back.size();
        h->n_sweep = nq - h->n_handed_back;
    }
    A.nq = nq, A.Q = Q, A.self0 = self0;
    A.idx_out = h->idx_out.p, A.score_out = h->score_out.p, A.cnt_out = h->cnt_out.p;
    if (h->n_sweep + h->n_handed_back == 0) {  // the scan answers the whole call
        h->n_scan = nq;
        GORSE_TRY(launch_scan(h, A, nq));
    } else if (!back.empty()) {
        h->n_scan = (int64_t)back.size();
        GORSE_TRY(h->list.ensure(back.size()));
        GORSE_HIP_CHECK(hipMemcpyAsync(h->list.p, back.data(), back.size() * 4, hipMemcpyHostToDevice, h->stream));
        A.list = h->list.p;
        GORSE_TRY(launch_scan(h, A, (int64_t)back.size()));
        GORSE_HIP_CHECK(hipStreamSynchronize(h->stream));  // `back` is pageable host memory
    }
    GORSE_HIP_CHECK(hipMemcpyAsync(idx_out, h->idx_out.p, (size_t)(nq * k) * 4, hipMemcpyDeviceToHost, h->stream));
    GORSE_HIP_CHECK(hipMemcpyAsync(score_out, h->score_out.p, (size_t)(nq * k) * 4, hipMemcpyDeviceToHost, h->stream));
    GORSE_HIP_CHECK(hipMemcpyAsync(count_out, h->cnt_out.p, (size_t)nq * 4, hipMemcpyDeviceToHost, h->stream));
    GORSE_HIP_CHECK(hipStreamSynchronize(h->stream));
    return GORSE_OK;
}

int32_t check_search(gorse_sq *h, int32_t k, const void *a, const void *b, const void *c) {
    if (!h) return fail(GORSE_ERR_INVALID, "handle is NULL");
    if (k < 1 || k > sq::kMaxK) return fail(GORSE_ERR_INVALID, "k = %d outside 1 .. %d", k, sq::kMaxK);
    if (!a || !b || !c) return fail(GORSE_ERR_INVALID, "idx_out, score_out and count_out are required");
    return h->use();
}

}  // namespace

extern "C" void gorse_hip_test_set_sq(int32_t path, int32_t list_capacity) {
    g_force_path = path >= 0 && path <= 2 ? path : 0;
    g_cap_hint = list_capacity > 0 ? list_capacity : 0;
}

extern "C" int32_t gorse_sq_create(gorse_sq **out, int32_t device, int64_t N, int32_t d, int32_t metric, int32_t bits, const float *X) {
    if (!out || !X) return fail(GORSE_ERR_INVALID, "NULL argument");
    if (N < 1 || N >= ((int64_t)1 << 31)) return fail(GORSE_ERR_INVALID, "N = %lld outside 1 .. 2^31 - 1", (long long)N);
    if (d < 1 || d > sq::kMaxD) return fail(GORSE_ERR_INVALID, "d = %d outside 1 .. %d", d, sq::kMaxD);
    if (bits != 0 && bits != 8) return fail(GORSE_ERR_INVALID, "bits = %d: a scalar-quantised index holds 8-bit codes", bits);
    if (metric != GORSE_METRIC_NEG_DOT && metric != GORSE_METRIC_EUCLIDEAN && metric != GORSE_METRIC_COSINE)
        return fail(GORSE_ERR_INVALID, "metric %d not offered by the scalar-quantised index", metric);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return fail(GORSE_ERR_NO_DEVICE, "no device %d", device);
    gorse_sq *h = new (std::nothrow) gorse_sq;
    if (!h) return fail(GORSE_ERR_NOMEM, "host allocation failed");
    h->device = device, h->N = N, h->d = d, h->dp = sq::padded_d(d), h->metric = metric;
    auto build = [&]() -> int32_t {
        GORSE_TRY(h->use());
        GORSE_HIP_CHECK(hipStreamCreate(&h->stream));
        GORSE_TRY(h->codes.alloc((size_t)N * (size_t)h->dp));
        GORSE_TRY(h->scale.alloc((size_t)N));
        GORSE_TRY(h->sn.alloc((size_t)N));
        GORSE_TRY(h->rn.alloc((size_t)N));
        return encode(h, X, N, h->codes.p, h->scale.p, h->sn.p, h->rn.p);
    };
    const int32_t rc = build();
    if (rc != GORSE_OK) {
        const std::string keep = last_error();
        gorse_sq_destroy(h);
        last_error() = keep;
        return rc;
    }
    *out = h;
    return GORSE_OK;
}

extern "C" int32_t gorse_sq_destroy(gorse_sq *h) {
    if (!h) return GORSE_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) {
        (void)hipStreamSynchronize(h->stream);
        (void)hipStreamDestroy(h->stream);
    }
    delete h;
    return GORSE_OK;
}

extern "C" int32_t gorse_sq_set_mask(gorse_sq *h, const uint8_t *admissible) {
    if (!h) return fail(GORSE_ERR_INVALID, "handle is NULL");
    GORSE_TRY(h->use());
    h->has_mask = false;
    if (!admissible) return GORSE_OK;
    GORSE_TRY(h->mask.ensure((size_t)h->N));
    GORSE_HIP_CHECK(hipMemcpyAsync(h->mask.p, admissible, (size_t)h->N, hipMemcpyHostToDevice, h->stream));
    GORSE_HIP_CHECK(hipStreamSynchronize(h->stream));
    h->has_mask = true;
    return GORSE_OK;
}

extern "C" int32_t gorse_sq_search_vector(gorse_sq *h, const float *Q, int64_t nq, int32_t k, int32_t *idx_out, float *score_out,
                                          int32_t *count_out) {
    GORSE_TRY(check_search(h, k, idx_out, score_out, count_out));
    if (!Q || nq < 0 || nq >= ((int64_t)1 << 31)) return fail(GORSE_ERR_INVALID, "bad queries");
    if (nq == 0) return GORSE_OK;
    // the queries' codes and constants live in scratch of their own: a refused query leaves the index as it was
    GORSE_TRY(h->qcodes.ensure((size_t)nq * (size_t)h->dp));
    GORSE_TRY(h->qconst.ensure((size_t)nq * 3));
    const SqRows R{h->qcodes.p, h->qconst.p, h->qconst.p + nq, h->qconst.p + 2 * nq};
    GORSE_TRY(encode(h, Q, nq, h->qcodes.p, h->qconst.p, h->qconst.p + nq, h->qconst.p + 2 * nq));
    return search(h, R, nq, -1, k, idx_out, score_out, count_out);
}

extern "C" int32_t gorse_sq_search_rows(gorse_sq *h, int64_t q_begin, int64_t q_end, int32_t k, int32_t exclude_self, int32_t *idx_out,
                                        float *score_out, int32_t *count_out) {
    GORSE_TRY(check_search(h, k, idx_out, score_out, count_out));
    if (q_begin < 0 || q_end < q_begin || q_end > h->N) return fail(GORSE_ERR_RANGE, "rows [%lld, %lld) outside the index", (long long)q_begin, (long long)q_end);
    if (q_end == q_begin) return GORSE_OK;
    const SqRows R{h->codes.p + q_begin * h->dp, h->scale.p + q_begin, h->sn.p + q_begin, h->rn.p + q_begin};
    return search(h, R, q_end - q_begin, exclude_self ? q_begin : -1, k, idx_out, score_out, count_out);
}

extern "C" int32_t gorse_sq_get_codes(gorse_sq *h, int64_t r_begin, int64_t r_end, int8_t *codes, float *scale) {
    if (!h) return fail(GORSE_ERR_INVALID, "handle is NULL");
    if (r_begin < 0 || r_end < r_begin || r_end > h->N) return fail(GORSE_ERR_RANGE, "rows [%lld, %lld) outside the index", (long long)r_begin, (long long)r_end);
    GORSE_TRY(h->use());
    const int64_t m = r_end - r_begin;
    if (m == 0) return GORSE_OK;
    GORSE_HIP_CHECK(hipStreamSynchronize(h->stream));
    if (codes) GORSE_HIP_CHECK(hipMemcpy2D(codes, (size_t)h->d, h->codes.p + r_begin * h->dp, (size_t)h->dp, (size_t)h->d, (size_t)m, hipMemcpyDeviceToHost));
    if (scale) GORSE_HIP_CHECK(hipMemcpy(scale, h->scale.p + r_begin, (size_t)m * 4, hipMemcpyDeviceToHost));
    return GORSE_OK;
}

extern "C" int32_t gorse_sq_last_stats(gorse_sq *h, int64_t *n_sweep, int64_t *n_scan, int64_t *n_handed_back) {
    if (!h) return fail(GORSE_ERR_INVALID, "handle is NULL");
    if (n_sweep) *n_sweep = h->n_sweep;
    if (n_scan) *n_scan = h->n_scan;
    if (n_handed_back) *n_handed_back = h->n_handed_back;
    return GORSE_OK;
}

extern "C" int32_t gorse_sq_set_profiling(gorse_sq *h, int32_t on) {
    if (!h) return fail(GORSE_ERR_INVALID, "handle is NULL");
    GORSE_TRY(h->use());
    GORSE_HIP_CHECK(hipStreamSynchronize(h->stream));
    h->prof.resolve();
    h->prof.on = on != 0;
    return GORSE_OK;
}

extern "C" int32_t gorse_sq_get_profile(gorse_sq *h, int32_t cls, int64_t *launches, double *total_ms) {
    if (!h || cls < 0 || cls >= kProfClasses) return fail(GORSE_ERR_INVALID, "bad kernel class");
    GORSE_TRY(h->use());
    GORSE_HIP_CHECK(hipStreamSynchronize(h->stream));
    h->prof.resolve();
    if (launches) *launches = h->prof.launches[cls];
    if (total_ms) *total_ms = h->prof.ms[cls];
    return GORSE_OK;
}
