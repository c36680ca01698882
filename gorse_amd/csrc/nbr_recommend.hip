// nbr_recommend.hip -- gorse_nbr_recommend: recommendItemToItem and recommendUserToUser (logics/recommend.go:244-348) for many
// users at once, as one two-hop weighted walk over two CSR tables resident on the device.
//
// One workgroup per query.  The query's accumulator is an open-addressing table of (int32 item, double sum), slot = item mod slots,
// linear probing; it lies in LDS when the query's bound (nbr_plan.hpp) fits there and in global scratch otherwise -- the same
// kernel, instantiated for either address space.  The seen row goes in first as BLOCKED keys (~item), so exclusion is the probe
// that finds the slot and needs no second structure.
//   Order of additions: the reference adds list after list.  Within one hop-2 list every addend that meets one slot is the same
//   value (unweighted hop 2: w1) or there is only one (weighted hop 2: distinct indices, checked at set_table), so the lanes of a
//   list may add in any order; an addition is a compare-and-swap loop around a plain IEEE add, never the LDS adder.  Across lists
//   the order is kept by construction: a 64-thread workgroup is ONE wave, whose LDS operations complete in order; a 256-thread
//   workgroup passes a barrier between two lists.  nbr_plan.hpp chooses per query: tables of up to 512 slots take the wave form.
//   Selection: order-preserving 64-bit keys from the sums, extended by the complemented item index to 96 bits that are distinct
//   for every live slot; a most-significant-byte-first radix select finds the k-th largest of them (it stops as soon as a byte
//   separates exactly k), the survivors go to an LDS buffer and are ranked there by counting.
#include <algorithm>
#include <cmath>

#include "nbr_internal.hpp"
#include "nbr_plan.hpp"

using namespace gorse;

namespace {

constexpr int kHead = 256;                 // hop-1 entries whose list headers are staged at once
constexpr int32_t kEmpty = INT32_MIN;      // a free slot; a blocked key is ~item (-1 .. -2^31 + 1), a live one the item
constexpr size_t kStageBytes = 6208;       // surv bits 2048 | surv item 1024 | hist 1024 | misc 64 | head weight 2048
static_assert(kStageBytes + (size_t)nbr::kMaxLdsSlots * 12 <= 163840, "the largest table and the staging share 160 KiB");

int32_t g_nbr_lds_slots = 0;    // test hook: > 0 replaces nbr::kMaxLdsSlots
int64_t g_nbr_query_chunk = 0;  // test hook: > 0 = queries per launch at most

struct NbrArgs {
    const int64_t *ptr1, *ptr2;
    const int32_t *idx1, *idx2;
    const float *w1, *w2;  // null: unweighted
    int32_t tr1, tr2;
    double sc1, sc2;
    const int32_t *rows;   // null: query t walks row t
    const int64_t *sptr;   // null: no seen rows
    const int32_t *seen;
    const int32_t *order;  // the launch's queries
    const int32_t *cap;    // global path: slots per query of the launch ...
    const int64_t *off;    // ... and the table's first slot in gkeys / gsums
    int32_t slots;         // LDS path: slots of every table of the launch
    int32_t k;
    int32_t *gkeys;
    unsigned long long *gsums;
    int32_t *out_items;
    unsigned long long *out_sums;
    int32_t *out_cnt;
};

__device__ __forceinline__ double nbr_weight(float raw, int32_t tr, double sc) {
    const double w = (double)raw * sc;
    return tr == GORSE_NBR_RECIP ? 1.0 / (1.0 - w) : w;
}

// larger sum = larger key; -0 as +0; every NaN below every number
__device__ __forceinline__ unsigned long long nbr_sum_key(unsigned long long bits) {
    if ((bits << 1) > 0xffe0000000000000ull) return 0;
    if ((bits << 1) == 0) bits = 0;
    return (bits >> 63) ? ~bits : (bits | 0x8000000000000000ull);
}

// A table in global memory is read past the CU's vector cache: the workgroup's own compare-and-swaps change it in L2.
template <bool LDS>
__device__ __forceinline__ int32_t nbr_key_at(const int32_t *p) {
    if constexpr (LDS)
        return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else
        return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <bool LDS>
__device__ __forceinline__ unsigned long long nbr_sum_at(const unsigned long long *p) {
    if constexpr (LDS)
        return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else
        return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// s_j = (absent ? 0.0 : s_j) + v: every slot's sum starts at +0.0.  The table always keeps a free slot (cap > bound), so the probe ends.
template <bool LDS>
__device__ __forceinline__ void nbr_add(int32_t *keys, unsigned long long *sums, uint32_t cap, int32_t j, double v) {
    uint32_t s = (uint32_t)j % cap;
    for (;;) {
        int32_t kx = nbr_key_at<LDS>(keys + s);
        if (kx == kEmpty) kx = (int32_t)atomicCAS(keys + s, kEmpty, j), kx = kx == kEmpty ? j : kx;
        if (kx == j) break;
        if (kx == ~j) return;  // seen
        s = s + 1 == cap ? 0 : s + 1;
    }
    unsigned long long old = nbr_sum_at<LDS>(sums + s);
    for (;;) {
        const double nv = __longlong_as_double((long long)old) + v;
        const unsigned long long got = atomicCAS(sums + s, old, (unsigned long long)__double_as_longlong(nv));
        if (got == old) break;
        old = got;
    }
}

template <int T, bool LDS>
__global__ __launch_bounds__(T) void nbr_walk_kernel(const NbrArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned long long *sbits = (unsigned long long *)smem;  // the survivors' sums; before the selection: the staged lists' offsets
    int32_t *sitem = (int32_t *)(smem + 2048);               // the survivors' items; before: the staged lists' lengths
    int32_t *hist = (int32_t *)(smem + 3072);
    int32_t *misc = (int32_t *)(smem + 4096);
    double *hw = (double *)(smem + 4160);                    // the staged lists' hop-1 weights
    long long *ha = (long long *)sbits;
    int32_t *hl = sitem;
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int64_t t = A.order[b];
    const int k = A.k;
    uint32_t cap;
    int32_t *keys;
    unsigned long long *sums;
    if constexpr (LDS) {
        cap = (uint32_t)A.slots;
        sums = (unsigned long long *)(smem + kStageBytes);
        keys = (int32_t *)(sums + cap);
    } else {
        cap = (uint32_t)A.cap[b];
        sums = A.gsums + A.off[b];
        keys = A.gkeys + A.off[b];
    }
    const int64_t r = A.rows ? A.rows[t] : t;
    for (uint32_t s = tid; s < cap; s += T) {
        keys[s] = kEmpty;
        sums[s] = 0;
    }
    if (tid == 0) misc[0] = misc[1] = 0;
    if constexpr (!LDS) __threadfence();  // the cleared table is in L2 before any wave's compare-and-swap goes there
    __syncthreads();
    if (r >= 0) {
        if (A.sptr) {
            const int64_t s0 = A.sptr[t], s1 = A.sptr[t + 1];
            for (int64_t e = s0 + tid; e < s1; e += T) {
                const int32_t bk = ~A.seen[e];
                uint32_t s = (uint32_t)A.seen[e] % cap;
                for (;;) {
                    int32_t kx = nbr_key_at<LDS>(keys + s);
                    if (kx == kEmpty) kx = (int32_t)atomicCAS(keys + s, kEmpty, bk), kx = kx == kEmpty ? bk : kx;
                    if (kx == bk) break;
                    s = s + 1 == cap ? 0 : s + 1;
                }
            }
        }
        const int64_t p0 = A.ptr1[r], p1 = A.ptr1[r + 1];
        for (int64_t c0 = p0; c0 < p1; c0 += kHead) {
            const int n = (int)min((int64_t)kHead, p1 - c0);
            __syncthreads();  // the seen row is in; the previous chunk's headers are read
            for (int x = tid; x < n; x += T) {
                const int32_t src = A.idx1[c0 + x];
                const int64_t a = A.ptr2[src];
                ha[x] = a;
                hl[x] = (int32_t)(A.ptr2[src + 1] - a);
                hw[x] = A.w1 ? nbr_weight(A.w1[c0 + x], A.tr1, A.sc1) : 1.0;
            }
            __syncthreads();
            // list x + 1's first entries are fetched while list x is added
            int64_t a = ha[0];
            int32_t len = hl[0], j = 0;
            float raw = 0.0f;
            if (tid < len) {
                j = A.idx2[a + tid];
                if (A.w2) raw = A.w2[a + tid];
            }
            for (int x = 0; x < n; x++) {
                const double w1 = hw[x];
                int64_t na = 0;
                int32_t nl = 0, nj = 0;
                float nraw = 0.0f;
                if (x + 1 < n) {
                    na = ha[x + 1];
                    nl = hl[x + 1];
                    if (tid < nl) {
                        nj = A.idx2[na + tid];
                        if (A.w2) nraw = A.w2[na + tid];
                    }
                }
                if (tid < len) nbr_add<LDS>(keys, sums, cap, j, w1 * (A.w2 ? nbr_weight(raw, A.tr2, A.sc2) : 1.0));
                for (int32_t e = tid + T; e < len; e += T)
                    nbr_add<LDS>(keys, sums, cap, A.idx2[a + e], w1 * (A.w2 ? nbr_weight(A.w2[a + e], A.tr2, A.sc2) : 1.0));
                __syncthreads();  // list x is in before list x + 1 starts (one wave: its table operations complete in order)
                a = na, len = nl, j = nj, raw = nraw;
            }
        }
    }
    __syncthreads();

    // ---- selection: the k-th largest 96-bit key (sum key | ~item) among the live slots
    {
        int live = 0;
        for (uint32_t s = tid; s < cap; s += T) live += nbr_key_at<LDS>(keys + s) >= 0 ? 1 : 0;
        for (int m = 32; m >= 1; m >>= 1) live += __shfl_xor(live, m, 64);
        if ((tid & 63) == 0 && live > 0) atomicAdd(&misc[0], live);
    }
    __syncthreads();
    const int n_live = misc[0];
    unsigned long long pre_hi = 0, mask_hi = 0;
    uint32_t pre_lo = 0, mask_lo = 0;
    if (n_live > k) {
        int need = k;
        for (int d = 11; d >= 0; d--) {
            for (int x = tid; x < 256; x += T) hist[x] = 0;
            __syncthreads();
            for (uint32_t s = tid; s < cap; s += T) {
                const int32_t kx = nbr_key_at<LDS>(keys + s);
                if (kx < 0) continue;
                const unsigned long long sk = nbr_sum_key(nbr_sum_at<LDS>(sums + s));
                const uint32_t lo = ~(uint32_t)kx;
                if ((sk & mask_hi) != pre_hi || (lo & mask_lo) != pre_lo) continue;
                const int byte = d >= 4 ? (int)((sk >> (8 * (d - 4))) & 255) : (int)((lo >> (8 * d)) & 255);
                atomicAdd(&hist[byte], 1);
            }
            __syncthreads();
            if (tid < 64) {  // lane l: bins 4l .. 4l + 3; incl = the entries of the bins of lanes >= l
                const int c0 = hist[4 * tid], c1 = hist[4 * tid + 1], c2 = hist[4 * tid + 2], c3 = hist[4 * tid + 3];
                const int own = c0 + c1 + c2 + c3;
                int incl = own;
                for (int m = 1; m < 64; m <<= 1) {
                    const int o = __shfl_down(incl, m, 64);
                    if (tid + m < 64) incl += o;
                }
                int above = incl - own;
                if (above < need && need <= incl) {
                    int bin = 4 * tid + 3, c = c3;
                    if (above + c < need) above += c, bin--, c = c2;
                    if (above + c < need) above += c, bin--, c = c1;
                    if (above + c < need) above += c, bin--, c = c0;
                    misc[2] = bin;
                    misc[3] = above;
                    misc[4] = c;
                }
            }
            __syncthreads();
            const int bin = misc[2];
            need -= misc[3];
            const int in_bin = misc[4];
            if (d >= 4) {
                pre_hi |= (unsigned long long)bin << (8 * (d - 4));
                mask_hi |= 0xffull << (8 * (d - 4));
            } else {
                pre_lo |= (uint32_t)bin << (8 * d);
                mask_lo |= 0xffu << (8 * d);
            }
            if (in_bin == need) break;  // the bytes fixed so far separate exactly k keys from the rest
        }
    }
    // survivors: the keys whose fixed bytes are >= the prefix (no byte fixed: every live slot)
    for (uint32_t s = tid; s < cap; s += T) {
        const int32_t kx = nbr_key_at<LDS>(keys + s);
        if (kx < 0) continue;
        const unsigned long long bits = nbr_sum_at<LDS>(sums + s);
        const unsigned long long sk = nbr_sum_key(bits) & mask_hi;
        const uint32_t lo = ~(uint32_t)kx & mask_lo;
        if (sk > pre_hi || (sk == pre_hi && lo >= pre_lo)) {
            const int pos = atomicAdd(&misc[1], 1);
            if (pos < kHead) {  // (always: exactly min(k, n_live) <= 256 keys pass)
                sbits[pos] = bits;
                sitem[pos] = kx;
            }
        }
    }
    __syncthreads();
    const int m = min(min(misc[1], k), kHead);
    for (int e = tid; e < m; e += T) {
        const unsigned long long bits = sbits[e], sk = nbr_sum_key(bits);
        const int32_t it = sitem[e];
        int rank = 0;
        for (int x = 0; x < m; x++) {
            const unsigned long long ok = nbr_sum_key(sbits[x]);
            rank += (ok > sk || (ok == sk && sitem[x] < it)) ? 1 : 0;
        }
        A.out_items[t * k + rank] = it;
        A.out_sums[t * k + rank] = bits;
    }
    for (int e = m + tid; e < k; e += T) {
        A.out_items[t * k + e] = -1;
        A.out_sums[t * k + e] = 0;
    }
    if (tid == 0) A.out_cnt[t] = m;
}

}  // namespace

extern "C" void gorse_hip_test_set_nbr(int32_t lds_slots, int64_t query_chunk) {
    g_nbr_lds_slots = lds_slots > 0 ? std::min(lds_slots, nbr::kMaxLdsSlots) : 0;
    g_nbr_query_chunk = query_chunk > 0 ? query_chunk : 0;
}

extern "C" int32_t gorse_nbr_create(gorse_nbr **out, int32_t device, int64_t n_items) {
    if (!out) return fail(GORSE_ERR_INVALID, "handle pointer is NULL");
    *out = nullptr;
    if (n_items < 1 || n_items > INT32_MAX) return fail(GORSE_ERR_INVALID, "n_items = %lld outside 1 .. 2^31 - 1", (long long)n_items);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(GORSE_ERR_NO_DEVICE, "no HIP device visible (libgorse_hip needs an MI355X / gfx950)");
    if (device < 0 || device >= ndev) return fail(GORSE_ERR_INVALID, "device %d out of range [0,%d)", device, ndev);
    gorse_nbr *h = new (std::nothrow) gorse_nbr();
    if (!h) return fail(GORSE_ERR_NOMEM, "out of host memory");
    h->device = device;
    h->n_items = n_items;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete h;
        return fail(GORSE_ERR_HIP, "gorse_nbr_create: %s", hipGetErrorString(e));
    }
    *out = h;
    return GORSE_OK;
}

extern "C" int32_t gorse_nbr_destroy(gorse_nbr *h) {
    if (!h) return GORSE_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) {
        (void)hipStreamSynchronize(h->stream);
        (void)hipStreamDestroy(h->stream);
    }
    delete h;
    return GORSE_OK;
}

extern "C" int32_t gorse_nbr_set_table(gorse_nbr *h, int32_t which, int64_t n_rows, const int64_t *indptr, const int32_t *indices,
                                       const float *weights, int32_t transform, double scale) {
    if (!h) return fail(GORSE_ERR_INVALID, "handle is NULL");
    std::string msg;
    int64_t max_index = -1;
    const int32_t rc = nbr::validate_table(which, n_rows, indptr, indices, weights, transform, scale, h->n_items, &max_index, &msg);
    if (rc != GORSE_OK) return fail(rc, "gorse_nbr_set_table: %s", msg.c_str());
    GORSE_TRY(h->use());
    const int64_t nnz = indptr[n_rows];
    // the new table stands on the device before the old one goes
    DevBuf<int64_t> d_ptr;
    DevBuf<int32_t> d_idx;
    DevBuf<float> d_w;
    GORSE_TRY(d_ptr.alloc((size_t)n_rows + 1));
    GORSE_TRY(d_idx.alloc((size_t)nnz));
    if (weights) GORSE_TRY(d_w.alloc((size_t)nnz));
    GORSE_HIP_CHECK(hipStreamSynchronize(h->stream));
    GORSE_HIP_CHECK(hipMemcpy(d_ptr.p, indptr, (size_t)(n_rows + 1) * 8, hipMemcpyHostToDevice));
    if (nnz > 0) GORSE_HIP_CHECK(hipMemcpy(d_idx.p, indices, (size_t)nnz * 4, hipMemcpyHostToDevice));
    if (nnz > 0 && weights) GORSE_HIP_CHECK(hipMemcpy(d_w.p, weights, (size_t)nnz * 4, hipMemcpyHostToDevice));
    NbrTable &T = h->tab[which];
    T.set = true;
    T.weighted = weights != nullptr;
    T.n_rows = n_rows;
    T.nnz = nnz;
    T.max_index = max_index;
    T.transform = weights ? transform : GORSE_NBR_RAW;
    T.scale = weights ? scale : 1.0;
    T.on_device_only = false;
    T.ptr.assign(indptr, indptr + n_rows + 1);
    if (which == GORSE_NBR_HOP1)
        T.idx.assign(indices, indices + nnz);
    std::swap(T.d_ptr.p, d_ptr.p), std::swap(T.d_ptr.n, d_ptr.n);
    std::swap(T.d_idx.p, d_idx.p), std::swap(T.d_idx.n, d_idx.n);
    std::swap(T.d_w.p, d_w.p), std::swap(T.d_w.n, d_w.n);
    h->bounds_valid = false;
    return GORSE_OK;
}

extern "C" int32_t gorse_nbr_recommend_stats(gorse_nbr *h, int64_t *n_lds, int64_t *n_global, double *device_ms) {
    if (!h) return fail(GORSE_ERR_INVALID, "handle is NULL");
    if (n_lds) *n_lds = h->n_lds;
    if (n_global) *n_global = h->n_global;
    if (device_ms) *device_ms = h->ms;
    return GORSE_OK;
}

namespace {

template <int T, bool LDS>
int32_t nbr_launch(const NbrArgs &A, int64_t nq, size_t lds, hipStream_t stream) {
    if (lds > 65536)
        GORSE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&nbr_walk_kernel<T, LDS>),
                                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    nbr_walk_kernel<T, LDS><<<dim3((unsigned)nq), dim3(T), lds, stream>>>(A);
    GORSE_HIP_CHECK(hipGetLastError());
    return GORSE_OK;
}

}  // namespace

namespace gorse {

int32_t nbr_recommend_check(gorse_nbr *h, const char *who, int64_t n_queries, const int32_t *rows, int32_t k, const int64_t *seen_indptr,
                            const int32_t *seen_items) {
    NbrTable &T1 = h->tab[GORSE_NBR_HOP1], &T2 = h->tab[GORSE_NBR_HOP2];
    if (!T1.set || !T2.set) return fail(GORSE_ERR_INVALID, "%s: the hop-%d table is not set", who, T1.set ? 2 : 1);
    std::string msg;
    const int32_t rc = nbr::validate_call(n_queries, rows, k, seen_indptr, seen_items, T1.n_rows, h->n_items, &msg);
    if (rc != GORSE_OK) return fail(rc, "%s: %s", who, msg.c_str());
    if (T1.max_index >= T2.n_rows)
        return fail(GORSE_ERR_RANGE, "%s: hop-1 index %lld outside the hop-2 table's %lld rows", who, (long long)T1.max_index,
                    (long long)T2.n_rows);
    return GORSE_OK;
}

int32_t nbr_recommend_core(gorse_nbr *h, int64_t n_queries, const int32_t *rows, int32_t k, const int64_t *sptr_host,
                           const int64_t *d_sptr, const int32_t *d_seen, NbrDeviceRows *res) {
    NbrTable &T1 = h->tab[GORSE_NBR_HOP1], &T2 = h->tab[GORSE_NBR_HOP2];
    GORSE_TRY(h->use());
    h->n_lds = h->n_global = 0;
    h->ms = 0.0;
    *res = NbrDeviceRows();
    if (n_queries == 0) return GORSE_OK;
    if (!h->bounds_valid) {
        if (T1.on_device_only)  // its indices never crossed to the host: the same sums, formed where they lie
            GORSE_TRY(nbr_device_row_bounds(h, &h->src_sum));
        else
            nbr::row_bounds(T1.n_rows, T1.ptr.data(), T1.idx.data(), T2.ptr.data(), &h->src_sum);
        h->bounds_valid = true;
    }
    const bool has_seen = sptr_host != nullptr;
    std::vector<int64_t> bound((size_t)n_queries);
    for (int64_t t = 0; t < n_queries; t++) {
        const int64_t r = rows ? rows[t] : t;
        bound[(size_t)t] = r < 0 ? 0 : nbr::query_bound(h->n_items, h->src_sum[(size_t)r], has_seen ? sptr_host[t + 1] - sptr_host[t] : 0);
    }
    nbr::Plan plan;
    if (!nbr::make_plan(n_queries, bound.data(), g_nbr_lds_slots > 0 ? g_nbr_lds_slots : nbr::kMaxLdsSlots, g_nbr_query_chunk,
                        nbr::kScratchSlots, &plan))
        return fail(GORSE_ERR_NOMEM, "gorse_nbr_recommend: a query's table exceeds 2^31 - 1 slots");
    int64_t scratch_slots = 0;
    for (const nbr::Launch &L : plan.launches)
        if (L.slots == 0) scratch_slots = std::max(scratch_slots, plan.off[(size_t)L.q1 - 1] + plan.cap[(size_t)L.q1 - 1]);

    // ---- the rows asked for and the plan to the device
    Carver in;
    const size_t o_rows = in.take((size_t)n_queries * 4), o_order = in.take((size_t)n_queries * 4), o_cap = in.take((size_t)n_queries * 4),
                 o_off = in.take((size_t)n_queries * 8);
    GORSE_TRY(h->in.ensure(in.off));
    Carver oc;
    const size_t o_items = oc.take((size_t)n_queries * k * 4), o_sums = oc.take((size_t)n_queries * k * 8), o_cnt = oc.take((size_t)n_queries * 4);
    GORSE_TRY(h->out.ensure(oc.off));
    Carver sc;
    const size_t o_gsums = sc.take((size_t)scratch_slots * 8), o_gkeys = sc.take((size_t)scratch_slots * 4);
    GORSE_TRY(h->scratch.ensure(sc.off));
    hipStream_t st = h->stream;
    if (rows) GORSE_HIP_CHECK(hipMemcpyAsync(h->in.p + o_rows, rows, (size_t)n_queries * 4, hipMemcpyHostToDevice, st));
    GORSE_HIP_CHECK(hipMemcpyAsync(h->in.p + o_order, plan.order.data(), (size_t)n_queries * 4, hipMemcpyHostToDevice, st));
    GORSE_HIP_CHECK(hipMemcpyAsync(h->in.p + o_cap, plan.cap.data(), (size_t)n_queries * 4, hipMemcpyHostToDevice, st));
    GORSE_HIP_CHECK(hipMemcpyAsync(h->in.p + o_off, plan.off.data(), (size_t)n_queries * 8, hipMemcpyHostToDevice, st));

    NbrArgs A{};
    A.ptr1 = T1.d_ptr.p, A.idx1 = T1.d_idx.p, A.w1 = T1.weighted ? T1.d_w.p : nullptr, A.tr1 = T1.transform, A.sc1 = T1.scale;
    A.ptr2 = T2.d_ptr.p, A.idx2 = T2.d_idx.p, A.w2 = T2.weighted ? T2.d_w.p : nullptr, A.tr2 = T2.transform, A.sc2 = T2.scale;
    A.rows = rows ? (const int32_t *)(h->in.p + o_rows) : nullptr;
    A.sptr = has_seen ? d_sptr : nullptr;
    A.seen = d_seen;
    A.k = k;
    A.gsums = (unsigned long long *)(h->scratch.p + o_gsums);
    A.gkeys = (int32_t *)(h->scratch.p + o_gkeys);
    A.out_items = (int32_t *)(h->out.p + o_items);
    A.out_sums = (unsigned long long *)(h->out.p + o_sums);
    A.out_cnt = (int32_t *)(h->out.p + o_cnt);

    hipEvent_t ev_a = nullptr, ev_b = nullptr;
    GORSE_HIP_CHECK(hipEventCreate(&ev_a));
    if (hipEventCreate(&ev_b) != hipSuccess) {
        (void)hipEventDestroy(ev_a);
        return fail(GORSE_ERR_HIP, "gorse_nbr_recommend: hipEventCreate");
    }
    int32_t rc = [&]() -> int32_t {
        GORSE_HIP_CHECK(hipEventRecord(ev_a, st));
        for (const nbr::Launch &L : plan.launches) {
            A.order = (const int32_t *)(h->in.p + o_order) + L.q0;
            A.cap = (const int32_t *)(h->in.p + o_cap) + L.q0;
            A.off = (const int64_t *)(h->in.p + o_off) + L.q0;
            A.slots = L.slots;
            const int64_t nq = L.q1 - L.q0;
            if (L.slots == 0)
                GORSE_TRY((nbr_launch<256, false>(A, nq, kStageBytes, st)));
            else if (L.threads == 64)
                GORSE_TRY((nbr_launch<64, true>(A, nq, kStageBytes + (size_t)L.slots * 12, st)));
            else
                GORSE_TRY((nbr_launch<256, true>(A, nq, kStageBytes + (size_t)L.slots * 12, st)));
        }
        GORSE_HIP_CHECK(hipEventRecord(ev_b, st));
        GORSE_HIP_CHECK(hipEventSynchronize(ev_b));
        float ms = 0.0f;
        GORSE_HIP_CHECK(hipEventElapsedTime(&ms, ev_a, ev_b));
        h->ms = ms;
        return GORSE_OK;
    }();
    (void)hipEventDestroy(ev_a);
    (void)hipEventDestroy(ev_b);
    GORSE_TRY(rc);
    res->items = A.out_items, res->sums = A.out_sums, res->cnt = A.out_cnt;
    h->n_lds = plan.n_lds;
    h->n_global = plan.n_global;
    return GORSE_OK;
}

}  // namespace gorse

extern "C" int32_t gorse_nbr_recommend(gorse_nbr *h, int64_t n_queries, const int32_t *rows, int32_t k, const int64_t *seen_indptr,
                                       const int32_t *seen_items, int32_t *items_out, double *scores_out, int32_t *count_out) {
    if (!h) return fail(GORSE_ERR_INVALID, "handle is NULL");
    GORSE_TRY(nbr_recommend_check(h, "gorse_nbr_recommend", n_queries, rows, k, seen_indptr, seen_items));
    GORSE_TRY(h->use());
    // ---- the seen rows to the device; the core walks from device rows (the candidate chain hands it its own)
    const bool has_seen = n_queries > 0 && seen_indptr && seen_indptr[n_queries] > seen_indptr[0];
    const int64_t n_seen = has_seen ? seen_indptr[n_queries] - seen_indptr[0] : 0;
    std::vector<int64_t> sptr_host;
    Carver in;
    const size_t o_sptr = in.take((size_t)(n_queries + 1) * 8), o_seen = in.take((size_t)std::max<int64_t>(n_seen, 1) * 4);
    hipStream_t st = h->stream;
    if (has_seen) {
        GORSE_TRY(h->seen_in.ensure(in.off));
        sptr_host.resize((size_t)n_queries + 1);
        for (int64_t t = 0; t <= n_queries; t++) sptr_host[(size_t)t] = seen_indptr[t] - seen_indptr[0];
        GORSE_HIP_CHECK(hipMemcpyAsync(h->seen_in.p + o_sptr, sptr_host.data(), (size_t)(n_queries + 1) * 8, hipMemcpyHostToDevice, st));
        GORSE_HIP_CHECK(hipMemcpyAsync(h->seen_in.p + o_seen, seen_items + seen_indptr[0], (size_t)n_seen * 4, hipMemcpyHostToDevice, st));
    }
    NbrDeviceRows R;
    GORSE_TRY(nbr_recommend_core(h, n_queries, rows, k, has_seen ? sptr_host.data() : nullptr,
                                 has_seen ? (const int64_t *)(h->seen_in.p + o_sptr) : nullptr,
                                 has_seen ? (const int32_t *)(h->seen_in.p + o_seen) : nullptr, &R));
    if (n_queries == 0) return GORSE_OK;
    if (items_out) GORSE_HIP_CHECK(hipMemcpyAsync(items_out, R.items, (size_t)n_queries * k * 4, hipMemcpyDeviceToHost, st));
    if (scores_out) GORSE_HIP_CHECK(hipMemcpyAsync(scores_out, R.sums, (size_t)n_queries * k * 8, hipMemcpyDeviceToHost, st));
    if (count_out) GORSE_HIP_CHECK(hipMemcpyAsync(count_out, R.cnt, (size_t)n_queries * 4, hipMemcpyDeviceToHost, st));
    GORSE_HIP_CHECK(hipStreamSynchronize(st));
    return GORSE_OK;
}
