// fm_eval.hip -- EvaluateClassification (model/ctr/evaluator.go:46-153) from a test split that stays on the device.
//
// gorse_fm_set_test partitions the test rows once (positives first, then the others, each side in dataset order), gathers their
// embeddings once and keeps all of it resident.  gorse_fm_evaluate scores the two sides as BatchInternalPredict would score them
// (fm.go:156-178: slices of batch_size rows, each side sliced on its own) through score_rounds (fm_resident.hip: the kernels of
// gorse_fm_predict_embeddings, so the same bits, many slices per launch; the rows are the split's padded rows, and a row's
// embedding is its own row of the split's tables), and forms the metrics' raw counts on the device:
//   fm_eval_keys_kernel      order-preserving keys of the logits (-0 folded onto +0, NaN = 0xffffffff: sorts last), and the
//                            threshold tallies (positives > 0, negatives > 0, negatives < 0, NaNs per side) in the same pass
//   fm_eval_sort_*_kernel    an LSD radix sort of the two sides' keys, 8 bits a pass: per-tile digit counts into a digit x tile
//                            matrix, one exclusive scan over it, a stable scatter (ranks inside a wave by ballots, across the
//                            waves through LDS; no global atomic).  Both sides in one launch (blockIdx.y).  Deterministic.
//   fm_eval_count_kernel     per positive (ascending) the negatives strictly below it: a lower bound in the sorted negatives;
//                            their exact 64-bit total is pairs_less
//   fm_eval_chain_kernel     AUC's running float32 sum (evaluator.go:139-148) over those counts in order: one wave, 64 counts
//                            loaded at a time and added one after the other; exact integers up to 2^24 are not chained
#include "fm_internal.hpp"
#include "fm_eval_plan.hpp"
#include "rank_keys.hpp"

namespace gorse {
namespace fm {

constexpr int64_t kEvalSortTile = 4096;   // keys per sort workgroup
constexpr int64_t kEvalMaxTiles = 65536;  // tiles per side at most: beyond, the tile grows
constexpr uint32_t kNanKey = 0xffffffffu;
// slots of gorse_fm::e_acc
enum { kAccPosAbove = 0, kAccNegAbove, kAccNegBelow, kAccNanPos, kAccNanNeg, kAccPairs, kAccAuc, kAccSlots };

// test hooks (gorse_hip_test_set_fm_evaluate): 0 = the library's choice
static int64_t g_eval_round_rows = 0;
static int64_t g_eval_sort_tile = 0;

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

struct KeyArgs {
    const float *logit;  // the positives, then the negatives
    int64_t n, n_pos;
    uint32_t *key;
    unsigned long long *acc;
};

__global__ __launch_bounds__(kBlock) void fm_eval_keys_kernel(KeyArgs a) {
    __shared__ unsigned int tally[5];
    if (threadIdx.x < 5) tally[threadIdx.x] = 0;
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    bool f[5] = {false, false, false, false, false};
    if (i < a.n) {
        const float x = a.logit[i];
        const bool pos = i < a.n_pos, nan = x != x;
        a.key[i] = nan ? kNanKey : rank::score_ord(x);
        f[kAccPosAbove] = pos && x > 0.0f;
        f[kAccNegAbove] = !pos && x > 0.0f;
        f[kAccNegBelow] = !pos && x < 0.0f;
        f[kAccNanPos] = pos && nan;
        f[kAccNanNeg] = !pos && nan;
    }
#pragma unroll
    for (int k = 0; k < 5; k++) {
        const unsigned int c = (unsigned int)__popcll(__ballot(f[k]));
        if ((threadIdx.x & 63) == 0 && c) atomicAdd(&tally[k], c);
    }
    __syncthreads();
    if (threadIdx.x < 5 && tally[threadIdx.x]) atomicAdd(&a.acc[threadIdx.x], (unsigned long long)tally[threadIdx.x]);
}

// one side of the sort: n keys in tiles of `tile`, counts / offsets in hist[digit x ntiles + tile]
struct SortSeg {
    const uint32_t *in;
    uint32_t *out;
    uint32_t *hist;
    int64_t n, tile, ntiles;
};
struct SortArgs {
    SortSeg pos, neg;
    int shift;
};

// the side of blockIdx `which`, chosen field by field (no private copy of the argument block)
__device__ __forceinline__ SortSeg pick_seg(const SortArgs &a, unsigned which) {
    SortSeg s;
    s.in = which ? a.neg.in : a.pos.in;
    s.out = which ? a.neg.out : a.pos.out;
    s.hist = which ? a.neg.hist : a.pos.hist;
    s.n = which ? a.neg.n : a.pos.n;
    s.tile = which ? a.neg.tile : a.pos.tile;
    s.ntiles = which ? a.neg.ntiles : a.pos.ntiles;
    return s;
}

__global__ __launch_bounds__(kBlock) void fm_eval_sort_count_kernel(SortArgs a) {
    __shared__ unsigned int cnt[256];
    const SortSeg s = pick_seg(a, blockIdx.y);
    if ((int64_t)blockIdx.x >= s.ntiles) return;  // the whole workgroup
    cnt[threadIdx.x] = 0;
    __syncthreads();
    const int64_t t0 = (int64_t)blockIdx.x * s.tile, t1 = t0 + s.tile < s.n ? t0 + s.tile : s.n;
    for (int64_t i = t0 + threadIdx.x; i < t1; i += kBlock) atomicAdd(&cnt[(s.in[i] >> a.shift) & 255u], 1u);
    __syncthreads();
    s.hist[(int64_t)threadIdx.x * s.ntiles + blockIdx.x] = cnt[threadIdx.x];
}

// exclusive scan over a side's digit x tile matrix, in place: one workgroup per side walks it 256 entries at a time
__global__ __launch_bounds__(kBlock) void fm_eval_sort_scan_kernel(SortArgs a) {
    __shared__ uint32_t wsum[kBlock / 64];
    const SortSeg s = pick_seg(a, blockIdx.x);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t total = 256 * s.ntiles;
    uint32_t carry = 0;
    for (int64_t base = 0; base < total; base += kBlock) {
        const int64_t i = base + threadIdx.x;
        const uint32_t v = i < total ? s.hist[i] : 0u;
        uint32_t incl = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        if (lane == 63) wsum[w] = incl;
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (int k = 0; k < kBlock / 64; k++) {
            const uint32_t x = wsum[k];
            if (k < w) before += x;
            all += x;
        }
        if (i < total) s.hist[i] = carry + before + incl - v;
        carry += all;
        __syncthreads();
    }
}

// Stable scatter of a tile by the pass's digit.  The tile is walked 256 keys at a time in order; a key's place is the digit's
// running base + the keys of that digit in the chunk's earlier waves + those in earlier lanes of its own wave.
__global__ __launch_bounds__(kBlock) void fm_eval_sort_scatter_kernel(SortArgs a) {
    __shared__ uint32_t base[256];
    __shared__ uint32_t wcnt[kBlock / 64][256];
    const SortSeg s = pick_seg(a, blockIdx.y);
    if ((int64_t)blockIdx.x >= s.ntiles) return;  // the whole workgroup
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    base[threadIdx.x] = s.hist[(int64_t)threadIdx.x * s.ntiles + blockIdx.x];
#pragma unroll
    for (int k = 0; k < kBlock / 64; k++) wcnt[k][threadIdx.x] = 0;
    __syncthreads();
    const int64_t t0 = (int64_t)blockIdx.x * s.tile, t1 = t0 + s.tile < s.n ? t0 + s.tile : s.n;
    for (int64_t c0 = t0; c0 < t1; c0 += kBlock) {
        const int64_t i = c0 + threadIdx.x;
        const bool live = i < t1;
        const uint32_t key = live ? s.in[i] : 0u;
        const uint32_t digit = (key >> a.shift) & 255u;
        // the wave's lanes that hold the same digit
        uint64_t same = __ballot(live);
#pragma unroll
        for (int b = 0; b < 8; b++) {
            const bool bit = (digit >> b) & 1u;
            const uint64_t m = __ballot(bit);
            same &= bit ? m : ~m;
        }
        const uint32_t rank = (uint32_t)__popcll(same & (((uint64_t)1 << lane) - 1));
        if (live && rank == 0) wcnt[w][digit] = (uint32_t)__popcll(same);  // one writer per digit and wave
        __syncthreads();
        if (live) {
            uint32_t at = base[digit] + rank;
#pragma unroll
            for (int k = 0; k < kBlock / 64; k++)
                if (k < w) at += wcnt[k][digit];
            if ((int64_t)at < s.n) s.out[at] = key;  // always true for counts that match the keys
        }
        __syncthreads();
        uint32_t add = 0;
#pragma unroll
        for (int k = 0; k < kBlock / 64; k++) {
            add += wcnt[k][threadIdx.x];
            wcnt[k][threadIdx.x] = 0;
        }
        base[threadIdx.x] += add;
        __syncthreads();
    }
}

struct CountArgs {
    const uint32_t *pos, *neg;  // sorted keys, the NaNs at each side's end
    int64_t n_pos, n_neg;
    uint32_t *cnt;  // per positive, ascending
    unsigned long long *acc;
};

__global__ __launch_bounds__(kBlock) void fm_eval_count_kernel(CountArgs a) {
    __shared__ unsigned long long part[kBlock / 64];
    const int64_t np = a.n_pos - (int64_t)a.acc[kAccNanPos], nn = a.n_neg - (int64_t)a.acc[kAccNanNeg];
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    uint64_t c = 0;
    if (i < np) {
        const uint32_t k = a.pos[i];
        int64_t lo = 0, hi = nn;
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (a.neg[mid] < k)
                lo = mid + 1;
            else
                hi = mid;
        }
        c = (uint64_t)lo;
        a.cnt[i] = (uint32_t)lo;
    }
    c = wave_sum_u64(c);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
#pragma unroll
        for (int k = 0; k < kBlock / 64; k++) t += part[k];
        if (t) atomicAdd(&a.acc[kAccPairs], t);
    }
}

// sum += float32(count), count by count (evaluator.go:139-148).  While the exact total stays within 2^24 every partial sum is an
// integer the format holds, so the float equals it and nothing needs to be chained; from there on every step may round, and
// lane order is the only order: the counts of 64 positives come out of the wave's registers one after the other.
__global__ __launch_bounds__(64) void fm_eval_chain_kernel(const uint32_t *cnt, int64_t n_pos, unsigned long long *acc) {
    const int lane = threadIdx.x;
    const int64_t n = n_pos - (int64_t)acc[kAccNanPos];
    uint64_t exact = 0;
    float s = 0.0f;
    bool fast = true;
    for (int64_t b = 0; b < n; b += 64) {
        const uint32_t c = b + lane < n ? cnt[b + lane] : 0u;
        if (fast) {
            const uint64_t t = wave_sum_u64(c);
            if (exact + t <= ((uint64_t)1 << 24)) {
                exact += t;
                s = (float)exact;
                continue;
            }
            fast = false;
        }
        const uint32_t f = __float_as_uint((float)c);  // the tail's zeros add nothing: s is never -0
#pragma unroll
        for (int j = 0; j < 64; j++) s = s + __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)f, j));
    }
    if (lane == 0) acc[kAccAuc] = (unsigned long long)__float_as_uint(s);
}

int64_t sort_tile_for(int64_t n) {
    int64_t tile = g_eval_sort_tile > 0 ? g_eval_sort_tile : kEvalSortTile;
    if (ceil_div(n, tile) > kEvalMaxTiles) tile = ceil_div(ceil_div(n, kEvalMaxTiles), kBlock) * kBlock;
    return tile;
}

// The metric stage on h->e_logit = n_pos positives' logits, then n_neg negatives': enqueued on the handle's stream; records
// e_ev[2] before the chain and e_ev[3] after it.
int32_t enqueue_metrics(gorse_fm *h, int64_t n_pos, int64_t n_neg) {
    const int64_t n = n_pos + n_neg;
    GORSE_TRY(h->e_acc.ensure(kAccSlots));
    GORSE_HIP_CHECK(hipMemsetAsync(h->e_acc.p, 0, kAccSlots * sizeof(uint64_t), h->s));
    if (n > 0) {
        const int64_t tile_p = sort_tile_for(n_pos), tile_n = sort_tile_for(n_neg);
        const int64_t nt_p = ceil_div(n_pos, tile_p), nt_n = ceil_div(n_neg, tile_n);
        GORSE_TRY(h->e_key[0].ensure((size_t)n));
        GORSE_TRY(h->e_key[1].ensure((size_t)n));
        GORSE_TRY(h->e_hist.ensure((size_t)(256 * (nt_p + nt_n))));
        GORSE_TRY(h->e_cnt.ensure((size_t)std::max<int64_t>(n_pos, 1)));
        auto *acc = reinterpret_cast<unsigned long long *>(h->e_acc.p);
        KeyArgs k{h->e_logit.p, n, n_pos, h->e_key[0].p, acc};
        fm_eval_keys_kernel<<<dim3((unsigned)ceil_div(n, kBlock)), dim3(kBlock), 0, h->s>>>(k);
        const unsigned gx = (unsigned)std::max<int64_t>(1, std::max(nt_p, nt_n));
        for (int pass = 0; pass < 4; pass++) {  // an even number of passes: the sorted keys end in e_key[0]
            const uint32_t *in = h->e_key[pass & 1].p;
            uint32_t *out = h->e_key[(pass & 1) ^ 1].p;
            SortArgs s{};
            s.pos = SortSeg{in, out, h->e_hist.p, n_pos, tile_p, nt_p};
            s.neg = SortSeg{in + n_pos, out + n_pos, h->e_hist.p + 256 * nt_p, n_neg, tile_n, nt_n};
            s.shift = 8 * pass;
            fm_eval_sort_count_kernel<<<dim3(gx, 2), dim3(kBlock), 0, h->s>>>(s);
            fm_eval_sort_scan_kernel<<<dim3(2), dim3(kBlock), 0, h->s>>>(s);
            fm_eval_sort_scatter_kernel<<<dim3(gx, 2), dim3(kBlock), 0, h->s>>>(s);
        }
        if (n_pos > 0) {
            CountArgs c{h->e_key[0].p, h->e_key[0].p + n_pos, n_pos, n_neg, h->e_cnt.p, acc};
            fm_eval_count_kernel<<<dim3((unsigned)ceil_div(n_pos, kBlock)), dim3(kBlock), 0, h->s>>>(c);
        }
        GORSE_HIP_CHECK(hipGetLastError());
    }
    GORSE_HIP_CHECK(hipEventRecord(h->e_ev[2], h->s));
    if (n_pos > 0) {
        fm_eval_chain_kernel<<<dim3(1), dim3(64), 0, h->s>>>(h->e_cnt.p, n_pos, reinterpret_cast<unsigned long long *>(h->e_acc.p));
        GORSE_HIP_CHECK(hipGetLastError());
    }
    GORSE_HIP_CHECK(hipEventRecord(h->e_ev[3], h->s));
    return GORSE_OK;
}

// after the stream drained: the seven counts, the chain's sum and the stage times
int32_t read_metrics(gorse_fm *h, int64_t n_pos, int64_t n_neg, int64_t *counts, float *auc_sum) {
    uint64_t acc[kAccSlots];
    GORSE_HIP_CHECK(hipMemcpy(acc, h->e_acc.p, sizeof(acc), hipMemcpyDeviceToHost));
    if (counts) {
        counts[0] = n_pos, counts[1] = n_neg;
        counts[2] = (int64_t)acc[kAccPosAbove], counts[3] = (int64_t)acc[kAccNegAbove], counts[4] = (int64_t)acc[kAccNegBelow];
        counts[5] = (int64_t)(acc[kAccNanPos] + acc[kAccNanNeg]);
        counts[6] = (int64_t)acc[kAccPairs];
    }
    if (auc_sum) {
        const uint32_t bits = (uint32_t)acc[kAccAuc];
        memcpy(auc_sum, &bits, 4);
    }
    float ms[3] = {0.0f, 0.0f, 0.0f};
    for (int k = 0; k < 3; k++) GORSE_HIP_CHECK(hipEventElapsedTime(&ms[k], h->e_ev[k], h->e_ev[k + 1]));
    h->ev_ms[1] = ms[0], h->ev_ms[2] = ms[1], h->ev_ms[3] = ms[2];
    h->ev_ms[0] = (double)ms[0] + ms[1] + ms[2];
    return GORSE_OK;
}

}  // namespace fm
}  // namespace gorse

using namespace gorse;

extern "C" void gorse_hip_test_set_fm_evaluate(int64_t round_rows, int32_t sort_tile) {
    fm::g_eval_round_rows = round_rows > 0 ? round_rows : 0;
    fm::g_eval_sort_tile = sort_tile > 0 ? sort_tile : 0;
}

extern "C" int32_t gorse_fm_set_test(gorse_fm *h, int64_t n, int32_t width, const int32_t *indices, const float *values,
                                     const float *target, const uint16_t *const *emb) {
    if (!h) return fail(GORSE_ERR_INVALID, "handle is NULL");
    if (n < 0 || n > INT32_MAX) return fail(GORSE_ERR_INVALID, "n must be in [0, 2^31)");
    GORSE_HIP_CHECK(hipSetDevice(h->device));
    if (n == 0) {
        GORSE_HIP_CHECK(hipStreamSynchronize(h->s));
        h->test.reset();
        h->test_dropped = false;
        return GORSE_OK;
    }
    if (width <= 0) return fail(GORSE_ERR_INVALID, "width must be positive (got %d)", width);
    if (!indices || !values || !target) return fail(GORSE_ERR_INVALID, "indices / values / target is NULL");
    const int64_t ne = n * (int64_t)width;
    for (int64_t e = 0; e < ne; e++)
        if (indices[e] < 0 || indices[e] >= h->nf)
            return fail(GORSE_ERR_RANGE, "feature index %d at position %lld out of range [0,%lld)", indices[e], (long long)e,
                        (long long)h->nf);
    GORSE_TRY(fm::check_emb(h, emb));
    double bytes = (double)ne * 8 + (double)n * 12;
    for (int k = 0; k < h->n_fields; k++) bytes += (double)n * h->fld[k].D * 2;
    GORSE_TRY(fm::check_fits(bytes, "test split"));
    // built beside the resident one, which stays until the new one is complete
    std::unique_ptr<fm::TestSplit> t(new (std::nothrow) fm::TestSplit());
    if (!t) return fail(GORSE_ERR_NOMEM, "out of host memory");
    t->n = n, t->width = width;
    t->n_pos = fm::eval_partition(target, n, t->order);
    {
        std::vector<int32_t> pi((size_t)ne);
        std::vector<float> pv((size_t)ne);
        for (int64_t r = 0; r < n; r++) {
            const int64_t src = (int64_t)t->order[(size_t)r] * width;
            std::copy(indices + src, indices + src + width, pi.begin() + r * width);
            std::copy(values + src, values + src + width, pv.begin() + r * width);
        }
        GORSE_TRY(fm::upload(t->idx, pi.data(), (size_t)ne));
        GORSE_TRY(fm::upload(t->val, pv.data(), (size_t)ne));
    }
    // the embedding rows gathered through a bounded staging buffer
    for (int k = 0; k < h->n_fields; k++) {
        const int32_t D = h->fld[k].D;
        GORSE_TRY(t->emb[k].alloc((size_t)fm::eval_emb_offset(n, D)));
        const int64_t chunk = std::max<int64_t>(1, ((int64_t)32 << 20) / D);
        std::vector<uint16_t> stage((size_t)(std::min(chunk, n) * D));
        for (int64_t r0 = 0; r0 < n; r0 += chunk) {
            const int64_t nr = std::min(chunk, n - r0);
            for (int64_t r = 0; r < nr; r++) {
                const uint16_t *src = emb[k] + fm::eval_emb_offset(t->order[(size_t)(r0 + r)], D);
                std::copy(src, src + D, stage.begin() + r * D);
            }
            GORSE_HIP_CHECK(hipMemcpy(t->emb[k].p + fm::eval_emb_offset(r0, D), stage.data(), (size_t)(nr * D) * sizeof(uint16_t),
                                      hipMemcpyHostToDevice));
        }
    }
    GORSE_HIP_CHECK(hipStreamSynchronize(h->s));
    h->test = std::move(t);
    h->test_dropped = false;
    return GORSE_OK;
}

extern "C" int32_t gorse_fm_evaluate(gorse_fm *h, int32_t batch_size, const volatile int32_t *cancel, int64_t *counts,
                                     float *auc_sum, float *logits_out) {
    if (!h) return fail(GORSE_ERR_INVALID, "handle is NULL");
    if (!h->test && h->test_dropped)
        return fail(GORSE_ERR_INVALID, "the sample-form test split was dropped when the item catalogue it indexed was replaced or "
                                       "dropped (gorse_fm_set_items, gorse_fm_set_embedding_dims): set it again");
    if (!h->test) return fail(GORSE_ERR_INVALID, "no resident test split (gorse_fm_set_test)");
    if (h->test->samples && !h->cat) return fail(GORSE_ERR_INVALID, "the sample-form test split has no item catalogue");
    if (batch_size <= 0) return fail(GORSE_ERR_INVALID, "batch_size must be positive");
    GORSE_HIP_CHECK(hipSetDevice(h->device));
    fm::TestSplit &t = *h->test;
    const int64_t n = t.n, n_pos = t.n_pos;

    // slices and launch rounds: built once per (split, batch size, rows of a round)
    const int maxD = fm::max_emb_dim(h);
    const int64_t R = fm::round_rows_for(maxD, h->d, batch_size, fm::g_eval_round_rows);
    if (t.plan_bs != batch_size || t.plan_rows != R) {
        const int64_t sides[3] = {0, n_pos, n};
        fm::SlicePlan plan;
        // sample form: a row's descriptor is (its user, its item) instead of (its side, its own number)
        fm::plan_slices(sides, 2, t.samples ? t.s_item.data() : nullptr, batch_size, R, plan);
        if (t.samples) std::copy(t.s_user.begin(), t.s_user.end(), plan.desc.begin());
        GORSE_HIP_CHECK(hipStreamSynchronize(h->s));
        t.plan_bs = 0;
        GORSE_TRY(fm::upload_plan(t.plan, plan, n));
        t.plan_bs = batch_size, t.plan_rows = R;
    }
    GORSE_TRY(h->e_logit.ensure((size_t)n));
    if (h->n_fields > 0) GORSE_TRY(h->rs.ensure(t.plan.max_round, h->d, maxD));
    GORSE_TRY(fm::ensure_events(h->e_ev));

    GORSE_HIP_CHECK(hipEventRecord(h->e_ev[0], h->s));
    if (t.samples) {
        const fm::Catalogue &cat = *h->cat;
        fm::ComposedRows src{};
        src.uptr = t.users.ptr.p, src.uidx = t.users.idx.p, src.uval = t.users.val.p, src.ulead = t.users.lead.p;
        src.iptr = cat.ptr.p, src.iidx = cat.idx.p, src.ival = cat.val.p, src.ilead = cat.lead.p;
        GORSE_TRY(fm::score_rounds(h, t.plan, src, cat.emb, cancel, h->rs, h->e_logit.p));
    } else {
        GORSE_TRY(fm::score_rounds(h, t.plan, fm::PaddedRows{t.idx.p, t.val.p, 0, t.width}, t.emb, cancel, h->rs, h->e_logit.p));
    }
    GORSE_HIP_CHECK(hipEventRecord(h->e_ev[1], h->s));
    GORSE_TRY(fm::enqueue_metrics(h, n_pos, n - n_pos));
    GORSE_HIP_CHECK(hipStreamSynchronize(h->s));
    GORSE_TRY(fm::read_metrics(h, n_pos, n - n_pos, counts, auc_sum));
    if (logits_out) {
        std::vector<float> tmp((size_t)n);
        GORSE_HIP_CHECK(hipMemcpy(tmp.data(), h->e_logit.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
        for (int64_t r = 0; r < n; r++) logits_out[t.order[(size_t)r]] = tmp[(size_t)r];
    }
    h->ev_rows = n, h->ev_slices = t.plan.n_slices, h->ev_rounds = t.plan.rounds();
    return GORSE_OK;
}

extern "C" int32_t gorse_fm_evaluate_stats(gorse_fm *h, int64_t *rows, int64_t *slices, int64_t *rounds, double *device_ms) {
    if (!h) return fail(GORSE_ERR_INVALID, "handle is NULL");
    if (rows) *rows = h->ev_rows;
    if (slices) *slices = h->ev_slices;
    if (rounds) *rounds = h->ev_rounds;
    if (device_ms) *device_ms = h->ev_ms[0];
    return GORSE_OK;
}

extern "C" int32_t gorse_hip_test_fm_evaluate_times(gorse_fm *h, double *ms3) {
    if (!h || !ms3) return fail(GORSE_ERR_INVALID, "handle / ms3 is NULL");
    for (int k = 0; k < 3; k++) ms3[k] = h->ev_ms[k + 1];
    return GORSE_OK;
}

extern "C" int32_t gorse_hip_test_fm_auc(gorse_fm *h, const float *pos, int64_t n_pos, const float *neg, int64_t n_neg,
                                         int64_t *counts, float *auc_sum) {
    if (!h) return fail(GORSE_ERR_INVALID, "handle is NULL");
    if (n_pos < 0 || n_neg < 0 || n_pos + n_neg > INT32_MAX) return fail(GORSE_ERR_INVALID, "between 0 and 2^31 - 1 logits");
    if ((n_pos > 0 && !pos) || (n_neg > 0 && !neg)) return fail(GORSE_ERR_INVALID, "pos / neg is NULL");
    GORSE_HIP_CHECK(hipSetDevice(h->device));
    GORSE_HIP_CHECK(hipStreamSynchronize(h->s));
    GORSE_TRY(h->e_logit.ensure((size_t)(n_pos + n_neg)));
    if (n_pos) GORSE_HIP_CHECK(hipMemcpy(h->e_logit.p, pos, (size_t)n_pos * sizeof(float), hipMemcpyHostToDevice));
    if (n_neg) GORSE_HIP_CHECK(hipMemcpy(h->e_logit.p + n_pos, neg, (size_t)n_neg * sizeof(float), hipMemcpyHostToDevice));
    GORSE_TRY(fm::ensure_events(h->e_ev));
    GORSE_HIP_CHECK(hipEventRecord(h->e_ev[0], h->s));
    GORSE_HIP_CHECK(hipEventRecord(h->e_ev[1], h->s));
    GORSE_TRY(fm::enqueue_metrics(h, n_pos, n_neg));
    GORSE_HIP_CHECK(hipStreamSynchronize(h->s));
    return fm::read_metrics(h, n_pos, n_neg, counts, auc_sum);
}
