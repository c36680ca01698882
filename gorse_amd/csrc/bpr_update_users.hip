// bpr_update_users.hip -- the user-run BPR update on gfx950 (the production Hogwild form for >= 4096 users and nFactors
// 8/16/32/64/128: bpr_plan.hpp bpr_schedule).  Reference: model/cf/model.go:469-488.
//   bpr_update_user_kernel : model.go:469-488 -- one 16-lane group applies ALL samples of one user: p_u is loaded
//                            once, updated in registers and stored once; q_i / q_j are gathered ahead (64-byte
//                            contiguous segments per load) and updated with fp32 atomics (hot items through replica
//                            rows) -- or, the negative of a COLD item, by one write-through store of fma(t, lr, row).
// The folders of the launch are bpr_fold.hpp's (run_folders<true>: they make the last pass themselves, no fold kernel follows); the
// launch's grid, folder count and flags are bpr_plan.hpp's.  The chunk arrives sorted by user from bpr_prepare.hip.
#include "bpr_internal.hpp"

using namespace gorse;

namespace {

// ---- user-run schedule ---------------------------------------------------------------------------
// The chunk's triplets are counting-sorted by USER (the order in which a Hogwild epoch applies its samples is free:
// parallel.go:44-68) and one 16-lane group walks ALL samples of one user: p_u is loaded once, updated in registers
// sample after sample -- exact sequential SGD on the user side, no lost or delayed update -- and stored once, so a
// third of the fp32 atomics (the unit this kernel is bound by: ~1 dword/clk per L2 channel) and a third of the
// gathers disappear.  q_i / q_j are gathered two samples (q_j with the store route: one) ahead of the arithmetic and updated
// with atomics as in bpr_update_kernel (hot items through the replicas).  Users are drawn uniformly (model.go:452-458), so
// the runs are Poisson(N / U)-sized: balanced without any work splitting.
// POSITIVE SERIES.  A series is a maximal stretch of consecutive valid samples of a run with the same positive i (the preparation
// puts a run's repeats of a positive next to each other: bpr_group_positives_kernel; the kernel combines whatever is adjacent).
// Its first sample computes from the gathered snapshot as every sample did before; after each sample the group's own copy of the
// row becomes mad(t1, lr, a), the next sample of the series computes from that copy -- the operands of the sequential code, not a
// snapshot two samples stale -- and its row is not gathered at all; t1 * lr adds up in registers and goes out as ONE atomic per
// element when the series ends: the next positive differs, the next sample is invalid, the run ends, or one of the two samples has
// the series' positive as its NEGATIVE (hand-made streams; i == j included): such a sample's negative-side update then never meets a
// row with a change pending, nothing is lost or counted twice.  A series of one sample issues exactly the atomic of t1 * lr it
// always did.  The sum goes out in the iteration of the series' LAST sample, so no change is pending across iterations outside a
// series, and inside one the previous sample's positive (im1) is the pending row: the own-history rule of the store route holds as
// it stands.  Bound on the delay: a change waits for at most kSeriesFlush = 8 samples of its group (the sum goes out every 8
// samples of a longer series, which keeps walking on its own copy) -- ~28 us at nFactors 64, ~14 us at 16 -- and it is ONE group's
// change to the row, each sample of it computed from a row that holds the group's earlier ones.  The fold-period sweep
// (kDefaultFoldPeriod) diverged when EVERY group's updates of a hot row, ~1800 of them, were computed from one stale row; here
// the other groups' updates keep arriving and only the series' own group reads past them, for the length of the series (<= the
// run; 2 samples on average at C2, ~9 for a user of 19 feedbacks).  tests/test_gpu_bpr_positive_series.py runs 30 epochs at
// nFactors 8 and 16.
// Item classes (hot.slot): >= 0 = the replica rows of a HOT item or the accumulator row of an item of the accumulated tier,
// kWarm = fp32 atomics straight onto the row, kCold = an item whose
// row is touched so rarely (expected touches per `cold window` samples < 1, gorse_mf_create) that the reference's own unlocked
// load / fma / store (model.go:473-488 under parallel.go:44-81) loses next to nothing: its update is ONE write-through store of
// fma(t, lr, row) instead of d atomic dwords.  NEG_STORE opens that route for the NEGATIVE item of a sample; the positive's update is
// always an atomic (by store it cost 0.003-0.005 of NDCG: see kDefaultStoreMode).
constexpr int kCold = -2;  // (-1 = "warm": fp32 atomics straight onto the row)
constexpr int kSeriesFlush = 8;  // samples of a positive series whose summed change goes out together (see POSITIVE SERIES below)
#ifndef GORSE_BPR_SERIES_SKIP_GATHERS
// make ab AB=gathers AB_SRC=bpr_update_users AB_FLAGS=-DGORSE_BPR_SERIES_SKIP_GATHERS=0
#define GORSE_BPR_SERIES_SKIP_GATHERS 1  // A/B: 0 = the positive's row is gathered for every sample, used or not
#endif

// D8: nFactors = 8 (the width of model_test.go:35-48): lanes 0..7 of the group own the eight elements -- the unfused 8-lane tail of
// the AVX512 kernels (floats_avx512.c:350-358, VecShape::unfused) -- and lanes 8..15 mirror them (the reduction needs the products
// replicated there); only lanes 0..7 write.
#ifndef GORSE_BPR_D8_PAIRS
// make ab AB=d8_mirror AB_SRC=bpr_update_users AB_FLAGS=-DGORSE_BPR_D8_PAIRS=0
#define GORSE_BPR_D8_PAIRS 1  // A/B: 0 = nFactors 8 with lanes 8..15 of a group mirroring lanes 0..7 (rounds 4-5)
#endif
template <int NC, bool NEG_STORE, bool D8 = false>
__global__ __launch_bounds__(kBlock) void bpr_update_user_kernel(float *P, float *Q, const int32_t *__restrict__ si,
                                                                 const int32_t *__restrict__ sj,
                                                                 const int32_t *__restrict__ off, int32_t U, int d,
                                                                 float lr, float reg, int exp_mode, double *loss,
                                                                 HotRows hot, int folders, int neg_replicas) {
    if ((int)blockIdx.x < folders) {
        run_folders<true>(hot, Q, folders);
        return;
    }
    // sample (i1, j1) continues the series of the sample (i0, j0) in front of it: the same positive, both samples valid, and neither
    // negative is that positive (hand-made streams: such a sample's negative-side update must meet a row without pending change)
    auto continues = [](int i0, int j0, int i1, int j1) { return i0 == i1 && (i0 | j0 | j1) >= 0 && i0 != j0 && i0 != j1; };
    const int glane = threadIdx.x & (kGroup - 1);
    const int lane = D8 ? (glane & 7) : glane;   // element owned inside a 16-float chunk
    // D8 (round 6): the two halves of a 16-lane group take a user run EACH (eight lanes own a row of eight: until round 5 lanes 8..15
    // mirrored lanes 0..7 and only wrote nothing) -- eight runs per wave instead of four
    constexpr int SUBS = D8 && GORSE_BPR_D8_PAIRS ? 2 : 1;
    const bool writer = !D8 || SUBS == 2 || glane < 8;
    auto mad = [](float x, float y, float z) { return D8 ? x * y + z : fmaf(x, y, z); };
    auto tree8 = [](float v) { return SUBS == 2 ? group_tree8_halves(v) : group_tree8(v); };
    const int gib = threadIdx.x / kGroup;
    const int64_t group = ((int64_t)((int)blockIdx.x - folders) * kGroupsPerBlock + gib) * SUBS + (SUBS == 2 ? glane >> 3 : 0);
    const int64_t ngroups = (int64_t)((int)gridDim.x - folders) * kGroupsPerBlock * SUBS;
    const float nreg = -reg;
    double my_loss = 0.0;
    // which class look-ups this launch needs (every path issues the same loads from a valid address: a look-up nobody needs
    // reads a word that is in cache anyway)
    const bool open = folders > 0;  // the launch has rows that take an item's updates, of either tier (open_hot)
    const bool look_i = open;
    const bool look_j = (open && neg_replicas) || NEG_STORE;
    const int32_t *slot_of = (look_i || look_j) ? hot.slot : si;
    // the items of this group's last two samples: a row one of them wrote is NOT in the snapshot of the current sample (gathered
    // two samples ago), so its update goes through an atomic whatever its class -- a store would overwrite the group's own work
    int im1 = -1, jm1 = -1, im2 = -1, jm2 = -1;
    for (int64_t u = group; u < U; u += ngroups) {
        const int beg = off[u], end = off[u + 1];
        if (beg >= end) continue;
        float *pu = P + u * d;
        // item rows are gathered G = 2 samples ahead of the arithmetic (ra[0] / rb[0]: this sample, ra[k]: sample s + k, the row of sample
        // s + G in flight), their indices IA = 3 ahead and the class of an item G ahead; positions past the run's end re-read the
        // last sample (result unused).  Nothing is used in the iteration that loads it: the counter the waits go by also counts the
        // atomics and returns in order, so a wait for a load issued after them is a wait for their acknowledgement from the memory
        // side.  What a load waits behind is therefore the atomics of min(G, IA - G) iterations ago: with few groups per SIMD
        // (C2: 6040 groups on 1024 SIMDs) that distance IS the time of an iteration.  (Deeper pipelines -- up to rows 6 and ids 9 ahead --
        // and a ring without register rotation were measured and were no faster: profiles/r04_s_probe_bpr_depth.txt.)
        constexpr int G = 2, IA = 3;  // (the own-history rule of the store route looks G = 2 samples back)
        // with the store route open for negatives their rows are gathered ONE sample ahead instead of two: what a store can
        // overwrite is what other groups added between the gather and the store, and that window halves
        constexpr int GB = NEG_STORE ? 1 : G;  // the negative's gather distance
        float p[NC], ra[G][NC], rb[GB][NC];
        const int last = end - 1;
        auto at = [&](int s) { return s <= last ? s : last; };
        auto cl = [](int x) { return x < 0 ? 0 : x; };  // a skipped sample (i = j = -1) gathers row 0, its results are not used
        auto idx_i = [&](int i_, int j_) { return look_i ? cl(i_) : (look_j ? cl(j_) : beg); };
        auto idx_j = [&](int i_, int j_) { return look_j ? cl(j_) : (look_i ? cl(i_) : beg); };
        int ii[IA], jj[IA], sli[G], slj[G];
#pragma unroll
        for (int k = 0; k < IA; k++) ii[k] = si[at(beg + k)], jj[k] = sj[at(beg + k)];
#pragma unroll
        for (int k = 0; k < G; k++) sli[k] = slot_of[idx_i(ii[k], jj[k])], slj[k] = slot_of[idx_j(ii[k], jj[k])];
        // the series in flight: `cur` the positive's row as this group has left it, `acc` its change not yet sent (of `pending`
        // samples), `cont` = the current sample continues the series of the one before
        float cur[NC], acc[NC];
        bool cont = false;
        int pending = 0;
#pragma unroll
        for (int c = 0; c < NC; c++) {
            p[c] = load_row<MODE_ATOMIC>(pu + 16 * c + lane);
#pragma unroll
            for (int k = 0; k < G; k++) ra[k][c] = load_row<MODE_ATOMIC>(Q + (int64_t)cl(ii[k]) * d + 16 * c + lane);
#pragma unroll
            for (int k = 0; k < GB; k++) rb[k][c] = load_row<MODE_ATOMIC>(Q + (int64_t)cl(jj[k]) * d + 16 * c + lane);
        }
        for (int s = beg; s < end; s++) {
            const int in_ = si[at(s + IA)], jn_ = sj[at(s + IA)];
            const int sli_n = slot_of[idx_i(ii[G], jj[G])];
            const int slj_n = slot_of[idx_j(ii[G], jj[G])];
            const int i = ii[0], j = jj[0], slot = sli[0], slotj = slj[0];
            float(&a)[NC] = ra[0];
            float(&b)[NC] = rb[0];
            float ran[NC], rbn[NC];
            // the positive's row of sample s + G: not gathered where that sample will continue a series (it computes from `cur`)
            const bool gather_i = !GORSE_BPR_SERIES_SKIP_GATHERS || !(s + G <= last && continues(ii[G - 1], jj[G - 1], ii[G], jj[G]));
#pragma unroll
            for (int c = 0; c < NC; c++) ran[c] = 0.0f;
            if (gather_i) {
#pragma unroll
                for (int c = 0; c < NC; c++) ran[c] = load_row<MODE_ATOMIC>(Q + (int64_t)cl(ii[G]) * d + 16 * c + lane);
            }
#pragma unroll
            for (int c = 0; c < NC; c++) rbn[c] = load_row<MODE_ATOMIC>(Q + (int64_t)cl(jj[GB]) * d + 16 * c + lane);
            if (cont) {
#pragma unroll
                for (int c = 0; c < NC; c++) a[c] = cur[c];
            }
            const bool more = s < last && continues(i, j, ii[1], jj[1]);  // the next sample continues this one's series
            const bool valid = j >= 0;  // j < 0: the sampler found no negative for this sample (bpr_sample_items_kernel)
            float *qi = Q + (int64_t)cl(i) * d, *qj = Q + (int64_t)cl(j) * d;
            if (open && slot >= 0) qi = hot_row(hot, slot, group);
            if (open && neg_replicas && slotj >= 0) qj = hot_row(hot, slotj, group);
            bool st_j = false;
            if constexpr (NEG_STORE) {
                const bool own_j = i == j || j == im1 || j == jm1 || j == im2 || j == jm2;
                st_j = slotj == kCold && !own_j;
            }
            const float diff = D8 ? tree8(p[0] * a[0]) - tree8(p[0] * b[0]) : dot512_regs<NC>(p, a) - dot512_regs<NC>(p, b);
            const float ex = bpr_exp(-diff, exp_mode);
            const float grad = ex / (1.0f + ex);
            if (loss && (SUBS == 2 ? (glane & 7) == 0 : glane == 0) && valid) my_loss += (double)log1pf(ex);
            float t1[NC], t2[NC];
#pragma unroll
            for (int c = 0; c < NC; c++) {
                t1[c] = mad(a[c], nreg, p[c] * grad);
                t2[c] = mad(b[c], nreg, p[c] * (-grad));
                const float t3 = mad(p[c], nreg, (a[c] - b[c]) * grad);
                p[c] = valid ? mad(t3, lr, p[c]) : p[c];
            }
            if (valid) {  // (every lane keeps the series: the lanes that mirror a row of eight need `cur` as the writers do)
#pragma unroll
                for (int c = 0; c < NC; c++) {
                    acc[c] = pending > 0 ? acc[c] + t1[c] * lr : t1[c] * lr;  // a series of one sends t1 * lr, as the kernel did without series
                    cur[c] = mad(t1[c], lr, a[c]);
                }
                if (!more || ++pending >= kSeriesFlush) {
                    pending = 0;
                    if (writer) {
#pragma unroll
                        for (int c = 0; c < NC; c++)
                            __hip_atomic_fetch_add(qi + 16 * c + lane, acc[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                }
            }
            cont = more;
            if (!valid || !writer) {
            } else if (st_j) {
#pragma unroll
                for (int c = 0; c < NC; c++)
                    __hip_atomic_store(qj + 16 * c + lane, mad(t2[c], lr, b[c]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } else {
#pragma unroll
                for (int c = 0; c < NC; c++)
                    __hip_atomic_fetch_add(qj + 16 * c + lane, t2[c] * lr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
#pragma unroll
            for (int c = 0; c < NC; c++) {
#pragma unroll
                for (int k = 0; k + 1 < G; k++) ra[k][c] = ra[k + 1][c];
                ra[G - 1][c] = ran[c];
#pragma unroll
                for (int k = 0; k + 1 < GB; k++) rb[k][c] = rb[k + 1][c];
                rb[GB - 1][c] = rbn[c];
            }
            im2 = im1, jm2 = jm1, im1 = i, jm1 = j;
#pragma unroll
            for (int k = 0; k + 1 < IA; k++) ii[k] = ii[k + 1], jj[k] = jj[k + 1];
            ii[IA - 1] = in_, jj[IA - 1] = jn_;
#pragma unroll
            for (int k = 0; k + 1 < G; k++) sli[k] = sli[k + 1], slj[k] = slj[k + 1];
            sli[G - 1] = sli_n, slj[G - 1] = slj_n;
        }
        if (writer) {
#pragma unroll
            for (int c = 0; c < NC; c++)  // the only writer of this row in the launch
                __hip_atomic_store(pu + 16 * c + lane, p[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (loss && (SUBS == 2 ? (glane & 7) == 0 : glane == 0) && my_loss != 0.0) atomicAdd(loss, my_loss);
    if (folders > 0) worker_done<true>(hot);
}

}  // namespace

// start / stop (may be null): events bound to the kernel's own dispatch (hipExtLaunchKernelGGL) -- its timestamps and its completion
// signal, no marker packet on the stream (epoch_impl)
int32_t gorse::bpr_launch_update_users(gorse_mf *h, const int32_t *sorted, const int32_t *bucket, size_t cap, float lr, float reg,
                                       int exp_mode, double *loss, hipStream_t st, bool stores, hipEvent_t start, hipEvent_t stop) {
    const int d = h->d;
    int64_t blocks = bpr_user_run_workers(h->U, d, GORSE_BPR_D8_PAIRS);  // nFactors 8: two runs per group
    HotRows hot = make_hot(h);
    const int folders = has_hot(h) ? open_hot(h, hot) : 0;
    blocks += folders;
    const int neg_rep = bpr_neg_replicas(hot.n_hot, hot.n_acc, h->I) ? 1 : 0;
    dim3 grid((unsigned)blocks), block(kBlock);
    const bool neg_store = bpr_neg_store(stores, h->n_cold, g_bpr.store_mode);
    hot.sole = bpr_fold_sole(GORSE_BPR_FOLD_SOLE_WRITER, hot.n_acc, neg_store, h->hot_base.p != nullptr) ? 1 : 0;
    if (folders > 0) h->fold_sole_last = hot.sole;
#define LAUNCH2(NC, NEG_STORE)                                                                                         \
    hipExtLaunchKernelGGL((bpr_update_user_kernel<(NC == 0 ? 1 : NC), NEG_STORE, NC == 0>), grid, block, 0, st, start, stop, 0,     \
                          h->P.p, h->Q.p, sorted + cap, sorted + 2 * cap, bucket, (int32_t)h->U, d, lr, reg, exp_mode, loss, hot, \
                          folders, neg_rep)
#define LAUNCH(NC)                                                                                                     \
    do {                                                                                                               \
        if (neg_store)                                                                                                 \
            LAUNCH2(NC, true);                                                                                         \
        else                                                                                                           \
            LAUNCH2(NC, false);                                                                                        \
    } while (0)
    if (d == 8)
        LAUNCH(0);
    else if (d == 16)
        LAUNCH(1);
    else if (d == 32)
        LAUNCH(2);
    else if (d == 64)
        LAUNCH(4);
    else
        LAUNCH(8);
#undef LAUNCH2
#undef LAUNCH
    GORSE_HIP_CHECK(hipGetLastError());
    return GORSE_OK;
}
