// fm_internal.hpp -- what the factorization machine's sources share.  fm.hip trains and scores batches handed over by the host;
// fm_rank.hip and fm_eval.hip score rows that stay on the device (an item catalogue, a test split) through the one resident
// path of fm_resident.hip.  In here: the handle; the ONE forward kernel (a template over the lane shape, where a row's entries
// come from and what is written) with the helper that picks the lane shape; the attention branch's three forward kernels (a
// template over where a launch's rows come from) with the function that launches them for a field; and the small host helpers
// every entry point uses.  Each is written once, so the scores of all routes agree in every bit by construction.
#pragma once
#include <memory>
#include <type_traits>

#include "common.hpp"
#include "cf_device.hpp"
#include "fm_eval_plan.hpp"

namespace gorse {
namespace fm {
constexpr int kMaxFields = 8;     // embedding fields per model
constexpr int kMaxEmbDim = 4096;  // floats per embedding
constexpr int kGradSegs = 8;      // row segments the branch's parameter gradients are summed in (fixed: the order depends on shapes alone)

// one dense tensor of the embedding branch for the optimizer pass: read from device memory by tensor number
struct DenseDesc {
    float *p, *m, *v;
    const float *g;   // kGradSegs partial sums, gstride apart
    int64_t len, gstride;
};

// One embedding field: H (d x D) | Wa (D x d) | ba (d) | We (D x d) | be (d) in one allocation, every tensor starting at a
// multiple of four floats; the moments lie in the same layout.
struct Field {
    int D = 0;
    size_t off[5] = {0, 0, 0, 0, 0}, len[5] = {0, 0, 0, 0, 0}, total = 0;
    DevBuf<float> p, m, v;
    DevBuf<float> gpart;    // kGradSegs x (dH: d*D | dWa,dba: (D+1)*d | dWe,dbe: (D+1)*d)
    DevBuf<uint16_t> x;     // the training set's embeddings, n x D bf16
    bool have_x = false;
    DevBuf<float> h, a;     // per batch: relu(pre) (rows x d), the softmax output (rows x D; holds s, then e, then a)
    size_t gstride() const { return len[0] + 2 * (len[1] + len[2]); }
};

// The resident item side of gorse_fm_rank_users (gorse_fm_set_items): the items' feature rows as one CSR, each row's number of
// leading entries, and one n_items x D bf16 table per embedding field.  Replaced as a whole.
struct Catalogue {
    int64_t n_items = 0;
    DevBuf<int64_t> ptr;    // n_items + 1
    DevBuf<int32_t> idx, lead;
    DevBuf<float> val;
    DevBuf<uint16_t> emb[kMaxFields];
    // the CSR and the lead array once more on the host (never the embedding tables): a sample-form training set's per-batch
    // plan is built from composed rows (fm_samples_plan.hpp)
    std::vector<int64_t> h_ptr;
    std::vector<int32_t> h_idx, h_lead;
    std::vector<float> h_val;
};

// The user side a sample-form set keeps (gorse_fm_set_train_samples, gorse_fm_set_test_samples): the users' CSR in the form
// gorse_fm_rank_users takes, on the device, and for a training set on the host as well.
struct UserSide {
    int64_t n_users = 0;
    DevBuf<int64_t> ptr;
    DevBuf<int32_t> idx, lead;
    DevBuf<float> val;
};

// A training set in sample form: per sample (user, item, target); sample i is the row gorse_fm_rank_users composes for user[i]
// and catalogue row item[i], and its embedding in field k is row item[i] of the catalogue's table k.  The per-batch plan
// (fm_samples_plan.hpp) belongs to one batch size.
struct SampleSet {
    int64_t n = 0;
    UserSide users;
    std::vector<int64_t> h_uptr;
    std::vector<int32_t> h_uidx, h_ulead, h_user, h_item;
    std::vector<float> h_uval;
    DevBuf<int32_t> user, item;
    DevBuf<float> tgt;
    int32_t plan_bs = 0;
    int64_t max_slots = 0;
    std::vector<int64_t> uoff, eoff;  // n_batches + 1 each: batch k's slots and entries
    DevBuf<int32_t> uniq, seg, row;   // seg: per batch its slots + 1 batch-local entry offsets, at uoff[k] + k
    DevBuf<float> val;
};

// a SlicePlan (fm_eval_plan.hpp) whose per-row descriptors are on the device
struct RoundPlan {
    DevBuf<int32_t> desc;  // segment | item | slice row0 | slice length, n entries each
    std::vector<int64_t> round_begin;
    int64_t n = 0, n_slices = 0, max_round = 0;
    int64_t rounds() const { return (int64_t)round_begin.size() - 1; }
};

// The resident test split of gorse_fm_evaluate (gorse_fm_set_test): the rows in EvaluateClassification's order (the n_pos
// positives first, then the others, each side in dataset order), their padded index / value matrices and one n x D bf16 table per
// field, gathered once.  Replaced as a whole.  The plan belongs to one (batch size, round rows).
struct TestSplit {
    int64_t n = 0, n_pos = 0;
    int width = 0;
    std::vector<int32_t> order;  // resident row -> dataset row
    DevBuf<int32_t> idx;
    DevBuf<float> val;
    DevBuf<uint16_t> emb[kMaxFields];
    // sample form (gorse_fm_set_test_samples): no rows and no embeddings of its own; resident row r is composed from user
    // s_user[r] of `users` and catalogue row s_item[r], whose embeddings are read in place from the catalogue's tables
    bool samples = false;
    UserSide users;
    std::vector<int32_t> s_user, s_item;
    int32_t plan_bs = 0;
    int64_t plan_rows = 0;
    RoundPlan plan;
};

// What one launch round of score_rounds works in (the model has fields): vx and h (rows x d), s (rows x maxD), the Softmax's
// maxima and sums.  One instance per handle: gorse_fm_rank_users and gorse_fm_evaluate run on the handle's one stream and
// drain it before they return, and every round writes each of these before it reads it.
struct RoundScratch {
    DevBuf<float> vx, h, s, rmax, rsum;
    int32_t ensure(int64_t rows, int d, int maxD) {
        GORSE_TRY(vx.ensure((size_t)rows * d));
        GORSE_TRY(h.ensure((size_t)rows * d));
        GORSE_TRY(s.ensure((size_t)rows * maxD));
        GORSE_TRY(rmax.ensure((size_t)rows));
        return rsum.ensure((size_t)rows);
    }
};
}  // namespace fm
}  // namespace gorse

struct gorse_fm {
    int device = 0;
    int64_t nf = 0;
    int d = 0;
    hipStream_t s = nullptr;
    gorse::DevBuf<float> V, W, B, mV, mW, mB, vV, vW, vB;  // parameters and Adam moments, one allocation per tensor
    gorse::DevBuf<int64_t> tag;                            // per feature row: ((step + 1) << 32) | slot of the step that touched it
    int64_t step = 0;                                      // training steps this handle has run (the tags' clock)
    int64_t adam_t = 0;                                    // nn.Adam's t: reset by set_params (a new Fit)
    // training set
    int64_t n = 0;
    int width = 0;
    std::vector<int32_t> h_idx;
    std::vector<float> h_val;
    gorse::DevBuf<int32_t> idx;
    gorse::DevBuf<float> val, tgt;
    // per-batch-size plan: for every batch the features it touches (ascending) and each one's positions (ascending)
    int plan_bs = 0;
    std::vector<int64_t> uoff;  // n_batches + 1: slots of batch k = [uoff[k], uoff[k+1])
    int64_t max_slots = 0;
    gorse::DevBuf<int32_t> uniq, seg, pos;
    // the training set in sample form (fm_samples.hip): set means it is what gorse_fm_epoch trains, and n above is its rows
    std::unique_ptr<gorse::fm::SampleSet> smp;
    bool smp_dropped = false, test_dropped = false;  // a sample-form set went away with the catalogue it indexed
    // scratch
    gorse::DevBuf<float> gs, loss, vx, gV, gW, gB, cost;
    gorse::DevBuf<int32_t> p_idx;
    gorse::DevBuf<float> p_val, p_out;
    hipEvent_t ev[2] = {nullptr, nullptr};
    // the item-embedding branch (fm.go:127-132): empty unless gorse_fm_set_embedding_dims configured fields
    int n_fields = 0;
    gorse::fm::Field fld[gorse::fm::kMaxFields];
    gorse::DevBuf<gorse::fm::DenseDesc> descs;
    int64_t dense_blocks = 0;  // blocks of the longest dense tensor
    gorse::DevBuf<float> a_rmax, a_rsum, a_sumdx, a_gx, a_dpre, a_esum, a_vxe, a_logit;
    gorse::DevBuf<uint16_t> p_x;
    gorse::DevBuf<float> p_vx;
    // scoring resident rows (fm_resident.hip): the round scratch both calls below work in.  Nothing from here on is read or
    // written by training or by gorse_fm_predict*, and the two calls touch none of the buffers above but the parameters.
    gorse::fm::RoundScratch rs;
    // ranking from a resident catalogue (fm_rank.hip)
    std::unique_ptr<gorse::fm::Catalogue> cat;
    gorse::DevBuf<int64_t> r_uptr, r_cptr;  // the call's user CSR pointer and candidate pointer
    gorse::DevBuf<int32_t> r_uidx, r_ulead;
    gorse::DevBuf<float> r_uval, r_scores;
    gorse::fm::RoundPlan r_plan;            // the call's slices: segment = user, item = candidate
    gorse::DevBuf<int32_t> r_order;
    gorse::DevBuf<double> r_final;            // gorse_fm_rank_cand_decayed: the decayed scores
    hipEvent_t r_ev[2] = {nullptr, nullptr};  // timing events of gorse_fm_rank_stats, created by the first rank call
    int64_t rk_rows = 0, rk_slices = 0, rk_rounds = 0, rk_host_sorted = 0;
    double rk_ms = 0.0;
    // evaluation from a resident test split (fm_eval.hip)
    std::unique_ptr<gorse::fm::TestSplit> test;
    gorse::DevBuf<float> e_logit;
    gorse::DevBuf<uint32_t> e_key[2], e_hist, e_cnt;  // the sort's two key arrays, its tile x digit counts, negatives below each positive
    gorse::DevBuf<uint64_t> e_acc;                    // the tallies, pairs_less and (as bits) auc_sum
    hipEvent_t e_ev[4] = {nullptr, nullptr, nullptr, nullptr};  // start | scored | sorted and counted | chain done
    int64_t ev_rows = 0, ev_slices = 0, ev_rounds = 0;
    double ev_ms[4] = {0.0, 0.0, 0.0, 0.0};  // all | scoring | keys, sort, count | chain
};

namespace gorse {
namespace fm {

constexpr int kBlock = 256;
constexpr int kMaxFactors = 128;

// lanes per sample: the smallest of 8 / 16 / 32 / 64 that holds d (two factors per lane above 64)
inline int lanes_for(int d) {
    int g = 8;
    while (g < d && g < 64) g *= 2;
    return g;
}

// fn(G, NF) with d's lane shape as compile-time constants (std::integral_constant): the one statement of that mapping
template <class F>
inline void with_lanes(int d, F &&fn) {
    using std::integral_constant;
    const int G = lanes_for(d);
    switch (G) {
        case 8: fn(integral_constant<int, 8>{}, integral_constant<int, 1>{}); break;
        case 16: fn(integral_constant<int, 16>{}, integral_constant<int, 1>{}); break;
        case 32: fn(integral_constant<int, 32>{}, integral_constant<int, 1>{}); break;
        default:
            if (d > 64) fn(integral_constant<int, 64>{}, integral_constant<int, 2>{});
            else fn(integral_constant<int, 64>{}, integral_constant<int, 1>{});
    }
}

inline unsigned row_grid(int64_t nrows) { return (unsigned)ceil_div(nrows, kBlock / 64); }

// sum over each aligned group of G lanes; the group's first lane holds the total (a fixed tree: deterministic)
template <int G>
__device__ __forceinline__ float group_sum(float v) {
    if constexpr (G == 8) {
        v = group_tree8_halves(v);
    } else {
        v = group_tree16(v);
        if constexpr (G >= 32) v = v + __shfl_xor(v, 16, 64);
        if constexpr (G == 64) v = v + __shfl_xor(v, 32, 64);
    }
    return v;
}

// One nonzero entry (feature id, value x) of a row joins the lane's chains: vx_f += V[id, f] x, sq_f += V[id, f]^2 x^2 for the
// lane's factors f = lane + k G, and lin += W[id] x.  The one statement of the forward pass's arithmetic.
template <int G, int NF>
__device__ __forceinline__ void fm_entry(const float *V, const float *W, int d, int lane, int64_t id, float x, float (&vx)[NF],
                                         float (&sq)[NF], float &lin) {
    const float *vr = V + id * d;
    const float x2 = x * x;
#pragma unroll
    for (int k = 0; k < NF; k++) {
        const int f = lane + k * G;
        if (f < d) {
            const float v = vr[f];
            vx[k] = fmaf(v, x, vx[k]);
            sq[k] = fmaf(v * v, x2, sq[k]);
        }
    }
    lin = fmaf(W[id], x, lin);
}

// the row's logit from its chains (valid in the group's first lane)
template <int G, int NF>
__device__ __forceinline__ float fm_logit(const float (&vx)[NF], const float (&sq)[NF], float lin, const float *B) {
    float part = 0.0f;
#pragma unroll
    for (int k = 0; k < NF; k++) part += vx[k] * vx[k] - sq[k];
    part = group_sum<G>(part);
    return (lin + 0.5f * part) + B[0];
}

// ---- the forward kernel ---------------------------------------------------------------------------------------------------
// Where a row's entries come from.  Both sources hand the nonzero entries to fm_entry one after the other; zero values (the
// padding: index 0, value 0) are skipped, they would add only signed zeros.  round() points a source at the launch round that
// begins at row r0 of a plan's per-row segment and item descriptors.

// row0 + b of a padded n x width index / value matrix (training, gorse_fm_predict*, the resident test split)
struct PaddedRows {
    const int32_t *idx;
    const float *val;
    int64_t row0;
    int width;
    void round(const int32_t *, const int32_t *, int64_t r0) { row0 = r0; }
    template <int G, int NF>
    __device__ __forceinline__ void walk(int64_t b, const float *V, const float *W, int d, int lane, float (&vx)[NF],
                                         float (&sq)[NF], float &lin) const {
        const int64_t r = row0 + b;
        const int32_t *ri = idx + r * width;
        const float *rv = val + r * width;
        for (int j = 0; j < width; j++) {
            const float x = rv[j];
            if (x == 0.0f) continue;
            fm_entry<G, NF>(V, W, d, lane, ri[j], x, vx, sq, lin);
        }
    }
};

__device__ __forceinline__ int64_t first_lane64(int64_t v) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// The row gorse_fm_rank_users composes in BatchPredict's order (fm.go:183-206): user lead | item lead | user rest | item rest,
// through the row's (user, item) descriptor into the call's user CSR and the resident catalogue.
struct ComposedRows {
    const int64_t *uptr;  // the call's users: CSR pointer, entries, leading entries per user
    const int32_t *uidx;
    const float *uval;
    const int32_t *ulead;
    const int64_t *iptr;  // the catalogue
    const int32_t *iidx;
    const float *ival;
    const int32_t *ilead;
    const int32_t *user, *item;  // per row of the round
    void round(const int32_t *seg, const int32_t *it, int64_t r0) { user = seg + r0, item = it + r0; }
    // entries [j0, j1) of a CSR in order.  UNIFORM: the range is the same in every lane of the wave (the caller checked), so
    // index and value come through scalar loads.
    template <int G, int NF, bool UNIFORM>
    __device__ __forceinline__ static void span(const int32_t *idx, const float *val, int64_t j0, int64_t j1, const float *V,
                                                const float *W, int d, int lane, float (&vx)[NF], float (&sq)[NF], float &lin) {
        if (UNIFORM) {
            j0 = first_lane64(j0);
            j1 = first_lane64(j1);
        }
        for (int64_t j = j0; j < j1; j++) {
            const float x = val[j];
            if (x == 0.0f) continue;
            fm_entry<G, NF>(V, W, d, lane, idx[j], x, vx, sq, lin);
        }
    }
    template <int G, int NF>
    __device__ __forceinline__ void walk(int64_t b, const float *V, const float *W, int d, int lane, float (&vx)[NF],
                                         float (&sq)[NF], float &lin) const {
        const int32_t u = user[b], c = item[b];
        const int64_t u0 = uptr[u], u1 = uptr[u + 1], um = u0 + ulead[u];
        const int64_t i0 = iptr[c], i1 = iptr[c + 1], im = i0 + ilead[c];
        // a user's rows are consecutive: most waves hold one user only
        const bool one_user = __all(u == __builtin_amdgcn_readfirstlane(u));
        if (one_user)
            span<G, NF, true>(uidx, uval, u0, um, V, W, d, lane, vx, sq, lin);
        else
            span<G, NF, false>(uidx, uval, u0, um, V, W, d, lane, vx, sq, lin);
        span<G, NF, false>(iidx, ival, i0, im, V, W, d, lane, vx, sq, lin);
        if (one_user)
            span<G, NF, true>(uidx, uval, um, u1, V, W, d, lane, vx, sq, lin);
        else
            span<G, NF, false>(uidx, uval, um, u1, V, W, d, lane, vx, sq, lin);
        span<G, NF, false>(iidx, ival, im, i1, V, W, d, lane, vx, sq, lin);
    }
};

// what a forward launch writes: the logit; the logit and vx (scoring a model with fields); or what a training step needs
enum { kLogit = 0, kLogitVx = 1, kTrain = 2 };

template <class Src>
struct FwdArgs {
    Src src;
    const float *V, *W, *B;
    int64_t nrows;
    int d;
    float *out;          // nrows logits (kTrain: NULL, or where the embedding branch wants the FM's logit)
    float *vx;           // nrows x d: vx_f = sum_j V[idx_j, f] x_j (kLogitVx, kTrain)
    const float *tgt;    // kTrain: the launch's rows' targets
    float inv_n;         // kTrain: 1 / rows of the batch
    float *gs, *loss;    // kTrain: per sample g_b and loss_b
};

// one sample per G-lane group: the row's chains, the DPP-reduced pairwise term, the logit in the group's first lane
template <int G, int NF, class Src, int OUT>
__global__ __launch_bounds__(kBlock) void fm_forward_kernel(FwdArgs<Src> a) {
    const int lane = threadIdx.x & (G - 1);
    const int64_t b = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / G;
    if (b >= a.nrows) return;  // whole groups leave together
    float vx[NF], sq[NF];
#pragma unroll
    for (int k = 0; k < NF; k++) vx[k] = sq[k] = 0.0f;
    float lin = 0.0f;
    a.src.template walk<G, NF>(b, a.V, a.W, a.d, lane, vx, sq, lin);
    const float logit = fm_logit<G, NF>(vx, sq, lin, a.B);
    if (OUT != kLogit) {
#pragma unroll
        for (int k = 0; k < NF; k++) {
            const int f = lane + k * G;
            if (f < a.d) a.vx[b * a.d + f] = vx[k];
        }
    }
    if (lane != 0) return;
    if (OUT != kTrain) {
        a.out[b] = logit;
        return;
    }
    // BCEWithLogits (common/nn/functions.go:218-243) with y = (t + 1) / 2
    const float y = (a.tgt[b] + 1.0f) * 0.5f;
    a.loss[b] = fmaxf(logit, 0.0f) - logit * y + logf(1.0f + expf(-fabsf(logit)));
    a.gs[b] = (1.0f / (1.0f + expf(-logit)) - y) * a.inv_n;
    if (a.out) a.out[b] = logit;  // with embedding fields att_loss_kernel forms loss and g again from the full logit
}

template <int OUT, class Src>
inline int32_t launch_forward(hipStream_t s, const FwdArgs<Src> &a) {
    const int64_t grid = ceil_div(a.nrows * lanes_for(a.d), kBlock);
    if (grid == 0) return GORSE_OK;
    with_lanes(a.d, [&](auto G, auto NF) {
        fm_forward_kernel<decltype(G)::value, decltype(NF)::value, Src, OUT><<<dim3((unsigned)grid), dim3(kBlock), 0, s>>>(a);
    });
    GORSE_HIP_CHECK(hipGetLastError());
    return GORSE_OK;
}

// ---- the item-embedding branch: forward kernels ----------------------------------------------------------------------------

constexpr int kFC = 16;  // factors per accumulator chunk

struct AttArgs {
    const uint16_t *x;  // the batch rows' embeddings, nrows x D bf16 (SliceRows: the field's resident table)
    const float *H, *Wa, *ba, *We, *be;
    int64_t nrows;
    int D, d;
    float *h;           // nrows x d
    float *s;           // nrows x D: s (att_score), e (att_exp), a (att_enc)
    float *rmax, *rsum; // nrows
    const float *vx;    // nrows x d
    float *logit;       // nrows: the field's contribution is added
    float *esum;        // nrows x d: sum of the fields' enc (training), or NULL
    int first;          // field 0 writes esum, later fields add
    // backward
    const float *gs;    // nrows: the loss gradient of the rows' logits
    float *gx;          // nrows x D: a * da, then ds
    float *sumdx;       // nrows
    float *dpre;        // nrows x d
    float *gpart;       // kGradSegs x Field::gstride()
    int64_t gstride;
};

// Where a launch's rows come from.  BatchRows: the launch is one batch, row r's embedding is row r of x, and the Softmax's
// maxima and sums are indexed over the whole launch.  SliceRows (a launch round of score_rounds): the launch holds many
// slices, each a batch of its own; row r's embedding is row item[r] of the field's resident table, read in place, and r
// carries its slice's first row and length.
struct BatchRows {
    __device__ __forceinline__ const uint16_t *x(const AttArgs &a, int64_t r) const { return a.x + r * a.D; }
    // n = the slice's rows, base = its first row, returns (local row x D) % n
    __device__ __forceinline__ uint32_t wrap(const AttArgs &a, int64_t r, uint32_t &n, int64_t &base) const {
        n = (uint32_t)a.nrows;
        base = 0;
        return (uint32_t)((r * a.D) % a.nrows);
    }
    __device__ __forceinline__ const uint16_t *xu(const AttArgs &a, int64_t r) const { return x(a, r); }
};
struct SliceRows {
    const int32_t *item, *row0, *len;  // per row of the launch
    __device__ __forceinline__ const uint16_t *x(const AttArgs &a, int64_t r) const { return a.x + (int64_t)item[r] * a.D; }
    __device__ __forceinline__ uint32_t wrap(const AttArgs &a, int64_t r, uint32_t &n, int64_t &base) const {
        const int64_t sn = len[r];
        n = (uint32_t)sn;
        base = row0[r];
        return (uint32_t)(((r - base) * a.D) % sn);
    }
};

// A batch of a sample-form training set: one batch as BatchRows has it (the Softmax indexes over the whole launch), but row r's
// embedding is row item[r] of the field's resident table, read in place.  xu: r is the same in every lane of the wave, so
// item[r] comes through a scalar load.
struct ItemRows {
    const int32_t *item;  // per row of the batch
    __device__ __forceinline__ const uint16_t *x(const AttArgs &a, int64_t r) const { return a.x + (int64_t)item[r] * a.D; }
    __device__ __forceinline__ const uint16_t *xu(const AttArgs &a, int64_t r) const {
        return a.x + (int64_t)__builtin_amdgcn_readfirstlane(item[r]) * a.D;
    }
    __device__ __forceinline__ uint32_t wrap(const AttArgs &a, int64_t r, uint32_t &n, int64_t &base) const {
        return BatchRows{}.wrap(a, r, n, base);
    }
};

__device__ __forceinline__ float bf16_f32(uint16_t u) { return __uint_as_float((uint32_t)u << 16); }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// w[k] = M[c, f0 + k] of a row-major (D x d) matrix, zero past d; 16-byte loads where d is a multiple of four
__device__ __forceinline__ void load_w16(const float *M, int64_t c, int d, int f0, bool vec, float (&w)[kFC]) {
    const float *p = M + c * d + f0;
    if (vec) {
#pragma unroll
        for (int j = 0; j < kFC / 4; j++) {
            float4 t = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (f0 + 4 * j < d) t = *reinterpret_cast<const float4 *>(p + 4 * j);
            w[4 * j] = t.x, w[4 * j + 1] = t.y, w[4 * j + 2] = t.z, w[4 * j + 3] = t.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < kFC; k++) w[k] = f0 + k < d ? p[k] : 0.0f;
    }
}

// the wave's total of every acc[k]; lane k keeps total k (selected without indexing the array by a register)
__device__ __forceinline__ float reduce_pick(float (&acc)[kFC], int lane) {
    float mine = 0.0f;
#pragma unroll
    for (int k = 0; k < kFC; k++) {
        const float t = wave_sum(acc[k]);
        if (lane == k) mine = t;
    }
    return mine;
}

// pre, h = relu(pre), s = h H and each row's maximum of s
template <class Rows>
__global__ __launch_bounds__(kBlock) void att_score_kernel(AttArgs a, Rows rows) {
    __shared__ float sh[kBlock / 64][kMaxFactors];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t r = (int64_t)blockIdx.x * (kBlock / 64) + w;
    const bool live = r < a.nrows;
    const bool vec = (a.d & 3) == 0;
    if (live) {
        const uint16_t *xr = rows.x(a, r);
        for (int f0 = 0; f0 < a.d; f0 += kFC) {
            float acc[kFC];
#pragma unroll
            for (int k = 0; k < kFC; k++) acc[k] = 0.0f;
            for (int c = lane; c < a.D; c += 64) {
                const float xv = bf16_f32(xr[c]);
                float wv[kFC];
                load_w16(a.Wa, c, a.d, f0, vec, wv);
#pragma unroll
                for (int k = 0; k < kFC; k++) acc[k] = fmaf(xv, wv[k], acc[k]);
            }
            const float mine = reduce_pick(acc, lane);
            if (lane < kFC && f0 + lane < a.d) {
                const float hv = fmaxf(mine + a.ba[f0 + lane], 0.0f);
                sh[w][f0 + lane] = hv;
                a.h[r * a.d + f0 + lane] = hv;
            }
        }
    }
    __syncthreads();
    if (!live) return;
    float *sr = a.s + r * a.D;
    float mx = -INFINITY;
    for (int c = lane; c < a.D; c += 64) {
        float acc = 0.0f;
        for (int f = 0; f < a.d; f++) acc = fmaf(sh[w][f], a.H[(int64_t)f * a.D + c], acc);  // floats.MM's chain over f
        sr[c] = acc;
        mx = fmaxf(mx, acc);
    }
    mx = wave_max(mx);
    if (lane == 0) a.rmax[r] = mx;
}

// e = exp(s - max[(r D + c) % n]) through fp64 (float32(math.Exp(float64(.))), tensor.go:414-419) and each row's sum of e
template <class Rows>
__global__ __launch_bounds__(kBlock) void att_exp_kernel(AttArgs a, Rows rows) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (r >= a.nrows) return;
    uint32_t n;
    int64_t base;
    const uint32_t m0 = rows.wrap(a, r, n, base);
    const float *rmax = a.rmax + base;
    float *sr = a.s + r * a.D;
    float sum = 0.0f;
    for (int c = lane; c < a.D; c += 64) {
        const uint32_t m = (m0 + (uint32_t)c) % n;
        const float e = (float)exp((double)(sr[c] - rmax[m]));
        sr[c] = e;
        sum += e;
    }
    sum = wave_sum(sum);
    if (lane == 0) a.rsum[r] = sum;
}

// a = e / sum[(r D + c) % n], z = a * x, enc = z We + be, logit += sum_f vx_f enc_f
template <class Rows>
__global__ __launch_bounds__(kBlock) void att_enc_kernel(AttArgs a, Rows rows) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (r >= a.nrows) return;
    const bool vec = (a.d & 3) == 0;
    uint32_t n;
    int64_t base;
    const uint32_t m0 = rows.wrap(a, r, n, base);
    const float *rsum = a.rsum + base;
    const uint16_t *xr = rows.x(a, r);
    float *sr = a.s + r * a.D;
    float contrib = 0.0f;
    for (int f0 = 0; f0 < a.d; f0 += kFC) {
        float acc[kFC];
#pragma unroll
        for (int k = 0; k < kFC; k++) acc[k] = 0.0f;
        for (int c = lane; c < a.D; c += 64) {
            float av = sr[c];
            if (f0 == 0) {  // the first chunk turns e into a in place (this lane owns the element in every chunk)
                av = av / rsum[(m0 + (uint32_t)c) % n];
                sr[c] = av;
            }
            const float zv = av * bf16_f32(xr[c]);
            float wv[kFC];
            load_w16(a.We, c, a.d, f0, vec, wv);
#pragma unroll
            for (int k = 0; k < kFC; k++) acc[k] = fmaf(zv, wv[k], acc[k]);
        }
        const float mine = reduce_pick(acc, lane);
        float part = 0.0f;
        if (lane < kFC && f0 + lane < a.d) {
            const int64_t o = r * a.d + f0 + lane;
            const float enc = mine + a.be[f0 + lane];
            if (a.esum) a.esum[o] = a.first ? enc : a.esum[o] + enc;
            part = a.vx[o] * enc;
        }
        contrib += wave_sum(part);
    }
    if (lane == 0) a.logit[r] = a.logit[r] + contrib;
}

// ---- host side ----------------------------------------------------------------------------------------------------------------

// field k's parameters and shape; the caller adds the rows and the buffers
inline AttArgs field_args(const gorse_fm *h, int k) {
    const Field &F = h->fld[k];
    AttArgs a{};
    a.H = F.p.p + F.off[0], a.Wa = F.p.p + F.off[1], a.ba = F.p.p + F.off[2], a.We = F.p.p + F.off[3], a.be = F.p.p + F.off[4];
    a.D = F.D, a.d = h->d;
    return a;
}

// the three forward launches of one field on the launch's rows
template <class Rows>
inline int32_t branch_forward(hipStream_t s, const AttArgs &a, const Rows &rows) {
    const unsigned grid = row_grid(a.nrows);
    att_score_kernel<<<dim3(grid), dim3(kBlock), 0, s>>>(a, rows);
    att_exp_kernel<<<dim3(grid), dim3(kBlock), 0, s>>>(a, rows);
    att_enc_kernel<<<dim3(grid), dim3(kBlock), 0, s>>>(a, rows);
    GORSE_HIP_CHECK(hipGetLastError());
    return GORSE_OK;
}

inline int max_emb_dim(const gorse_fm *h) {
    int maxD = 0;
    for (int k = 0; k < h->n_fields; k++) maxD = std::max(maxD, h->fld[k].D);
    return maxD;
}

// one table per field, where the model has fields
inline int32_t check_emb(const gorse_fm *h, const uint16_t *const *emb) {
    if (h->n_fields == 0) return GORSE_OK;
    if (!emb) return fail(GORSE_ERR_INVALID, "emb is NULL");
    for (int k = 0; k < h->n_fields; k++)
        if (!emb[k]) return fail(GORSE_ERR_INVALID, "emb[%d] is NULL", k);
    return GORSE_OK;
}

// what is to become resident is refused before anything is allocated where it is larger than the device's memory
inline int32_t check_fits(double bytes, const char *what) {
    size_t mem_free = 0, mem_total = 0;
    GORSE_HIP_CHECK(hipMemGetInfo(&mem_free, &mem_total));
    if (bytes > (double)mem_total) return fail(GORSE_ERR_NOMEM, "a %s of %.3g bytes does not fit the device's %zu", what, bytes, mem_total);
    return GORSE_OK;
}

template <typename T>
inline int32_t upload(DevBuf<T> &dst, const T *src, size_t n) {
    GORSE_TRY(dst.ensure(n));
    if (n) GORSE_HIP_CHECK(hipMemcpy(dst.p, src, n * sizeof(T), hipMemcpyHostToDevice));
    return GORSE_OK;
}

inline int32_t upload_plan(RoundPlan &dst, SlicePlan &src, int64_t n) {
    GORSE_TRY(upload(dst.desc, src.desc.data(), src.desc.size()));
    dst.round_begin = std::move(src.round_begin);
    dst.n = n, dst.n_slices = src.n_slices, dst.max_round = src.max_round;
    return GORSE_OK;
}

// a sample-form training set or test split goes away with the catalogue it indexes (gorse_fm_set_items,
// gorse_fm_set_embedding_dims); the flags let gorse_fm_epoch / gorse_fm_evaluate say why there is none
inline void drop_sample_sets(gorse_fm *h) {
    if (h->smp) {
        h->smp.reset();
        h->n = 0;
        h->smp_dropped = true;
    }
    if (h->test && h->test->samples) {
        h->test.reset();
        h->test_dropped = true;
    }
}

// timing events created by the first call that records them
template <size_t N>
inline int32_t ensure_events(hipEvent_t (&ev)[N]) {
    for (auto &e : ev)
        if (!e) GORSE_HIP_CHECK(hipEventCreate(&e));
    return GORSE_OK;
}

// fm_rank.hip: the feature rows of one side: a well-formed pointer, entries in range, lead[i] within row i
int32_t check_side(const gorse_fm *h, int64_t n, const int64_t *ptr, const int32_t *idx, const float *val, const int32_t *lead,
                   const char *what);

// fm_resident.hip: the rows of every round of `plan` scored into logit (plan.n entries): src's entries through the forward
// kernel and, where the model has fields, the branch on the rows' embeddings in tables[field] (row plan item[r]), in `rs`
// (ensured by the caller for plan.max_round rows).  Enqueued on the handle's stream; the cancel flag is read before every round
// and once after the last.
template <class Src>
int32_t score_rounds(gorse_fm *h, const RoundPlan &plan, Src src, const DevBuf<uint16_t> *tables, const volatile int32_t *cancel,
                     RoundScratch &rs, float *logit);

}  // namespace fm
}  // namespace gorse
