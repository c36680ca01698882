// fm_train.hpp -- what the two training routes share beyond the forward kernels of fm_internal.hpp.  gorse_fm_epoch (fm.hip)
// runs ONE loop over a TrainSource: the padded rows of gorse_fm_set_train (fm.hip) or the (user, item) samples of
// gorse_fm_set_train_samples (fm_samples.hip).  A source launches the kernels that read its rows; their arithmetic is written
// once, here, as __device__ templates over where a row's embedding (Rows) or a feature's entries (Entries) come from, and each
// source file wraps them in kernels of its own, so both routes produce the same bits by construction.
#pragma once
#include "fm_internal.hpp"

namespace gorse {
namespace fm {

struct AccArgs {
    const int32_t *uniq, *seg, *pos;  // the batch's slots: uniq[s] = feature, positions pos[seg[s] .. seg[s+1])
    int64_t slot0, nslots;
    const float *val;  // batch rows' values (row0 * width applied)
    const float *V;
    const float *gs, *loss, *vx;
    int64_t nrows;
    int width, d;
    int64_t tag_hi;  // (step + 1) << 32
    int64_t *tag;
    float *gV, *gW, *gB, *cost;
};

// Where entry q of a feature's list comes from: (batch-local row, value), or (0, 0) past the list's end.
// PaddedEntries: a position p of the batch's padded value matrix, row p / width.
struct PaddedEntries {
    const int32_t *pos;
    const float *val;
    int width;
    __device__ __forceinline__ void get(int q, bool live, int64_t &b, float &x) const {
        const int p = live ? pos[q] : 0;
        b = p / width;
        x = live ? val[p] : 0.0f;
    }
};
// SampleEntries: the plan carries the row and the value themselves (there is no padded matrix to index)
struct SampleEntries {
    const int32_t *row;
    const float *val;
    __device__ __forceinline__ void get(int q, bool live, int64_t &b, float &x) const {
        b = live ? row[q] : 0;
        x = live ? val[q] : 0.0f;
    }
};

// One wave per touched feature.  The wave's 64 / G groups take every (64 / G)-th entry of the feature's list in order, each
// group's lanes hold the row's factors; the groups' partial sums are then added in a fixed butterfly.  The last block instead
// sums dB and the batch's loss over the samples (one thread per stride, then an LDS tree) and adds the mean to the epoch's cost.
template <int G, int NF, class Entries>
__device__ __forceinline__ void fm_accum_body(const AccArgs &a, const Entries &ent) {
    if (blockIdx.x == gridDim.x - 1) {
        __shared__ float sg[kBlock], sl[kBlock];
        float g = 0.0f, l = 0.0f;
        for (int64_t b = threadIdx.x; b < a.nrows; b += kBlock) {
            g += a.gs[b];
            l += a.loss[b];
        }
        sg[threadIdx.x] = g;
        sl[threadIdx.x] = l;
        __syncthreads();
        for (int o = kBlock / 2; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) {
                sg[threadIdx.x] += sg[threadIdx.x + o];
                sl[threadIdx.x] += sl[threadIdx.x + o];
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            a.gB[0] = sg[0];
            a.cost[0] = a.cost[0] + sl[0] / (float)a.nrows;
        }
        return;
    }
    constexpr int NG = 64 / G;
    const int64_t s = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / 64;
    if (s >= a.nslots) return;
    const int lane = threadIdx.x & (G - 1);
    const int grp = (threadIdx.x & 63) / G;
    const int64_t gslot = a.slot0 + s;
    const int32_t feat = a.uniq[gslot];
    const int32_t beg = a.seg[gslot], end = a.seg[gslot + 1];
    float vr[NF], acc[NF];
#pragma unroll
    for (int k = 0; k < NF; k++) {
        const int f = lane + k * G;
        vr[k] = f < a.d ? a.V[(int64_t)feat * a.d + f] : 0.0f;
        acc[k] = 0.0f;
    }
    float accw = 0.0f;
    constexpr int U = 4;  // entries whose loads are issued together; the sum still runs in list order
    for (int q0 = beg + grp; q0 < end; q0 += U * NG) {
        float gx[U], xx[U], x2[U];
        int64_t bb[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int q = q0 + u * NG;
            int64_t b;
            float x;
            ent.get(q, q < end, b, x);
            const float g = q < end ? a.gs[b] : 0.0f;
            bb[u] = b;
            xx[u] = x;
            gx[u] = g;
            x2[u] = x * x;
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            if (q0 + u * NG >= end) break;
            accw += gx[u] * xx[u];
#pragma unroll
            for (int k = 0; k < NF; k++) {
                const int f = lane + k * G;
                if (f < a.d) {
                    const float t = xx[u] * a.vx[bb[u] * a.d + f] - vr[k] * x2[u];
                    acc[k] += gx[u] * t;
                }
            }
        }
    }
#pragma unroll
    for (int o = G; o < 64; o <<= 1) {
#pragma unroll
        for (int k = 0; k < NF; k++) acc[k] = acc[k] + __shfl_xor(acc[k], o, 64);
        accw = accw + __shfl_xor(accw, o, 64);
    }
    if (grp != 0) return;
#pragma unroll
    for (int k = 0; k < NF; k++) {
        const int f = lane + k * G;
        if (f < a.d) a.gV[s * a.d + f] = acc[k];
    }
    if (lane == 0) {
        a.gW[s] = accw;
        a.tag[feat] = a.tag_hi | s;
    }
}

// denc = g vx, dz = denc We^T, da = dz * x, gx = a * da and each row's sum of gx
template <class Rows>
__device__ __forceinline__ void att_bwd_gx_body(const AttArgs &a, const Rows &rows) {
    __shared__ float sh[kBlock / 64][kMaxFactors];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t r = (int64_t)blockIdx.x * (kBlock / 64) + w;
    const bool live = r < a.nrows;
    for (int f = lane; f < kMaxFactors; f += 64) sh[w][f] = live && f < a.d ? a.gs[r] * a.vx[r * a.d + f] : 0.0f;
    __syncthreads();
    if (!live) return;
    const bool vec = (a.d & 3) == 0;
    const uint16_t *xr = rows.x(a, r);
    const float *ar = a.s + r * a.D;
    float *gr = a.gx + r * a.D;
    float sum = 0.0f;
    for (int c = lane; c < a.D; c += 64) {
        float dz = 0.0f;
        for (int f0 = 0; f0 < a.d; f0 += kFC) {
            float wv[kFC];
            load_w16(a.We, c, a.d, f0, vec, wv);
#pragma unroll
            for (int k = 0; k < kFC; k++) dz = fmaf(sh[w][f0 + k], wv[k], dz);
        }
        const float g = ar[c] * (dz * bf16_f32(xr[c]));
        gr[c] = g;
        sum += g;
    }
    sum = wave_sum(sum);
    if (lane == 0) a.sumdx[r] = sum;
}

// The parameter gradients that reduce over the batch: dWe = z^T denc, dWa = x^T dpre, dH = h^T ds, and the bias sums as one
// more column (c = D) whose z and x are 1.  Block (column tile of 64, factor chunk of 16, row segment): wave w takes every
// fourth row of the segment in ascending order, the four waves' sums are added in wave order, and the kGradSegs segment sums
// are added in segment order by the optimizer pass: the order depends on the shapes alone, no atomics.
template <class Rows>
__device__ __forceinline__ void att_grad_body(const AttArgs &a, const Rows &rows) {
    __shared__ float sh[kBlock / 64][kFC][64];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int c = blockIdx.x * 64 + lane;
    const int f0 = blockIdx.y * kFC;
    const int seg = blockIdx.z;
    const int64_t rps = (a.nrows + kGradSegs - 1) / kGradSegs;
    const int64_t r_lo = seg * rps, r_hi = r_lo + rps < a.nrows ? r_lo + rps : a.nrows;
    float aWe[kFC], aWa[kFC], aH[kFC];
#pragma unroll
    for (int k = 0; k < kFC; k++) aWe[k] = aWa[k] = aH[k] = 0.0f;
    for (int64_t r = r_lo + w; r < r_hi; r += kBlock / 64) {
        float xv = 0.0f, zv = 0.0f, dsv = 0.0f;
        if (c < a.D) {
            xv = bf16_f32(rows.xu(a, r)[c]);  // r is the same in every lane
            zv = a.s[r * a.D + c] * xv;
            dsv = a.gx[r * a.D + c];
        } else if (c == a.D) {
            xv = zv = 1.0f;
        }
        const float g = a.gs[r];
#pragma unroll
        for (int k = 0; k < kFC; k++) {
            if (f0 + k < a.d) {
                const int64_t o = r * a.d + f0 + k;
                aWe[k] = fmaf(zv, g * a.vx[o], aWe[k]);
                aWa[k] = fmaf(xv, a.dpre[o], aWa[k]);
                aH[k] = fmaf(dsv, a.h[o], aH[k]);
            }
        }
    }
    const int64_t nH = (int64_t)a.d * a.D, nW = (int64_t)(a.D + 1) * a.d;
    float *gH = a.gpart + seg * a.gstride, *gWa = gH + nH, *gWe = gWa + nW;
#pragma unroll
    for (int t = 0; t < 3; t++) {
        if (t) __syncthreads();
#pragma unroll
        for (int k = 0; k < kFC; k++) sh[w][k][lane] = t == 0 ? aH[k] : t == 1 ? aWa[k] : aWe[k];
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kFC / (kBlock / 64); j++) {
            const int k = w + j * (kBlock / 64);
            const float v = ((sh[0][k][lane] + sh[1][k][lane]) + sh[2][k][lane]) + sh[3][k][lane];
            if (f0 + k >= a.d) continue;
            if (t == 0) {
                if (c < a.D) gH[(int64_t)(f0 + k) * a.D + c] = v;
            } else if (c <= a.D) {
                (t == 1 ? gWa : gWe)[(int64_t)c * a.d + f0 + k] = v;
            }
        }
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------

// What gorse_fm_epoch's loop asks of a training set.  Every launch goes to the handle's stream; k is the batch, r0 its first
// row and nr its rows.  The loop itself owns everything that reads no row: the loss, att_bwd_ds_kernel, the optimizer passes,
// the in-flight window, cancel, the tags and the cost.
struct TrainSource {
    virtual ~TrainSource() {}
    virtual const float *targets(const gorse_fm *h) const = 0;  // device, n
    virtual int32_t ready(const gorse_fm *h) const = 0;         // the set is complete (embeddings for every field)
    virtual int32_t plan(gorse_fm *h, int32_t bs, int64_t *max_slots) const = 0;  // the per-batch plan of this batch size
    virtual int32_t forward(gorse_fm *h, int64_t r0, int64_t nr) const = 0;
    virtual int32_t branch_forward(gorse_fm *h, int e, int64_t r0, int64_t nr) const = 0;
    virtual int32_t branch_gx(gorse_fm *h, int e, int64_t r0, int64_t nr) const = 0;
    virtual int32_t branch_grad(gorse_fm *h, int e, int64_t r0, int64_t nr) const = 0;
    virtual int32_t accum(gorse_fm *h, int64_t k, int64_t r0, int64_t nr, int64_t tag_hi) const = 0;
};

// fm_samples.hip: the source over h->smp
const TrainSource &samples_source();

// fm.hip: field e on a batch of nrows rows with embeddings x (scoring keeps nothing per field: every field works in field 0's
// buffers); the branch's per-batch buffers; the per-batch buffers every plan needs
AttArgs branch_args(gorse_fm *h, int k, const uint16_t *x, int64_t nrows, const float *vx, bool train);
int32_t ensure_step(gorse_fm *h, int32_t bs, int64_t max_slots);

// a training forward launch over src: what every source fills in the same way
template <class Src>
inline int32_t train_forward(gorse_fm *h, const Src &src, const float *tgt, int64_t nr) {
    FwdArgs<Src> f{};
    f.src = src;
    f.tgt = tgt;
    f.V = h->V.p, f.W = h->W.p, f.B = h->B.p;
    f.nrows = nr, f.d = h->d;
    f.inv_n = 1.0f / (float)nr;
    f.gs = h->gs.p, f.loss = h->loss.p, f.vx = h->vx.p;
    if (h->n_fields > 0) f.out = h->a_logit.p;
    return launch_forward<kTrain>(h->s, f);
}

// the accumulation's arguments but the batch's slots and entries
inline AccArgs accum_args(gorse_fm *h, int64_t nr, int64_t tag_hi) {
    AccArgs a{};
    a.V = h->V.p;
    a.gs = h->gs.p, a.loss = h->loss.p;
    a.vx = h->n_fields > 0 ? h->a_vxe.p : h->vx.p;  // with fields: vx + sum of enc, so that dV carries g * enc
    a.nrows = nr, a.d = h->d;
    a.tag_hi = tag_hi, a.tag = h->tag.p;
    a.gV = h->gV.p, a.gW = h->gW.p, a.gB = h->gB.p, a.cost = h->cost.p;
    return a;
}

inline dim3 grad_grid(const AttArgs &a) {
    return dim3((unsigned)ceil_div(a.D + 1, 64), (unsigned)ceil_div(a.d, kFC), kGradSegs);
}

}  // namespace fm
}  // namespace gorse
