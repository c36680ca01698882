// fm.hip -- ctr.AFM (model/ctr/fm.go:111-134).  First the factorization machine itself (fm.go:111-126); the item-embedding
// attention branch (fm.go:127-132) follows further down ("the item-embedding branch").  The factorization machine:
// logit = B + sum_j W[idx_j] x_j + 0.5 sum_f ((sum_j V[idx_j,f] x_j)^2 - sum_j V[idx_j,f]^2 x_j^2), trained with
// BCEWithLogits on contiguous batches (fm.go:362-378) and the reference's dense SGD / Adam steps
// (common/nn/optimizers.go:70-84, 118-156), plus batch scoring (BatchInternalPredict, fm.go:156-178).
//
// One training step = three launches, enqueued for a whole epoch without a host round trip:
//   fm_forward_kernel  (fm_internal.hpp: the one forward kernel, here over PaddedRows) one sample per G-lane group: gathers the
//                      row's V / W entries, DPP-reduces the pairwise term, writes the sample's loss, its loss gradient
//                      g_b = (sigmoid(logit) - y) / n_batch and its vx_f = sum_j V[idx_j,f] x_j;
//   fm_accum_kernel    one wave per feature the batch touches (the batch's (feature, position) list is sorted once per training
//                      set and batch size): the row's gradient summed over its positions in position order, in a fixed shape,
//                      no atomics; one extra block reduces dB and the batch's mean loss in a fixed tree;
//   fm_opt_kernel      one pass over every parameter (and the Adam moments) with 16-byte accesses: the dense step the reference
//                      takes, with the touched rows' gradient found through a per-row tag (step, slot).
// Every floats.* call of the reference runs the AVX512 kernels of common/floats/src/floats_avx512.c: a 16-lane FMA body and
// unfused 8-lane / scalar tails, and partitionAligned(.., 32) leaves the tail at the tensor's last len % 16 elements; the
// optimizer kernel applies the same rule by element position (fmaf vs. mul then add; the library builds with -ffp-contract=off).
#include "fm_train.hpp"

namespace gorse {
namespace fm {

constexpr float kBeta1 = 0.9f, kBeta2 = 0.999f, kEps = 1e-8f;

// One wave per touched feature over the batch's (feature, position) lists: fm_accum_body (fm_train.hpp) over PaddedEntries.
template <int G, int NF>
__global__ __launch_bounds__(kBlock) void fm_accum_kernel(AccArgs a) {
    fm_accum_body<G, NF>(a, PaddedEntries{a.pos, a.val, a.width});
}

struct OptArgs {  // tensor t = 0 (V), 1 (W), 2 (B); the kernel selects by constant index only (no private copy of the block)
    float *p[3], *m[3], *v[3];
    int64_t len[3];
    int64_t blocks0, blocks1;  // blocks of V, then W; the last block is B
    int d;
    const int64_t *tag;
    int64_t tag_hi;
    const float *gV, *gW, *gB;
    float wd, lr, c1, c2;  // c1 = 1 - beta1, c2 = 1 - beta2 (fp32, as the reference forms them)
};

template <bool ADAM>
__device__ __forceinline__ void opt_elem(float &p, float &m, float &v, float g, bool fused, float wd, float lr, float c1,
                                         float c2) {
    // floats.MulConstAddTo(p, wd, grad, b1): b1 = grad + p * wd
    const float b1 = fused ? fmaf(p, wd, g) : g + p * wd;
    if (!ADAM) {
        // floats.MulConstAdd(b, -lr, p)
        p = fused ? fmaf(b1, -lr, p) : p + b1 * (-lr);
        return;
    }
    float b2 = b1 - m;                                   // floats.SubTo(b1, m, b2)
    m = fused ? fmaf(b2, c1, m) : m + b2 * c1;       // floats.MulConstAdd(b2, 1 - beta1, m)
    b2 = b1 * b1;                                        // floats.MulTo(b1, b1, b2)
    b2 = b2 - v;                                         // floats.Sub(b2, v)
    v = fused ? fmaf(b2, c2, v) : v + b2 * c2;       // floats.MulConstAdd(b2, 1 - beta2, v)
    // floats.SqrtTo(v, b2), correctly rounded: v_sqrt_f32 alone is not; the fp64 square root is, and rounding it to fp32
    // again gives the correctly rounded fp32 root (53 >= 2 x 24 + 2 bits: double rounding is harmless for a square root)
    b2 = (float)sqrt((double)v);
    b2 = b2 + kEps;                                      // floats.AddConst(b2, eps)
    const float q = m / b2;                              // floats.DivTo(m, b2, b1) (the division is correctly rounded)
    p = fused ? fmaf(q, -lr, p) : p + q * (-lr);     // floats.MulConstAdd(b1, -lr, p)
}

template <bool ADAM>
__global__ __launch_bounds__(kBlock) void fm_opt_kernel(OptArgs a) {
    int t;
    int64_t blk = blockIdx.x;
    if (blk < a.blocks0) {
        t = 0;
    } else if (blk < a.blocks0 + a.blocks1) {
        t = 1;
        blk -= a.blocks0;
    } else {
        t = 2;
        blk = 0;
    }
    const int64_t L = t == 0 ? a.len[0] : t == 1 ? a.len[1] : a.len[2];
    const int64_t e0 = (blk * kBlock + threadIdx.x) * 4;
    if (e0 >= L) return;
    const int64_t body = L - L % 16;  // elements past this run the reference's unfused tails
    const int rowlen = t == 0 ? a.d : 1;
    float *P = t == 0 ? a.p[0] : t == 1 ? a.p[1] : a.p[2];
    float *M = t == 0 ? a.m[0] : t == 1 ? a.m[1] : a.m[2];
    float *Vm = t == 0 ? a.v[0] : t == 1 ? a.v[1] : a.v[2];
    float p[4], m[4], v[4], g[4];
    const bool full = e0 + 4 <= L;
    if (full) {
        const float4 p4 = *reinterpret_cast<const float4 *>(P + e0);
        p[0] = p4.x, p[1] = p4.y, p[2] = p4.z, p[3] = p4.w;
        if (ADAM) {
            const float4 m4 = *reinterpret_cast<const float4 *>(M + e0);
            const float4 v4 = *reinterpret_cast<const float4 *>(Vm + e0);
            m[0] = m4.x, m[1] = m4.y, m[2] = m4.z, m[3] = m4.w;
            v[0] = v4.x, v[1] = v4.y, v[2] = v4.z, v[3] = v4.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            p[k] = e0 + k < L ? P[e0 + k] : 0.0f;
            m[k] = ADAM && e0 + k < L ? M[e0 + k] : 0.0f;
            v[k] = ADAM && e0 + k < L ? Vm[e0 + k] : 0.0f;
        }
    }
    // gradient: the touched rows' sums through the tag of their row, zero elsewhere
    // a 32-bit division wherever the index fits (the 64-bit one is a long instruction sequence)
    int64_t row = e0 < ((int64_t)1 << 32) ? (int64_t)((uint32_t)e0 / (uint32_t)rowlen) : e0 / rowlen;
    int col = (int)(e0 - row * rowlen);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        float gk = 0.0f;
        if (t == 2) {
            gk = a.gB[0];
        } else if (e0 + k < L) {
            const int64_t tg = a.tag[row];
            if ((tg & ~(int64_t)0xffffffff) == a.tag_hi) {
                const int64_t slot = tg & 0xffffffff;
                gk = t == 0 ? a.gV[slot * a.d + col] : a.gW[slot];
            }
        }
        g[k] = gk;
        if (++col == rowlen) {
            col = 0;
            row++;
        }
    }
#pragma unroll
    for (int k = 0; k < 4; k++) opt_elem<ADAM>(p[k], m[k], v[k], g[k], e0 + k < body, a.wd, a.lr, a.c1, a.c2);
    if (full) {
        *reinterpret_cast<float4 *>(P + e0) = make_float4(p[0], p[1], p[2], p[3]);
        if (ADAM) {
            *reinterpret_cast<float4 *>(M + e0) = make_float4(m[0], m[1], m[2], m[3]);
            *reinterpret_cast<float4 *>(Vm + e0) = make_float4(v[0], v[1], v[2], v[3]);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (e0 + k < L) {
                P[e0 + k] = p[k];
                if (ADAM) {
                    M[e0 + k] = m[k];
                    Vm[e0 + k] = v[k];
                }
            }
        }
    }
}

// ---- the item-embedding branch (fm.go:127-132; nn.Attention + nn.Linear, common/nn/layers.go:36-60, 160-190) ------------
// Per field with embedding dimension D and a batch of n rows x (bf16, widened on load):
//   pre = x Wa + ba, h = relu(pre), s = h H, a = Softmax(s, 1), z = a * x, enc = z We + be, logit += sum_f vx_f enc_f.
// The reference's Softmax subtracts the maxima and divides by the sums through Tensor.sub / Tensor.div, which index the
// (n x 1) operand by flat index % n (tensor.go:328-337, 370-379): element (r, c) uses row (r D + c) % n's maximum and sum,
// forward and backward (op.go:760-777).  These kernels reproduce that indexing, so every maximum must exist before any
// exponential and every sum before any a: three launches forward, two backward plus the parameter-gradient reduction.
// One wave per row; lanes stride over the D columns; skinny products are formed 16 factors at a time and wave-reduced in
// a fixed butterfly.  The three forward kernels are in fm_internal.hpp (here over BatchRows; fm_resident.hip runs them over
// the slices of a launch round).

struct LossArgs {
    const float *logit, *tgt;  // tgt: the batch's rows
    const float *vx, *esum;
    int64_t nrows;
    int d;
    float inv_n;
    float *gs, *loss, *vxe;
};

// loss and g from the full logit (the expressions of fm_forward_kernel), and vx + sum of enc: d logit / d vx, which
// fm_accum_kernel reads in vx's place
__global__ __launch_bounds__(kBlock) void att_loss_kernel(LossArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < a.nrows * a.d) a.vxe[i] = a.vx[i] + a.esum[i];
    if (i >= a.nrows) return;
    const float logit = a.logit[i];
    const float y = (a.tgt[i] + 1.0f) * 0.5f;
    a.loss[i] = fmaxf(logit, 0.0f) - logit * y + logf(1.0f + expf(-fabsf(logit)));
    a.gs[i] = (1.0f / (1.0f + expf(-logit)) - y) * a.inv_n;
}

// denc = g vx, dz = denc We^T, da = dz * x, gx = a * da and each row's sum of gx: att_bwd_gx_body (fm_train.hpp) over BatchRows
__global__ __launch_bounds__(kBlock) void att_bwd_gx_kernel(AttArgs a) { att_bwd_gx_body(a, BatchRows{}); }

// ds = gx - a * sumdx[(r D + c) % n], dh = ds H^T, dpre = (pre > 0) dh
__global__ __launch_bounds__(kBlock) void att_bwd_ds_kernel(AttArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (r >= a.nrows) return;
    const uint32_t n = (uint32_t)a.nrows;
    const uint32_t m0 = (uint32_t)((r * a.D) % a.nrows);
    const float *ar = a.s + r * a.D;
    float *gr = a.gx + r * a.D;
    for (int c = lane; c < a.D; c += 64) {  // gx.sub(y.mul(sumdx)): the product is rounded before the difference
        const float t = ar[c] * a.sumdx[(m0 + (uint32_t)c) % n];
        gr[c] = gr[c] - t;
    }
    for (int f0 = 0; f0 < a.d; f0 += kFC) {  // this lane re-reads the elements it wrote
        float acc[kFC];
#pragma unroll
        for (int k = 0; k < kFC; k++) acc[k] = 0.0f;
        for (int c = lane; c < a.D; c += 64) {
            const float dsv = gr[c];
            // chunk entries past d re-read H's last row into sums nobody keeps: no per-entry condition to carry
            const float *hp = a.H + c;
#pragma unroll
            for (int k = 0; k < kFC; k++) acc[k] = fmaf(dsv, hp[min(f0 + k, a.d - 1) * a.D], acc[k]);
        }
        const float mine = reduce_pick(acc, lane);
        if (lane < kFC && f0 + lane < a.d) {
            const int64_t o = r * a.d + f0 + lane;
            a.dpre[o] = a.h[o] > 0.0f ? mine : 0.0f;
        }
    }
}

// the parameter gradients that reduce over the batch: att_grad_body (fm_train.hpp) over BatchRows
__global__ __launch_bounds__(kBlock) void att_grad_kernel(AttArgs a) { att_grad_body(a, BatchRows{}); }

// The dense step of the branch's tensors (blockIdx.y = tensor number in Parameters() order: per field H, Wa, ba, We, be), each
// as its own tensor: the FMA body / unfused tail split lies at its own last len % 16 elements.  The descriptors are read
// from device memory, so no by-value argument block is indexed by a runtime number.
template <bool ADAM>
__global__ __launch_bounds__(kBlock) void fm_dense_opt_kernel(const DenseDesc *descs, float wd, float lr, float c1, float c2) {
    const DenseDesc t = descs[blockIdx.y];
    const int64_t L = t.len;
    const int64_t e0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * 4;
    if (e0 >= L) return;
    const int64_t body = L - L % 16;
    float p[4], m[4], v[4], g[4];
    const bool full = e0 + 4 <= L;
    if (full) {
        const float4 p4 = *reinterpret_cast<const float4 *>(t.p + e0);
        p[0] = p4.x, p[1] = p4.y, p[2] = p4.z, p[3] = p4.w;
        if (ADAM) {
            const float4 m4 = *reinterpret_cast<const float4 *>(t.m + e0);
            const float4 v4 = *reinterpret_cast<const float4 *>(t.v + e0);
            m[0] = m4.x, m[1] = m4.y, m[2] = m4.z, m[3] = m4.w;
            v[0] = v4.x, v[1] = v4.y, v[2] = v4.z, v[3] = v4.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            p[k] = e0 + k < L ? t.p[e0 + k] : 0.0f;
            m[k] = ADAM && e0 + k < L ? t.m[e0 + k] : 0.0f;
            v[k] = ADAM && e0 + k < L ? t.v[e0 + k] : 0.0f;
        }
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        float gk = 0.0f;
        if (e0 + k < L) {
#pragma unroll
            for (int s = 0; s < kGradSegs; s++) gk += t.g[s * t.gstride + e0 + k];
        }
        g[k] = gk;
    }
#pragma unroll
    for (int k = 0; k < 4; k++) opt_elem<ADAM>(p[k], m[k], v[k], g[k], e0 + k < body, wd, lr, c1, c2);
    if (full) {
        *reinterpret_cast<float4 *>(t.p + e0) = make_float4(p[0], p[1], p[2], p[3]);
        if (ADAM) {
            *reinterpret_cast<float4 *>(t.m + e0) = make_float4(m[0], m[1], m[2], m[3]);
            *reinterpret_cast<float4 *>(t.v + e0) = make_float4(v[0], v[1], v[2], v[3]);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (e0 + k < L) {
                t.p[e0 + k] = p[k];
                if (ADAM) {
                    t.m[e0 + k] = m[k];
                    t.v[e0 + k] = v[k];
                }
            }
        }
    }
}

// ---- host side ----------------------------------------------------------------------

// math32.Pow(x, y) for a positive integer y (chewxy/math32 pow.go, the float32 statement of Go's math.Pow):
// x = x1 * 2^xe by Frexp, then square-and-multiply on the mantissa with the exponent kept apart.
inline float pow_int(float x, int64_t y) {
    int xe = 0;
    float x1 = std::frexp(x, &xe);
    float a1 = 1.0f;
    int64_t ae = 0;
    for (int64_t i = y; i != 0; i >>= 1) {
        if (i & 1) {
            a1 *= x1;
            ae += xe;
        }
        x1 *= x1;
        xe <<= 1;
        if (x1 < 0.5f) {
            x1 += x1;
            xe--;
        }
    }
    return std::ldexp(a1, (int)ae);
}

// nn.Adam.Step's lr for step t (optimizers.go:121-123), in fp32
inline float adam_lr(float alpha, int64_t t) {
    const float fix1 = 1.0f - pow_int(kBeta1, t);
    const float fix2 = 1.0f - pow_int(kBeta2, t);
    return alpha * std::sqrt(fix2) / fix1;
}

// train: the batches' position lists index a training set's padded positions in int32; scoring indexes in int64
int32_t check_rows(const gorse_fm *h, int64_t n, int32_t width, const int32_t *indices, const float *values, bool train) {
    if (n < 0 || width <= 0) return fail(GORSE_ERR_INVALID, "n must be >= 0 and width positive (n = %lld, width = %d)", (long long)n, width);
    if (n > 0 && (!indices || !values)) return fail(GORSE_ERR_INVALID, "indices / values are NULL");
    if (train && n * (int64_t)width > INT32_MAX) return fail(GORSE_ERR_INVALID, "a training set's n x width must fit int32");
    for (int64_t e = 0; e < n * width; e++)
        if (indices[e] < 0 || indices[e] >= h->nf)
            return fail(GORSE_ERR_RANGE, "feature index %d at position %lld out of range [0,%lld)", indices[e], (long long)e,
                        (long long)h->nf);
    return GORSE_OK;
}

int32_t launch_accum(gorse_fm *h, const AccArgs &a) {
    const int64_t grid = ceil_div(a.nslots * 64, kBlock) + 1;
    with_lanes(h->d, [&](auto G, auto NF) {
        fm_accum_kernel<decltype(G)::value, decltype(NF)::value><<<dim3((unsigned)grid), dim3(kBlock), 0, h->s>>>(a);
    });
    GORSE_HIP_CHECK(hipGetLastError());
    return GORSE_OK;
}

// The (feature, position) order of every batch: positions with a nonzero value, sorted by feature then position (the order
// the reference's embedding backward adds them in, op.go:694-699).  Depends only on the training set and the batch size.
int32_t build_plan(gorse_fm *h, int32_t bs) {
    const int64_t nb = ceil_div(h->n, bs);
    const int w = h->width;
    std::vector<std::vector<uint64_t>> keys((size_t)nb);
    parallel_rows(nb, nullptr, [&](int, int64_t k0, int64_t k1) {
        for (int64_t k = k0; k < k1; k++) {
            const int64_t r0 = k * bs, r1 = std::min<int64_t>(h->n, r0 + bs);
            auto &ks = keys[(size_t)k];
            ks.clear();
            for (int64_t p = 0; p < (r1 - r0) * w; p++)
                if (h->h_val[(size_t)(r0 * w + p)] != 0.0f)
                    ks.push_back(((uint64_t)(uint32_t)h->h_idx[(size_t)(r0 * w + p)] << 32) | (uint64_t)p);
            std::sort(ks.begin(), ks.end());
        }
    });
    std::vector<int32_t> uniq, seg, pos;
    h->uoff.assign((size_t)nb + 1, 0);
    h->max_slots = 0;
    for (int64_t k = 0; k < nb; k++) {
        const auto &ks = keys[(size_t)k];
        for (size_t q = 0; q < ks.size(); q++) {
            const int32_t f = (int32_t)(ks[q] >> 32);
            if (q == 0 || (int32_t)(ks[q - 1] >> 32) != f) {
                uniq.push_back(f);
                seg.push_back((int32_t)pos.size());
            }
            pos.push_back((int32_t)(ks[q] & 0xffffffffu));
        }
        h->uoff[(size_t)k + 1] = (int64_t)uniq.size();
        h->max_slots = std::max<int64_t>(h->max_slots, h->uoff[(size_t)k + 1] - h->uoff[(size_t)k]);
    }
    seg.push_back((int32_t)pos.size());
    GORSE_TRY(h->uniq.alloc(uniq.size()));
    GORSE_TRY(h->seg.alloc(seg.size()));
    GORSE_TRY(h->pos.alloc(pos.size()));
    if (!uniq.empty()) GORSE_HIP_CHECK(hipMemcpy(h->uniq.p, uniq.data(), uniq.size() * 4, hipMemcpyHostToDevice));
    GORSE_HIP_CHECK(hipMemcpy(h->seg.p, seg.data(), seg.size() * 4, hipMemcpyHostToDevice));
    if (!pos.empty()) GORSE_HIP_CHECK(hipMemcpy(h->pos.p, pos.data(), pos.size() * 4, hipMemcpyHostToDevice));
    h->plan_bs = bs;
    return GORSE_OK;
}

// what a step works in whatever the source: the touched rows' gradient sums and the batch's g, loss and vx
int32_t ensure_step(gorse_fm *h, int32_t bs, int64_t max_slots) {
    GORSE_TRY(h->gV.ensure((size_t)std::max<int64_t>(1, max_slots) * h->d));
    GORSE_TRY(h->gW.ensure((size_t)std::max<int64_t>(1, max_slots)));
    GORSE_TRY(h->gs.ensure((size_t)bs));
    GORSE_TRY(h->loss.ensure((size_t)bs));
    return h->vx.ensure((size_t)bs * h->d);
}

// ---- the embedding branch: host side -----------------------------------------------------

// per-batch buffers of the branch for batches of up to `rows` rows; train: also what the backward needs
int32_t ensure_branch(gorse_fm *h, int64_t rows, bool train) {
    const int maxD = std::max(1, max_emb_dim(h));
    GORSE_TRY(h->a_rmax.ensure((size_t)rows));
    GORSE_TRY(h->a_rsum.ensure((size_t)rows));
    GORSE_TRY(h->a_logit.ensure((size_t)rows));
    for (int k = 0; k < h->n_fields; k++) {
        // scoring keeps nothing per field: every field works in field 0's buffers
        Field &F = h->fld[train ? k : 0];
        GORSE_TRY(F.h.ensure((size_t)rows * h->d));
        GORSE_TRY(F.a.ensure((size_t)rows * (train ? F.D : maxD)));
    }
    if (!train) return GORSE_OK;
    GORSE_TRY(h->a_sumdx.ensure((size_t)rows));
    GORSE_TRY(h->a_gx.ensure((size_t)rows * maxD));
    GORSE_TRY(h->a_dpre.ensure((size_t)rows * h->d));
    GORSE_TRY(h->a_esum.ensure((size_t)rows * h->d));
    GORSE_TRY(h->a_vxe.ensure((size_t)rows * h->d));
    return GORSE_OK;
}

// field k on a batch of nrows rows with embeddings x: scoring keeps nothing per field, every field works in field 0's buffers
AttArgs branch_args(gorse_fm *h, int k, const uint16_t *x, int64_t nrows, const float *vx, bool train) {
    Field &F = h->fld[k], &S = h->fld[train ? k : 0];
    AttArgs a = field_args(h, k);
    a.x = x;
    a.nrows = nrows;
    a.h = S.h.p, a.s = S.a.p;
    a.rmax = h->a_rmax.p, a.rsum = h->a_rsum.p;
    a.vx = vx;
    a.logit = h->a_logit.p;
    a.esum = train ? h->a_esum.p : nullptr;
    a.first = k == 0;
    a.gs = h->gs.p, a.gx = h->a_gx.p, a.sumdx = h->a_sumdx.p, a.dpre = h->a_dpre.p;
    a.gpart = F.gpart.p, a.gstride = (int64_t)F.gstride();
    return a;
}

// the training set of gorse_fm_set_train (+ gorse_fm_set_train_embeddings): padded rows, one embedding row per sample
struct PaddedTrain final : TrainSource {
    const float *targets(const gorse_fm *h) const override { return h->tgt.p; }
    int32_t ready(const gorse_fm *h) const override {
        for (int k = 0; k < h->n_fields; k++)
            if (!h->fld[k].have_x)
                return fail(GORSE_ERR_INVALID, "embedding field %d has no training embeddings (gorse_fm_set_train_embeddings)", k);
        return GORSE_OK;
    }
    int32_t plan(gorse_fm *h, int32_t bs, int64_t *max_slots) const override {
        if (h->plan_bs != bs) GORSE_TRY(build_plan(h, bs));
        *max_slots = h->max_slots;
        return GORSE_OK;
    }
    int32_t forward(gorse_fm *h, int64_t r0, int64_t nr) const override {
        return train_forward(h, PaddedRows{h->idx.p, h->val.p, r0, h->width}, h->tgt.p + r0, nr);
    }
    AttArgs args(gorse_fm *h, int e, int64_t r0, int64_t nr) const {
        return branch_args(h, e, h->fld[e].x.p + r0 * h->fld[e].D, nr, h->vx.p, true);
    }
    int32_t branch_forward(gorse_fm *h, int e, int64_t r0, int64_t nr) const override {
        return fm::branch_forward(h->s, args(h, e, r0, nr), BatchRows{});
    }
    int32_t branch_gx(gorse_fm *h, int e, int64_t r0, int64_t nr) const override {
        att_bwd_gx_kernel<<<dim3(row_grid(nr)), dim3(kBlock), 0, h->s>>>(args(h, e, r0, nr));
        GORSE_HIP_CHECK(hipGetLastError());
        return GORSE_OK;
    }
    int32_t branch_grad(gorse_fm *h, int e, int64_t r0, int64_t nr) const override {
        const AttArgs a = args(h, e, r0, nr);
        att_grad_kernel<<<grad_grid(a), dim3(kBlock), 0, h->s>>>(a);
        GORSE_HIP_CHECK(hipGetLastError());
        return GORSE_OK;
    }
    int32_t accum(gorse_fm *h, int64_t k, int64_t r0, int64_t nr, int64_t tag_hi) const override {
        AccArgs a = accum_args(h, nr, tag_hi);
        a.uniq = h->uniq.p, a.seg = h->seg.p, a.pos = h->pos.p;
        a.slot0 = h->uoff[(size_t)k], a.nslots = h->uoff[(size_t)k + 1] - h->uoff[(size_t)k];
        a.val = h->val.p + r0 * h->width;
        a.width = h->width;
        return launch_accum(h, a);
    }
};

int32_t check_field(const gorse_fm *h, int32_t field) {
    if (!h) return fail(GORSE_ERR_INVALID, "handle is NULL");
    if (field < 0 || field >= h->n_fields)
        return fail(GORSE_ERR_INVALID, "embedding field %d out of range [0,%d)", field, h->n_fields);
    return GORSE_OK;
}

}  // namespace fm
}  // namespace gorse

using namespace gorse;

extern "C" int32_t gorse_fm_create(gorse_fm **out, int32_t device, int64_t n_features, int32_t n_factors) {
    if (!out) return fail(GORSE_ERR_INVALID, "handle pointer is NULL");
    *out = nullptr;
    if (n_features <= 0 || n_features > INT32_MAX) return fail(GORSE_ERR_INVALID, "n_features must be in [1, 2^31)");
    if (n_factors < 1 || n_factors > fm::kMaxFactors) return fail(GORSE_ERR_INVALID, "n_factors must be in 1..128 (got %d)", n_factors);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(GORSE_ERR_NO_DEVICE, "no HIP device visible (libgorse_hip needs an MI355X / gfx950)");
    if (device < 0 || device >= ndev) return fail(GORSE_ERR_INVALID, "device %d out of range [0,%d)", device, ndev);
    GORSE_HIP_CHECK(hipSetDevice(device));
    gorse_fm *h = new (std::nothrow) gorse_fm();
    if (!h) return fail(GORSE_ERR_NOMEM, "out of host memory");
    h->device = device;
    h->nf = n_features;
    h->d = n_factors;
    auto init = [&]() -> int32_t {
        GORSE_HIP_CHECK(hipStreamCreateWithFlags(&h->s, hipStreamNonBlocking));
        GORSE_HIP_CHECK(hipEventCreateWithFlags(&h->ev[0], hipEventDisableTiming));
        GORSE_HIP_CHECK(hipEventCreateWithFlags(&h->ev[1], hipEventDisableTiming));
        const size_t nv = (size_t)n_features * n_factors, nw = (size_t)n_features;
        for (auto *b : {&h->V, &h->mV, &h->vV}) GORSE_TRY(b->alloc(nv));
        for (auto *b : {&h->W, &h->mW, &h->vW}) GORSE_TRY(b->alloc(nw));
        for (auto *b : {&h->B, &h->mB, &h->vB, &h->gB, &h->cost}) GORSE_TRY(b->alloc(4));
        GORSE_TRY(h->tag.alloc(nw));
        GORSE_HIP_CHECK(hipMemsetAsync(h->tag.p, 0, nw * sizeof(int64_t), h->s));
        for (auto *b : {&h->V, &h->mV, &h->vV, &h->W, &h->mW, &h->vW, &h->B, &h->mB, &h->vB})
            GORSE_HIP_CHECK(hipMemsetAsync(b->p, 0, b->n * sizeof(float), h->s));
        GORSE_HIP_CHECK(hipStreamSynchronize(h->s));
        return GORSE_OK;
    };
    const int32_t rc = init();
    if (rc != GORSE_OK) {
        gorse_fm_destroy(h);
        return rc;
    }
    *out = h;
    return GORSE_OK;
}

extern "C" int32_t gorse_fm_destroy(gorse_fm *h) {
    if (!h) return GORSE_OK;
    (void)hipSetDevice(h->device);
    if (h->s) (void)hipStreamSynchronize(h->s);
    for (auto e : h->ev)
        if (e) (void)hipEventDestroy(e);
    for (auto e : h->r_ev)
        if (e) (void)hipEventDestroy(e);
    for (auto e : h->e_ev)
        if (e) (void)hipEventDestroy(e);
    if (h->s) (void)hipStreamDestroy(h->s);
    delete h;
    return GORSE_OK;
}

extern "C" int32_t gorse_fm_set_params(gorse_fm *h, float B, const float *W, const float *V) {
    if (!h || !W || !V) return fail(GORSE_ERR_INVALID, "handle / W / V is NULL");
    GORSE_HIP_CHECK(hipSetDevice(h->device));
    GORSE_HIP_CHECK(hipStreamSynchronize(h->s));
    GORSE_HIP_CHECK(hipMemcpy(h->V.p, V, (size_t)h->nf * h->d * sizeof(float), hipMemcpyHostToDevice));
    GORSE_HIP_CHECK(hipMemcpy(h->W.p, W, (size_t)h->nf * sizeof(float), hipMemcpyHostToDevice));
    GORSE_HIP_CHECK(hipMemcpy(h->B.p, &B, sizeof(float), hipMemcpyHostToDevice));
    for (auto *b : {&h->mV, &h->vV, &h->mW, &h->vW, &h->mB, &h->vB})
        GORSE_HIP_CHECK(hipMemsetAsync(b->p, 0, b->n * sizeof(float), h->s));
    GORSE_HIP_CHECK(hipStreamSynchronize(h->s));
    h->adam_t = 0;
    return GORSE_OK;
}

extern "C" int32_t gorse_fm_get_params(gorse_fm *h, float *B, float *W, float *V) {
    if (!h) return fail(GORSE_ERR_INVALID, "handle is NULL");
    GORSE_HIP_CHECK(hipSetDevice(h->device));
    GORSE_HIP_CHECK(hipStreamSynchronize(h->s));
    if (V) GORSE_HIP_CHECK(hipMemcpy(V, h->V.p, (size_t)h->nf * h->d * sizeof(float), hipMemcpyDeviceToHost));
    if (W) GORSE_HIP_CHECK(hipMemcpy(W, h->W.p, (size_t)h->nf * sizeof(float), hipMemcpyDeviceToHost));
    if (B) GORSE_HIP_CHECK(hipMemcpy(B, h->B.p, sizeof(float), hipMemcpyDeviceToHost));
    return GORSE_OK;
}

extern "C" int32_t gorse_fm_set_train(gorse_fm *h, int64_t n, int32_t width, const int32_t *indices, const float *values,
                                      const float *target) {
    if (!h) return fail(GORSE_ERR_INVALID, "handle is NULL");
    if (n <= 0) return fail(GORSE_ERR_INVALID, "the training set is empty");
    if (!target) return fail(GORSE_ERR_INVALID, "target is NULL");
    GORSE_TRY(fm::check_rows(h, n, width, indices, values, true));
    GORSE_HIP_CHECK(hipSetDevice(h->device));
    GORSE_HIP_CHECK(hipStreamSynchronize(h->s));
    const size_t ne = (size_t)n * width;
    h->smp.reset();  // a padded set replaces one in sample form
    h->smp_dropped = false;
    h->h_idx.assign(indices, indices + ne);
    h->h_val.assign(values, values + ne);
    GORSE_TRY(h->idx.alloc(ne));
    GORSE_TRY(h->val.alloc(ne));
    GORSE_TRY(h->tgt.alloc((size_t)n));
    GORSE_HIP_CHECK(hipMemcpy(h->idx.p, indices, ne * 4, hipMemcpyHostToDevice));
    GORSE_HIP_CHECK(hipMemcpy(h->val.p, values, ne * 4, hipMemcpyHostToDevice));
    GORSE_HIP_CHECK(hipMemcpy(h->tgt.p, target, (size_t)n * 4, hipMemcpyHostToDevice));
    h->n = n;
    h->width = width;
    h->plan_bs = 0;  // the batches' feature order is rebuilt for the new set
    for (int k = 0; k < h->n_fields; k++) {  // the embeddings belong to the set they were uploaded for
        h->fld[k].x.release();
        h->fld[k].have_x = false;
    }
    return GORSE_OK;
}

extern "C" int32_t gorse_fm_set_embedding_dims(gorse_fm *h, int32_t n_fields, const int32_t *dims) {
    if (!h) return fail(GORSE_ERR_INVALID, "handle is NULL");
    if (n_fields < 0 || n_fields > fm::kMaxFields)
        return fail(GORSE_ERR_INVALID, "n_fields must be in 0..%d (got %d)", fm::kMaxFields, n_fields);
    if (n_fields > 0 && !dims) return fail(GORSE_ERR_INVALID, "dims is NULL");
    for (int k = 0; k < n_fields; k++)
        if (dims[k] < 1 || dims[k] > fm::kMaxEmbDim)
            return fail(GORSE_ERR_INVALID, "embedding dimension %d of field %d outside 1..%d", dims[k], k, fm::kMaxEmbDim);
    GORSE_HIP_CHECK(hipSetDevice(h->device));
    GORSE_HIP_CHECK(hipStreamSynchronize(h->s));
    for (auto &F : h->fld) {
        for (auto *b : {&F.p, &F.m, &F.v, &F.gpart, &F.h, &F.a}) b->release();
        F.x.release();
        F.have_x = false;
        F.D = 0;
    }
    fm::drop_sample_sets(h);  // they index the catalogue
    h->cat.reset();  // the resident item catalogue holds one table per field of the set that is going away
    h->test.reset();  // and so does the resident test split
    h->n_fields = 0;
    h->dense_blocks = 0;
    std::vector<fm::DenseDesc> descs;
    for (int k = 0; k < n_fields; k++) {
        fm::Field &F = h->fld[k];
        F.D = dims[k];
        const size_t D = (size_t)F.D, d = (size_t)h->d;
        const size_t lens[5] = {d * D, D * d, d, D * d, d};  // H, Wa, ba, We, be
        size_t o = 0;
        for (int t = 0; t < 5; t++) {
            F.off[t] = o;
            F.len[t] = lens[t];
            o += (lens[t] + 3) / 4 * 4;
        }
        F.total = o;
        for (auto *b : {&F.p, &F.m, &F.v}) {
            GORSE_TRY(b->alloc(F.total));
            GORSE_HIP_CHECK(hipMemsetAsync(b->p, 0, F.total * sizeof(float), h->s));
        }
        GORSE_TRY(F.gpart.alloc(F.gstride() * fm::kGradSegs));
        // gradient blocks of one segment: dH | dWa, dba | dWe, dbe
        const size_t goff[5] = {0, lens[0], lens[0] + lens[1], lens[0] + lens[1] + lens[2], lens[0] + 2 * lens[1] + lens[2]};
        for (int t = 0; t < 5; t++) {
            descs.push_back({F.p.p + F.off[t], F.m.p + F.off[t], F.v.p + F.off[t], F.gpart.p + goff[t], (int64_t)lens[t],
                             (int64_t)F.gstride()});
            h->dense_blocks = std::max<int64_t>(h->dense_blocks, ceil_div(ceil_div((int64_t)lens[t], 4), fm::kBlock));
        }
    }
    if (n_fields > 0) {
        GORSE_TRY(h->descs.alloc(descs.size()));
        GORSE_HIP_CHECK(hipMemcpy(h->descs.p, descs.data(), descs.size() * sizeof(fm::DenseDesc), hipMemcpyHostToDevice));
    }
    GORSE_HIP_CHECK(hipStreamSynchronize(h->s));
    h->n_fields = n_fields;
    return GORSE_OK;
}

extern "C" int32_t gorse_fm_set_embedding_params(gorse_fm *h, int32_t field, const float *H, const float *Wa, const float *ba,
                                                 const float *We, const float *be) {
    GORSE_TRY(fm::check_field(h, field));
    if (!H || !Wa || !ba || !We || !be) return fail(GORSE_ERR_INVALID, "H / Wa / ba / We / be is NULL");
    GORSE_HIP_CHECK(hipSetDevice(h->device));
    GORSE_HIP_CHECK(hipStreamSynchronize(h->s));
    fm::Field &F = h->fld[field];
    const float *src[5] = {H, Wa, ba, We, be};
    for (int t = 0; t < 5; t++)
        GORSE_HIP_CHECK(hipMemcpy(F.p.p + F.off[t], src[t], F.len[t] * sizeof(float), hipMemcpyHostToDevice));
    for (auto *b : {&F.m, &F.v}) GORSE_HIP_CHECK(hipMemsetAsync(b->p, 0, F.total * sizeof(float), h->s));
    GORSE_HIP_CHECK(hipStreamSynchronize(h->s));
    return GORSE_OK;
}

extern "C" int32_t gorse_fm_get_embedding_params(gorse_fm *h, int32_t field, float *H, float *Wa, float *ba, float *We, float *be) {
    GORSE_TRY(fm::check_field(h, field));
    GORSE_HIP_CHECK(hipSetDevice(h->device));
    GORSE_HIP_CHECK(hipStreamSynchronize(h->s));
    fm::Field &F = h->fld[field];
    float *dst[5] = {H, Wa, ba, We, be};
    for (int t = 0; t < 5; t++)
        if (dst[t]) GORSE_HIP_CHECK(hipMemcpy(dst[t], F.p.p + F.off[t], F.len[t] * sizeof(float), hipMemcpyDeviceToHost));
    return GORSE_OK;
}

extern "C" int32_t gorse_fm_set_train_embeddings(gorse_fm *h, int32_t field, const uint16_t *emb) {
    GORSE_TRY(fm::check_field(h, field));
    if (h->smp)
        return fail(GORSE_ERR_INVALID, "the training set is in sample form: its embeddings are the item catalogue's (gorse_fm_set_items)");
    if (h->n <= 0) return fail(GORSE_ERR_INVALID, "no training set (gorse_fm_set_train)");
    if (!emb) return fail(GORSE_ERR_INVALID, "emb is NULL");
    fm::Field &F = h->fld[field];
    // n x D is formed in 64 bits everywhere; what bounds it is the device's memory
    if (h->n > INT64_MAX / (int64_t)(F.D * sizeof(uint16_t))) return fail(GORSE_ERR_INVALID, "n x D overflows");
    GORSE_HIP_CHECK(hipSetDevice(h->device));
    GORSE_HIP_CHECK(hipStreamSynchronize(h->s));
    F.have_x = false;
    const size_t ne = (size_t)h->n * (size_t)F.D;
    GORSE_TRY(F.x.alloc(ne));
    GORSE_HIP_CHECK(hipMemcpy(F.x.p, emb, ne * sizeof(uint16_t), hipMemcpyHostToDevice));
    F.have_x = true;
    return GORSE_OK;
}

extern "C" int32_t gorse_fm_epoch(gorse_fm *h, int32_t batch_size, int32_t optimizer, float lr, float wd,
                                  const volatile int32_t *cancel, float *cost_out) {
    if (!h) return fail(GORSE_ERR_INVALID, "handle is NULL");
    if (batch_size <= 0) return fail(GORSE_ERR_INVALID, "batch_size must be positive");
    if (optimizer != GORSE_OPT_SGD && optimizer != GORSE_OPT_ADAM) return fail(GORSE_ERR_INVALID, "unknown optimizer %d", optimizer);
    if (h->n <= 0 && h->smp_dropped)
        return fail(GORSE_ERR_INVALID, "the sample-form training set was dropped when the item catalogue it indexed was replaced or "
                                       "dropped (gorse_fm_set_items, gorse_fm_set_embedding_dims): set it again");
    if (h->n <= 0) return fail(GORSE_ERR_INVALID, "no training set (gorse_fm_set_train)");
    // one loop over two training sources: whichever set was set last
    static const fm::PaddedTrain padded;
    const fm::TrainSource &src = h->smp ? fm::samples_source() : static_cast<const fm::TrainSource &>(padded);
    GORSE_TRY(src.ready(h));
    GORSE_HIP_CHECK(hipSetDevice(h->device));
    int64_t max_slots = 0;
    GORSE_TRY(src.plan(h, batch_size, &max_slots));
    GORSE_TRY(fm::ensure_step(h, batch_size, max_slots));
    if (h->n_fields > 0) GORSE_TRY(fm::ensure_branch(h, std::min<int64_t>(h->n, batch_size), true));
    const float *tgt = src.targets(h);
    GORSE_HIP_CHECK(hipMemsetAsync(h->cost.p, 0, sizeof(float), h->s));
    const int64_t nb = ceil_div(h->n, batch_size);
    const bool adam = optimizer == GORSE_OPT_ADAM;
    fm::OptArgs o{};
    float *ps[3] = {h->V.p, h->W.p, h->B.p}, *ms[3] = {h->mV.p, h->mW.p, h->mB.p}, *vs[3] = {h->vV.p, h->vW.p, h->vB.p};
    const int64_t lens[3] = {h->nf * h->d, h->nf, 1};
    for (int t = 0; t < 3; t++) o.p[t] = ps[t], o.m[t] = ms[t], o.v[t] = vs[t], o.len[t] = lens[t];
    o.blocks0 = ceil_div(ceil_div(lens[0], 4), fm::kBlock);
    o.blocks1 = ceil_div(ceil_div(lens[1], 4), fm::kBlock);
    o.d = h->d;
    o.tag = h->tag.p;
    o.gV = h->gV.p, o.gW = h->gW.p, o.gB = h->gB.p;
    o.wd = wd;
    o.c1 = 1.0f - fm::kBeta1;
    o.c2 = 1.0f - fm::kBeta2;
    const unsigned opt_grid = (unsigned)(o.blocks0 + o.blocks1 + 1);
    for (int64_t k = 0; k < nb; k++) {
        if (k % 64 == 0 && k >= 128) {
            // at most two groups of 64 steps in flight: wait for the end of the group before the previous one
            GORSE_HIP_CHECK(hipEventSynchronize(h->ev[(k / 64) & 1]));
        }
        if (cancel && *cancel) {
            GORSE_HIP_CHECK(hipStreamSynchronize(h->s));
            return fail(GORSE_ERR_CANCELLED, "cancelled");
        }
        const int64_t r0 = k * batch_size, nr = std::min<int64_t>(h->n, r0 + batch_size) - r0;
        const int64_t tag_hi = (h->step + 1) << 32;
        GORSE_TRY(src.forward(h, r0, nr));
        if (h->n_fields > 0) {
            // the branch's contribution joins the logit before loss and g are formed (fm.go:127-132)
            for (int e = 0; e < h->n_fields; e++) GORSE_TRY(src.branch_forward(h, e, r0, nr));
            fm::LossArgs l{};
            l.logit = h->a_logit.p, l.tgt = tgt + r0;
            l.vx = h->vx.p, l.esum = h->a_esum.p;
            l.nrows = nr, l.d = h->d, l.inv_n = 1.0f / (float)nr;
            l.gs = h->gs.p, l.loss = h->loss.p, l.vxe = h->a_vxe.p;
            fm::att_loss_kernel<<<dim3((unsigned)ceil_div(nr * h->d, fm::kBlock)), dim3(fm::kBlock), 0, h->s>>>(l);
            for (int e = 0; e < h->n_fields; e++) {
                GORSE_TRY(src.branch_gx(h, e, r0, nr));
                // reads no embedding: the same launch for either source (x is not dereferenced)
                fm::att_bwd_ds_kernel<<<dim3(fm::row_grid(nr)), dim3(fm::kBlock), 0, h->s>>>(
                    fm::branch_args(h, e, nullptr, nr, h->vx.p, true));
                GORSE_TRY(src.branch_grad(h, e, r0, nr));
            }
        }
        GORSE_TRY(src.accum(h, k, r0, nr, tag_hi));
        o.tag_hi = tag_hi;
        if (adam) {
            h->adam_t++;
            o.lr = fm::adam_lr(lr, h->adam_t);
            fm::fm_opt_kernel<true><<<dim3(opt_grid), dim3(fm::kBlock), 0, h->s>>>(o);
        } else {
            o.lr = lr;
            fm::fm_opt_kernel<false><<<dim3(opt_grid), dim3(fm::kBlock), 0, h->s>>>(o);
        }
        if (h->n_fields > 0) {
            const dim3 dg((unsigned)h->dense_blocks, (unsigned)(5 * h->n_fields));
            if (adam)
                fm::fm_dense_opt_kernel<true><<<dg, dim3(fm::kBlock), 0, h->s>>>(h->descs.p, wd, o.lr, o.c1, o.c2);
            else
                fm::fm_dense_opt_kernel<false><<<dg, dim3(fm::kBlock), 0, h->s>>>(h->descs.p, wd, o.lr, o.c1, o.c2);
        }
        GORSE_HIP_CHECK(hipGetLastError());
        h->step++;
        if (k % 64 == 63) GORSE_HIP_CHECK(hipEventRecord(h->ev[(k / 64) & 1], h->s));
    }
    float cost = 0.0f;
    GORSE_HIP_CHECK(hipMemcpyAsync(&cost, h->cost.p, sizeof(float), hipMemcpyDeviceToHost, h->s));
    GORSE_HIP_CHECK(hipStreamSynchronize(h->s));
    if (cost_out) *cost_out = cost;
    return GORSE_OK;
}

extern "C" int32_t gorse_fm_predict(gorse_fm *h, int64_t n, int32_t width, const int32_t *indices, const float *values,
                                    float *logits_out) {
    if (!h) return fail(GORSE_ERR_INVALID, "handle is NULL");
    if (h->n_fields > 0)
        return fail(GORSE_ERR_INVALID, "the model has embedding fields: score it with gorse_fm_predict_embeddings");
    GORSE_TRY(fm::check_rows(h, n, width, indices, values, false));
    if (n == 0) return GORSE_OK;
    if (!logits_out) return fail(GORSE_ERR_INVALID, "logits_out is NULL");
    GORSE_HIP_CHECK(hipSetDevice(h->device));
    const size_t ne = (size_t)n * width;
    GORSE_TRY(h->p_idx.ensure(ne));
    GORSE_TRY(h->p_val.ensure(ne));
    GORSE_TRY(h->p_out.ensure((size_t)n));
    GORSE_HIP_CHECK(hipMemcpyAsync(h->p_idx.p, indices, ne * 4, hipMemcpyHostToDevice, h->s));
    GORSE_HIP_CHECK(hipMemcpyAsync(h->p_val.p, values, ne * 4, hipMemcpyHostToDevice, h->s));
    fm::FwdArgs<fm::PaddedRows> f{};
    f.src = {h->p_idx.p, h->p_val.p, 0, width};
    f.V = h->V.p, f.W = h->W.p, f.B = h->B.p;
    f.nrows = n, f.d = h->d;
    f.out = h->p_out.p;
    GORSE_TRY(fm::launch_forward<fm::kLogit>(h->s, f));
    GORSE_HIP_CHECK(hipMemcpyAsync(logits_out, h->p_out.p, (size_t)n * 4, hipMemcpyDeviceToHost, h->s));
    GORSE_HIP_CHECK(hipStreamSynchronize(h->s));
    return GORSE_OK;
}

extern "C" int32_t gorse_fm_predict_embeddings(gorse_fm *h, int64_t n, int32_t width, const int32_t *indices, const float *values,
                                               const uint16_t *const *emb, int32_t batch_size, float *logits_out) {
    if (!h) return fail(GORSE_ERR_INVALID, "handle is NULL");
    if (h->n_fields == 0) return gorse_fm_predict(h, n, width, indices, values, logits_out);
    if (batch_size <= 0) return fail(GORSE_ERR_INVALID, "batch_size must be positive");
    GORSE_TRY(fm::check_rows(h, n, width, indices, values, false));
    if (n == 0) return GORSE_OK;
    if (!logits_out) return fail(GORSE_ERR_INVALID, "logits_out is NULL");
    GORSE_TRY(fm::check_emb(h, emb));
    GORSE_HIP_CHECK(hipSetDevice(h->device));
    const int64_t bs = std::min<int64_t>(n, batch_size);
    const size_t ne = (size_t)n * width;
    GORSE_TRY(h->p_idx.ensure(ne));
    GORSE_TRY(h->p_val.ensure(ne));
    GORSE_TRY(h->p_x.ensure((size_t)bs * fm::max_emb_dim(h)));
    GORSE_TRY(h->p_vx.ensure((size_t)bs * h->d));
    GORSE_TRY(fm::ensure_branch(h, bs, false));
    GORSE_HIP_CHECK(hipMemcpyAsync(h->p_idx.p, indices, ne * 4, hipMemcpyHostToDevice, h->s));
    GORSE_HIP_CHECK(hipMemcpyAsync(h->p_val.p, values, ne * 4, hipMemcpyHostToDevice, h->s));
    // BatchInternalPredict's slices (fm.go:168-176): the softmax's indexing makes the slice length part of the result
    for (int64_t r0 = 0; r0 < n; r0 += bs) {
        const int64_t nr = std::min<int64_t>(n, r0 + bs) - r0;
        fm::FwdArgs<fm::PaddedRows> f{};
        f.src = {h->p_idx.p, h->p_val.p, r0, width};
        f.V = h->V.p, f.W = h->W.p, f.B = h->B.p;
        f.nrows = nr, f.d = h->d;
        f.out = h->a_logit.p, f.vx = h->p_vx.p;
        GORSE_TRY(fm::launch_forward<fm::kLogitVx>(h->s, f));
        for (int k = 0; k < h->n_fields; k++) {
            const int64_t D = h->fld[k].D;
            GORSE_HIP_CHECK(hipMemcpyAsync(h->p_x.p, emb[k] + r0 * D, (size_t)(nr * D) * sizeof(uint16_t), hipMemcpyHostToDevice, h->s));
            GORSE_TRY(fm::branch_forward(h->s, fm::branch_args(h, k, h->p_x.p, nr, h->p_vx.p, false), fm::BatchRows{}));
        }
        GORSE_HIP_CHECK(hipMemcpyAsync(logits_out + r0, h->a_logit.p, (size_t)nr * 4, hipMemcpyDeviceToHost, h->s));
    }
    GORSE_HIP_CHECK(hipStreamSynchronize(h->s));
    return GORSE_OK;
}
