// bpr_update.hip -- the per-sample BPR update on gfx950.  Reference: model/cf/model.go:469-488.
//   bpr_update_kernel      : the per-sample form (one group per sample, three rows updated in place): the
//                            sequential parity schedule, the racy diagnostic, and the Hogwild schedule of shapes
//                            with few users or another factor width.
//   bpr_fold_kernel        : after a Hogwild launch with folders, what is left in the replica and accumulator rows -> Q.
// The folders of the launch itself are bpr_fold.hpp's (run_folders<false>); the launch's grid, folder count and LDS are bpr_plan.hpp's.
// The user-run form is bpr_update_users.hip.
#include "bpr_internal.hpp"

using namespace gorse;

namespace {

// row[e] <- fma(t, lr, snapshot) in the flavour of MODE
template <int MODE>
__device__ __forceinline__ void apply(float *p, float snap, float t, float lr, bool fused) {
    if constexpr (MODE == MODE_ATOMIC) {
        (void)snap;
        (void)fused;
        __hip_atomic_fetch_add(p, t * lr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
        float r = fused ? fmaf(t, lr, snap) : t * lr + snap;
        if constexpr (MODE == MODE_EXACT)
            *p = r;
        else  // write-through (sc1) store: visible to the other XCDs' L2s, like a CPU store
            __hip_atomic_store(p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// one element of the three updates of model.go:473-488 (operation order of SURVEY.md A2)
template <int MODE>
__device__ __forceinline__ void update_elem(float *pu, float *qi, float *qj, int e, float p, float a, float b, float grad,
                                            float nreg, float lr, bool fused, bool same_item) {
    float t1 = p * grad;
    t1 = fused ? fmaf(a, nreg, t1) : a * nreg + t1;
    float t2 = p * (-grad);
    t2 = fused ? fmaf(b, nreg, t2) : b * nreg + t2;
    float t3 = a - b;
    t3 = t3 * grad;
    t3 = fused ? fmaf(p, nreg, t3) : p * nreg + t3;
    if constexpr (MODE == MODE_EXACT) {
        float qi_new = fused ? fmaf(t1, lr, a) : t1 * lr + a;
        qi[e] = qi_new;
        // i == j cannot come out of the sampler; a hand-made stream applies both updates in order
        float base = same_item ? qi_new : b;
        qj[e] = fused ? fmaf(t2, lr, base) : t2 * lr + base;
        pu[e] = fused ? fmaf(t3, lr, p) : t3 * lr + p;
    } else {
        apply<MODE>(qi + e, a, t1, lr, fused);
        apply<MODE>(qj + e, b, t2, lr, fused);
        apply<MODE>(pu + e, p, t3, lr, fused);
    }
}

template <int NC, int MODE>
__global__ __launch_bounds__(kBlock) void bpr_update_kernel(float *P, float *Q, const int32_t *__restrict__ us,
                                                            const int32_t *__restrict__ is,
                                                            const int32_t *__restrict__ js,
                                                            const int32_t *__restrict__ order, int64_t begin,
                                                            int64_t end, int d, float lr, float reg, int exp_mode,
                                                            double *loss, HotRows hot, int folders) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    if (MODE == MODE_ATOMIC && (int)blockIdx.x < folders) {
        run_folders<false>(hot, Q, folders);
        return;
    }
    const int lane = threadIdx.x & (kGroup - 1);
    const int gib = threadIdx.x / kGroup;
    const int64_t group = (int64_t)((int)blockIdx.x - folders) * kGroupsPerBlock + gib;
    const int64_t ngroups = (int64_t)((int)gridDim.x - folders) * kGroupsPerBlock;
    const VecShape vs(d);
    const float nreg = -reg;
    double my_loss = 0.0;
    for (int64_t s = begin + group; s < end; s += ngroups) {
        const int64_t t = order ? (int64_t)order[s] : s;
        const int u = us[t], i = is[t], j = js[t];
        if ((u | i | j) < 0) continue;
        float *pu = P + (int64_t)u * d, *qi = Q + (int64_t)i * d, *qj = Q + (int64_t)j * d;
        float *qiw = qi;  // where the positive item's update lands
        if (MODE == MODE_ATOMIC && folders > 0) {  // (a launch has folders where it has rows that take an item's updates: open_hot)
            const int32_t code = hot.slot[i];
            if (code >= 0) qiw = hot_row(hot, code, group);
        }
        if constexpr (NC > 0) {
            float p[NC], a[NC], b[NC];
#pragma unroll
            for (int c = 0; c < NC; c++) {
                p[c] = load_row<MODE>(pu + 16 * c + lane);
                a[c] = load_row<MODE>(qi + 16 * c + lane);
                b[c] = load_row<MODE>(qj + 16 * c + lane);
            }
            const float diff = dot512_regs<NC>(p, a) - dot512_regs<NC>(p, b);
            const float ex = bpr_exp(-diff, exp_mode);
            const float grad = ex / (1.0f + ex);
            if (loss && lane == 0) my_loss += (double)log1pf(ex);
#pragma unroll
            for (int c = 0; c < NC; c++)
                update_elem<MODE>(pu, qiw, qj, 16 * c + lane, p[c], a[c], b[c], grad, nreg, lr, true, i == j);
        } else {
            float *sp = smem + (size_t)gib * 3 * d, *sa = sp + d, *sb = sa + d;
            for (int e = lane; e < d; e += kGroup) {
                sp[e] = load_row<MODE>(pu + e);
                sa[e] = load_row<MODE>(qi + e);
                sb[e] = load_row<MODE>(qj + e);
            }
            __builtin_amdgcn_wave_barrier();
            const float diff = dot512_lds(sp, sa, vs, lane) - dot512_lds(sp, sb, vs, lane);
            const float ex = bpr_exp(-diff, exp_mode);
            const float grad = ex / (1.0f + ex);
            if (loss && lane == 0) my_loss += (double)log1pf(ex);
            for (int e = lane; e < d; e += kGroup)
                update_elem<MODE>(pu, qiw, qj, e, sp[e], sa[e], sb[e], grad, nreg, lr, !vs.unfused(e), i == j);
            __builtin_amdgcn_wave_barrier();
        }
    }
    if (loss && lane == 0 && my_loss != 0.0) atomicAdd(loss, my_loss);
    if (MODE == MODE_ATOMIC && folders > 0) worker_done<false>(hot);
}

// after a per-sample update launch: Q[item] += the sum of its replicas, replicas <- 0 (nothing else runs on the stream); the slots
// of both tiers
__global__ __launch_bounds__(256) void bpr_fold_kernel(HotRows hot, float *Q) {
    const int d = hot.d;
    const int64_t work = (int64_t)(hot.n_hot + hot.n_acc) * d;
    for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < work; w += (int64_t)gridDim.x * blockDim.x) {
        const int64_t slot = w / d;
        const int e = (int)(w - slot * d);
        const int32_t code = hot.meta[slot];
        float *r0 = hot.rep + hot_base(code) * d + e;
        float sum = 0.0f;
        for (int r = 0; r < (1 << hot_lg(code)); r++) {
            sum += r0[(int64_t)r * d];
            r0[(int64_t)r * d] = 0.0f;
        }
        if (sum != 0.0f) Q[(int64_t)hot.items[slot] * d + e] += sum;
    }
}

template <int MODE>
int32_t launch_update_mode(gorse_mf *h, const int32_t *us, const int32_t *is, const int32_t *js, const int32_t *order,
                           int64_t begin, int64_t end, float lr, float reg, int exp_mode, double *loss,
                           hipStream_t st, hipEvent_t start, hipEvent_t stop) {
    const int64_t n = end - begin;
    if (n <= 0) return GORSE_OK;
    const int d = h->d;
    int64_t blocks = bpr_sample_workers(n);
    HotRows hot = make_hot(h);
    const int folders = bpr_sample_folders(MODE, h->n_hot, h->n_acc) > 0 ? open_hot(h, hot) : 0;
    if (folders > 0) h->fold_sole_last = 0;  // (the per-sample kernel's fold is the atomic one, then bpr_fold_kernel)
    blocks += folders;
    dim3 grid((unsigned)blocks), block(kBlock);
    const size_t lds = bpr_sample_lds_bytes(d);
#define LAUNCH(NC)                                                                                                  \
    hipExtLaunchKernelGGL((bpr_update_kernel<NC, MODE>), grid, block, lds, st, start, folders > 0 ? nullptr : stop, 0, h->P.p, \
                          h->Q.p, us, is, js, order, begin, end, d, lr, reg, exp_mode, loss, hot, folders)
    switch (bpr_sample_chunks(d)) {
    case 1: LAUNCH(1); break;
    case 2: LAUNCH(2); break;
    case 4: LAUNCH(4); break;
    case 8: LAUNCH(8); break;
    default: LAUNCH(0); break;
    }
#undef LAUNCH
    GORSE_HIP_CHECK(hipGetLastError());
    if (folders > 0) {  // (its folders make no last pass: worker_done); the launch's stop event is this kernel's
        const int64_t fb = bpr_fold_grid(hot.n_hot, hot.n_acc, d);
        hipExtLaunchKernelGGL(bpr_fold_kernel, dim3((unsigned)fb), dim3(kFoldThreads), 0, st, nullptr, stop, 0, hot, h->Q.p);
        GORSE_HIP_CHECK(hipGetLastError());
    }
    return GORSE_OK;
}

}  // namespace

int32_t gorse::bpr_launch_update(gorse_mf *h, int mode, const int32_t *us, const int32_t *is, const int32_t *js,
                                 const int32_t *order, int64_t begin, int64_t end, float lr, float reg, int exp_mode, double *loss,
                                 hipStream_t st, hipEvent_t start, hipEvent_t stop) {
    switch (mode) {
    case MODE_ATOMIC:
        return launch_update_mode<MODE_ATOMIC>(h, us, is, js, order, begin, end, lr, reg, exp_mode, loss, st, start, stop);
    case MODE_EXACT:
        return launch_update_mode<MODE_EXACT>(h, us, is, js, order, begin, end, lr, reg, exp_mode, loss, st, start, stop);
    case MODE_RACY:
        return launch_update_mode<MODE_RACY>(h, us, is, js, order, begin, end, lr, reg, exp_mode, loss, st, start, stop);
    }
    return fail(GORSE_ERR_INVALID, "unknown BPR mode %d", mode);
}
