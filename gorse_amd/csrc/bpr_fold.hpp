// bpr_fold.hpp -- the hot-row replicas and the accumulated tier of the Hogwild BPR update launches, and the FOLDER workgroups that drain
// them into Q: HotRows (the launch argument), the fold constants, the arrival counter of the workers and the folds themselves (atomic
// and sole-writer).  A device header: the library is built without relocatable device code, so what the kernels of two units call
// lives here -- bpr_update.hip (bpr_update_kernel: run_folders<false>, then bpr_fold_kernel) and bpr_update_users.hip
// (bpr_update_user_kernel: run_folders<true>) both include it.  The host rules (folder counts, which launch folds as sole writer) are
// bpr_plan.hpp's; who owns which element of which slot is hot_rows.hpp's.
#pragma once
#include "bpr_plan.hpp"
#include "mf_internal.hpp"

namespace gorse {

// Hot-row replicas (GORSE_BPR_HOGWILD_ATOMIC only).  Device-scope atomics and L1-bypassing loads are
// served memory-side, line by line, in order: a row that a popularity-skewed epoch keeps hitting builds a
// deep atomic queue, and every gather of that row -- and the retirement of every wave that updated it --
// waits in it (measured: positive-item atomics redirected away from the rows being read = 2.0x, spread
// over 8 rows each = 2.7x on S-ml1m; profiles/r01_b_probe_rep.txt).  So the positive-item update of a HOT
// item (share of the training feedback >= 1/8192, chosen at create time) -- and, in the user-run schedule, the update of a
// hot item drawn as the NEGATIVE -- lands in one of the item's R_s private rows picked by the group id (R_s = 1 .. kHotReplicas by the
// item's expected update rate, gorse_mf_create / hot_rows.hpp), and FOLDER workgroups of the same launch drain the replicas into the
// real rows with one combined atomic per element and pass, one pass per fold period of the device's constant-rate clock.  Q stays the
// only source of truth for every reader; a hot row's update becomes visible one folder pass (a fold period) late, the same order as the
// latency of the atomics themselves.  Once every worker workgroup has finished, the folders make a last pass: the launch leaves every
// replica zero and Q complete, so nothing outside the BPR update units ever sees them.
// The ACCUMULATED tier (hot_rows.hpp acc_rows_layout; handles whose whole Q fits one XCD's L2): every WARM item has one accumulator
// row behind the replica rows, and its hot_slot word is that row's code -- to the workers it is a hot item with one replica, so on
// such a handle no worker atomic lands on a row that anybody gathers (atomics onto rows under agent-scope loads run at 241 G dwords/s
// on a table of that size, onto rows nobody reads at 311: profiles/r04_s_probe_atomics3.txt).  The tier's slots follow the hot ones in
// items / meta (n_hot .. n_hot + n_acc) and have folder workgroups of their own, kFolderBlocksAcc of them behind the hot tier's, which
// pass every kDefaultAccFoldEvery-th fold period; the hot tier's folders and their period are what they are without the tier.  In the last
// pass all folder workgroups share the rows of both tiers.  That is the ATOMIC fold: the per-sample kernel's, a handle's without the
// tier, a launch's with the store route open.  A user-run launch on a handle with the tier and the store route closed has no worker
// that writes Q and folds in the SOLE-WRITER form (below kFolderTimeout): loads and stores instead of the exchange and the add.
// (kFolderBlocks, kFolderBlocksAcc: bpr_plan.hpp, where the launches' folder count is)
constexpr int kHotReplicas = GORSE_HOT_REPLICAS;
// Fold periods between two passes of the tier's folders.  A warm item takes at most 1/8192 + 1/I of the updates (3.9e-4 at C2), the
// hottest item 1.5e-2 and is folded every period: at 4 a warm row's window holds 3.9e-4 x 4 / 1.5e-2 ~ 1/10 of the stale updates the
// hottest item's window holds, and at nFactors 16 about 50 where the 32 us window that diverged (kDefaultFoldPeriod below) held ~1800.
// Swept on C2 (profiles/bpr_acc_rows_sweep.txt): 2 / 4 / 8 -> 0.393 / 0.389 / 0.384 ms per epoch at nFactors 64, 0.202 / 0.202 / 0.201
// at 16; NDCG@10 after 30 epochs stays within 0.006 of the sequential oracle at 2 and 4 and leaves the +-0.01 bar at 8 (nFactors 8, 16).
constexpr int kDefaultAccFoldEvery = 4;
// Wall-clock ticks (100 MHz) from the start of one folder pass to the next: how late a hot row's update reaches Q.  Swept on C2
// (profiles/r07_hr_sweep_replica_unit.txt, replica unit 0.001): 8 / 16 / 32 us -> 0.545 / 0.544 / 0.538 ms per epoch at nFactors 64,
// 0.295 / 0.293 ms at 16 -- where 32 us DIVERGED (non-finite factors within 23 epochs, three handles of three): the hottest item takes
// ~1.5 % of the updates, and at the small widths' sample rate a 32 us window holds ~1800 of them computed from one stale row.  8 us
// keeps a factor of four from that; it costs nothing measurable at nFactors 64.
constexpr uint32_t kDefaultFoldPeriod = 800;
// folders that have waited this long (10 s) for the workers stop waiting (a launch of the largest chunk takes ~0.13 s): a last pass
// while workers still run leaves some updates in the replicas, where the next launch's folders find them -- never a hung device
constexpr uint64_t kFolderTimeout = 1000000000ull;
// The SOLE-WRITER fold.  On a handle with the accumulated tier every item has a row, so in a user-run launch without the store route
// no worker instruction writes Q: the folders are the only writers of the Q rows they fold, and their atomics -- an exchange per row
// and an add onto Q per pass, the add the only atomic of the launch that lands on rows the workers gather -- are not needed.  Such a
// launch (launch_update_users decides: HotRows::sole) folds with loads and stores instead.  At its start every folder thread copies
// the Q elements it owns into `base` (a table of (n_hot + n_acc) x d floats of the handle's, private to the update launch); a periodic pass
// LOADS the slot's rows and stores Q <- base + their sum -- nothing is zeroed, the rows grow for the length of the launch -- and the
// last pass exchanges the rows with zero and stores Q <- base + the sum of what it took.  The exchange stays there on purpose: it
// leaves every row zero without a race, and after a last pass made while workers still run (the timeout) whatever lands behind it
// stays in the row, where the next launch -- which starts from base = Q -- finds it.  What makes the stores safe is ownership: every
// (slot, element group) belongs to ONE thread for the whole launch, periodic and last pass alike (hot_rows.hpp fold_share), so no
// workgroup still in a periodic pass can overwrite another's final value.  Q = base + (the launch's updates of the row) is one of the
// associations a Hogwild launch produces anyway, and with one update per row the bits of the atomic form.  Every other launch -- a
// handle without the tier, the store route, the per-sample kernel -- keeps the atomic fold below.
// The only unit whose code depends on the macro is bpr_update_users.hip (the per-sample kernel's folders never make a last pass):
// make ab AB=fold_atomic AB_SRC=bpr_update_users AB_FLAGS=-DGORSE_BPR_FOLD_SOLE_WRITER=0
#ifndef GORSE_BPR_FOLD_SOLE_WRITER
#define GORSE_BPR_FOLD_SOLE_WRITER 1  // A/B: 0 = every launch folds with atomics
#endif

struct HotRows {
    const int32_t *slot;   // I entries: class of an item -- hot_code(first replica row, log2 R_s) of a HOT item, hot_code(its row, 0)
                           // of an item of the accumulated tier, -1 warm, -2 cold
    const int32_t *items;  // n_hot + n_acc entries: item of a slot (the hot slots first)
    const int32_t *meta;   // n_hot + n_acc entries: hot_code of a slot
    float *rep;            // replica rows, then the tier's rows, of d floats: all zero outside an update launch
    int32_t *done;         // two sets of arrival stripes (worker workgroups that have finished) + the folders' pass count
    int n_hot;
    int d;
    int set;               // the set of stripes this launch counts in (launch parity: the launch zeroes the other one for the next)
    uint32_t period;       // wall-clock ticks between two folder passes
    int n_acc;             // slots of the accumulated tier (0: the handle has none)
    int acc_every;         // fold periods between two passes of the tier's folders
    float *base;           // n_hot + n_acc rows of d floats: Q's rows of the slots as the launch found them (the sole-writer fold)
    int sole;              // the launch folds as Q's sole writer (launch_update_users)
    uint64_t timeout;      // wall-clock ticks after which the folders stop waiting for the workers
};

// a group of the sole-writer fold (kFoldGroup = 2 floats, 8-byte aligned: d and the element are even): agent-scope load, store and
// exchange with zero, the flavours the gathers and the cold-store route use across XCDs; the exchange per element, so that it meets
// the workers' fp32 adds as the atomic fold's does
static_assert(kFoldGroup == 2 && kFolderThreads == kBlock, "the sole-writer fold moves float pairs, one per thread of an update workgroup");
__device__ __forceinline__ float2 load_pair(const float *p) {
    const unsigned long long x = __hip_atomic_load((const unsigned long long *)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return make_float2(__uint_as_float((unsigned)x), __uint_as_float((unsigned)(x >> 32)));
}
__device__ __forceinline__ void store_pair(float *p, float2 v) {
    __hip_atomic_store((unsigned long long *)p, (unsigned long long)__float_as_uint(v.x) | ((unsigned long long)__float_as_uint(v.y) << 32),
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ float2 drain_pair(float *p) {
    const float x = __hip_atomic_exchange(p, 0.0f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const float y = __hip_atomic_exchange(p + 1, 0.0f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return make_float2(x, y);
}

// the replica row that group `group` adds a hot item's update to (code: the item's hot_slot word)
__device__ __forceinline__ float *hot_row(const HotRows &hot, int32_t code, int64_t group) {
    return hot.rep + (hot_base(code) + (group & ((1 << hot_lg(code)) - 1))) * hot.d;
}

// The arrival counter of the worker workgroups, in kDoneStripes words 256 bytes apart: one 64-byte line serves 88 M atomics/s
// (scripts/probe_atomics4.hip), and the per-sample kernel's 4096 workgroups, which all finish within a few microseconds of each other,
// queued 46 us on a single word at the end of every launch (S-ml100k: a third of the kernel).
constexpr int kDoneStripes = GORSE_HOT_DONE_STRIPES, kDoneStride = GORSE_HOT_DONE_STRIDE;
constexpr int kFoldPassesWord = 2 * kDoneStripes * kDoneStride;  // hot.done[]: the last launch's folder passes (gorse_hip_test_bpr_fold_stats)
__device__ __forceinline__ int32_t *done_set(const HotRows &hot, int set) { return hot.done + set * kDoneStripes * kDoneStride; }
// The end of a worker workgroup (every thread calls it).  LAST: the launch's folders make the last pass themselves, once every worker
// is counted -- so the workgroup's atomics on the replicas are performed, and released at agent scope, before it is counted.  Without
// LAST (the per-sample kernel: bpr_fold_kernel follows its launch) the count only ends the folders' passes and needs no order; there a
// release in each of the up to 4096 short-lived workgroups cost more than the fold kernel it saves (S-ml100k: update kernel 52 -> 126
// us, and the sampler beside it 56 -> 124 us: each agent-scope release writes back the XCD's L2, which the sampler's stores fill;
// profiles/r07_hr_full_ab.txt, session A).
template <bool LAST>
__device__ __forceinline__ void worker_done(const HotRows &hot) {
    if constexpr (LAST) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        if constexpr (LAST) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __hip_atomic_fetch_add(done_set(hot, hot.set) + (blockIdx.x & (kDoneStripes - 1)) * kDoneStride, 1, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
    }
}
__device__ __forceinline__ bool workers_done(const HotRows &hot, int workers) {  // (called by whole waves)
    const int lane = threadIdx.x & 63;
    const int32_t *c = done_set(hot, hot.set);
    int v = lane < kDoneStripes ? __hip_atomic_load(c + lane * kDoneStride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v >= workers;
}

// one folder pass: (slot, element) pairs strided over the folder threads; each exchanges the slot's R_s rows and adds their sum once
// (slots [s0, s1): the hot tier's are [0, n_hot))
__device__ __forceinline__ void fold_pass(const HotRows &hot, float *Q, int s0, int s1, int64_t tid, int64_t nthreads) {
    const int d = hot.d;
    const int64_t work = (int64_t)(s1 - s0) * d;
    for (int64_t w = tid; w < work; w += nthreads) {
        const int64_t slot = s0 + w / d;
        const int e = (int)(w - (slot - s0) * d);
        const int32_t code = hot.meta[slot];
        const int nr = 1 << hot_lg(code);
        float *r0 = hot.rep + hot_base(code) * d + e;
        float v[kHotReplicas];
#pragma unroll
        for (int r = 0; r < kHotReplicas; r++)
            v[r] = r < nr ? __hip_atomic_exchange(r0 + (int64_t)r * d, 0.0f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0f;
        float sum = 0.0f;
#pragma unroll
        for (int r = 0; r < kHotReplicas; r++) sum += v[r];
        if (sum != 0.0f)
            __hip_atomic_fetch_add(Q + (int64_t)hot.items[slot] * d + e, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// one pass over slots [s0, s1) of the accumulated tier (one row each): kAccBatch exchanges of a thread are in flight before the first
// add that depends on one -- the tier's pass is a few times the hot tier's, and a chain of exchange -> add round trips per pair is
// what its last pass, at the end of the launch, cannot afford
constexpr int kAccBatch = 4;
__device__ __forceinline__ void fold_acc_pass(const HotRows &hot, float *Q, int s0, int s1, int tid, int nthreads) {
    const int d = hot.d;
    const int work = (s1 - s0) * d;  // (at most 4 MiB / 4 pairs: hot_rows.hpp kAccTableBytes)
    for (int wb = tid; wb < work; wb += kAccBatch * nthreads) {
        float v[kAccBatch];
        float *q[kAccBatch];
#pragma unroll
        for (int b = 0; b < kAccBatch; b++) {
            const int w = wb + b * nthreads;
            v[b] = 0.0f;
            q[b] = Q;
            if (w < work) {
                const int slot = s0 + w / d;
                const int e = w - (slot - s0) * d;
                q[b] = Q + (int64_t)hot.items[slot] * d + e;
                v[b] = __hip_atomic_exchange(hot.rep + hot_base(hot.meta[slot]) * d + e, 0.0f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
#pragma unroll
        for (int b = 0; b < kAccBatch; b++)
            if (v[b] != 0.0f) __hip_atomic_fetch_add(q[b], v[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// The sole-writer fold (above HotRows).  sh: this thread's share of its tier (hot_rows.hpp fold_share).
// launch start: base <- Q for the groups this thread owns -- nobody else writes these elements of Q during the launch
__device__ __forceinline__ void fold_sole_begin(const HotRows &hot, const float *Q, const FoldShare &sh) {
    const int d = hot.d, groups = fold_groups(sh, d);
    for (int g = sh.tid; g < groups; g += sh.nthreads) {
        const int slot = fold_group_slot(sh, g, d), e = fold_group_elem(g, d);
        *(float2 *)(hot.base + (int64_t)slot * d + e) = load_pair(Q + (int64_t)hot.items[slot] * d + e);
    }
}
// one pass over the groups this thread owns: Q <- base + the sum of the slot's rows (at most ROWS of them: kHotReplicas in the hot
// tier, 1 in the accumulated tier), the rows loaded in a periodic pass and exchanged with zero in the LAST.  BATCH groups a time, their
// rows kFoldRowsAtOnce a time: all those loads or exchanges are in flight before the first instruction that depends on one.  Two
// pairs in either tier: with more, the folders and not the workers set the register count of the nFactors 8 / 16 kernels (64 -> 72
// VGPRs at 4 pairs of the accumulated tier), which is the workers' occupancy on every handle.
constexpr int kFoldRowsAtOnce = 2;
template <bool LAST, int ROWS, int BATCH>
__device__ __forceinline__ void fold_sole_pass(const HotRows &hot, float *Q, const FoldShare &sh) {
    constexpr int RC = ROWS < kFoldRowsAtOnce ? ROWS : kFoldRowsAtOnce;
    const int d = hot.d, groups = fold_groups(sh, d);
    for (int gb = sh.tid; gb < groups; gb += BATCH * sh.nthreads) {
        float2 sum[BATCH];
        int at[BATCH];  // slot * d + element of the group, < 0 = none
#pragma unroll
        for (int b = 0; b < BATCH; b++) {
            const int g = gb + b * sh.nthreads;
            at[b] = g < groups ? fold_group_slot(sh, g, d) * d + fold_group_elem(g, d) : -1;
            sum[b] = make_float2(0.0f, 0.0f);
        }
#pragma unroll
        for (int rc = 0; rc < ROWS; rc += RC) {
            float2 v[BATCH][RC];
#pragma unroll
            for (int b = 0; b < BATCH; b++) {
#pragma unroll
                for (int r = 0; r < RC; r++) v[b][r] = make_float2(0.0f, 0.0f);
                if (at[b] >= 0) {
                    const int32_t code = hot.meta[at[b] / d];
                    const int nr = 1 << hot_lg(code);
                    float *r0 = hot.rep + hot_base(code) * d + at[b] % d;
#pragma unroll
                    for (int r = 0; r < RC; r++)
                        if (rc + r < nr) v[b][r] = LAST ? drain_pair(r0 + (int64_t)(rc + r) * d) : load_pair(r0 + (int64_t)(rc + r) * d);
                }
            }
#pragma unroll
            for (int b = 0; b < BATCH; b++)
#pragma unroll
                for (int r = 0; r < RC; r++) sum[b].x += v[b][r].x, sum[b].y += v[b][r].y;  // (row after row, as the atomic fold sums)
        }
#pragma unroll
        for (int b = 0; b < BATCH; b++)
            if (at[b] >= 0) {
                const float2 base = *(const float2 *)(hot.base + at[b]);
                // (a select, not a skipped store: an element nothing was added to keeps its bits, a -0.0 included)
                store_pair(Q + (int64_t)hot.items[at[b] / d] * d + at[b] % d,
                           make_float2(sum[b].x != 0.0f ? base.x + sum[b].x : base.x, sum[b].y != 0.0f ? base.y + sum[b].y : base.y));
            }
    }
}

// The folder workgroups (blockIdx.x < folders) of an update launch: the hot tier's kFolderBlocks first, then -- on a handle with the
// accumulated tier -- the tier's own.  Wave 0 polls the workers' arrival count at the grain of one load round trip and decides for the
// workgroup: a pass over its tier when its period has run out (the hot tier's: the fold period; the accumulated tier's: acc_every of
// them), and once every worker has finished, with LAST, the last pass (an agent-scope acquire behind the count the workers released
// into), in which all folder workgroups share the rows of both tiers.  So the end of the launch never waits for a folder's sleep, and
// with LAST no fold kernel follows the launch.  Both kinds wait in the same loop, under the same bound (kFolderTimeout).
// A launch in the sole-writer form (hot.sole, above HotRows) waits and decides in the same way and differs in what a pass does: every
// thread works on its own share of its own tier's slots in every pass, the last included -- each workgroup decides for itself when
// its last pass begins, so a row shared out differently in that pass could be stored final by one workgroup and stale by another.
template <bool LAST>
__device__ void run_folders(const HotRows &hot, float *Q, int folders) {
    __shared__ int go;
    const int workers = (int)gridDim.x - folders;
    const int hotf = folders < kFolderBlocks ? folders : kFolderBlocks;  // the hot tier's workgroups
    const bool acc = (int)blockIdx.x >= hotf;                            // this workgroup serves the accumulated tier
    const int n_all = hot.n_hot + hot.n_acc;
    const uint64_t period = acc ? (uint64_t)hot.period * (uint64_t)hot.acc_every : hot.period;
    if (blockIdx.x == 0 && threadIdx.x < kDoneStripes)  // the stripes the launch before this one counted in: zero for the next launch
        __hip_atomic_store(done_set(hot, hot.set ^ 1) + threadIdx.x * kDoneStride, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // the sole-writer form: this thread's share of its tier's slots, the same in every pass of the launch; base <- Q first
    bool sole = false;
    FoldShare sh{};
    if constexpr (LAST && GORSE_BPR_FOLD_SOLE_WRITER) {
        sole = hot.sole != 0;
        sh = fold_share((int)blockIdx.x, (int)threadIdx.x, hot.n_hot, hot.n_acc, folders, kFolderBlocks);
        if (sole) fold_sole_begin(hot, Q, sh);
    }
    const uint64_t t0 = wall_clock64();
    uint64_t next = t0 + period;
    int passes = 0;
    for (;;) {
        if (threadIdx.x < 64) {
            const bool all = workers_done(hot, workers);
            if (threadIdx.x == 0) {
                const uint64_t now = wall_clock64();
                int g = 0;
                if (all || now - t0 > hot.timeout) {
                    if constexpr (LAST) {
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    }
                    g = 2;
                } else if (now >= next) {
                    next = now + period;
                    g = 1;
                }
                go = g;
            }
        }
        __syncthreads();
        const int g = go;
        __syncthreads();
        if (g == 0) continue;
        if (g == 2 && !LAST) break;
        // a periodic pass (g == 1): this workgroup's tier among the workgroups of its kind; the last pass (g == 2): both tiers among all
        const bool last = g == 2;
        if (sole) {  // both passes over this thread's own share: hot tier one group a time, the other tier two
            if constexpr (LAST && GORSE_BPR_FOLD_SOLE_WRITER) {
                if (!acc) {
                    if (last)
                        fold_sole_pass<true, kHotReplicas, 1>(hot, Q, sh);
                    else
                        fold_sole_pass<false, kHotReplicas, 1>(hot, Q, sh);
                } else {
                    if (last)
                        fold_sole_pass<true, 1, 2>(hot, Q, sh);
                    else
                        fold_sole_pass<false, 1, 2>(hot, Q, sh);
                }
            }
        } else {
            const int first = last || !acc ? 0 : hotf, among = last ? folders : (acc ? folders - hotf : hotf);
            const int tid = ((int)blockIdx.x - first) * (int)blockDim.x + (int)threadIdx.x, nthreads = among * (int)blockDim.x;
            if (last || !acc) fold_pass(hot, Q, 0, hot.n_hot, tid, nthreads);
            if (last || acc) fold_acc_pass(hot, Q, hot.n_hot, n_all, tid, nthreads);
        }
        passes++;
        if (last) break;
    }
    // the pass counts of the launch (gorse_hip_test_bpr_fold_stats): the hot tier's first workgroup and the accumulated tier's first
    if (threadIdx.x == 0 && ((int)blockIdx.x == 0 || (int)blockIdx.x == hotf)) hot.done[kFoldPassesWord + (acc ? 1 : 0)] = passes;
}

}  // namespace gorse
