// topk_sweep.hip -- the candidate sweep of path B of the exact top-k (topk_mfma.hip says what the path is and why it is exact):
// the kernel, its list compaction and its dispatch by operand depth, epilogue and form (main / pilot, history, symmetric).
//
// The reference scores all N vectors per query one pair at a time.  Here the N x nq score matrix is produced
// by v_mfma_f32_32x32x16_bf16 tiles and never leaves the CU: every wave keeps the operands of its 32*NCB queries
// in registers for the whole sweep, candidate rows stream through LDS, and the epilogue only compares the 16
// scores a lane holds (all of ONE query: the C layout puts a query per column) against that query's running
// filter threshold.  Scores that pass are appended to a small per-query candidate list in HBM; when a list
// fills, its wave raises the threshold to (K-th best approximate score so far) - margin and compacts the list.
// The launch geometry (waves, LDS-DMA or register staging, tile buffers, LDS bytes) is topk_plan.hpp's.
#include "topk_mfma_internal.hpp"

using namespace gorse;

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// One wave raises the filter threshold of local query ql and compacts its list.
// HIST: the entries the new threshold drops are appended to the query's history (hb, counter s_hc[ql]) instead of
// being forgotten; list + history then hold every vector the reference's heap can have accepted.
// SYM: the list holds only the rows of the workgroup's OWN part of the sweep (the rest of the query's candidates are in its
// foreign list), so what it proves about the warm start is one-sided: a K-th-best bound that clears the threshold verifies it
// (the own rows are a subset of all rows) and raises it; one that does not proves nothing -- the warm start is then verified over
// both lists by topk_rescore_kernel, which learns from the final threshold (f_out) whether the sweep ever raised it.
template <bool HIST, bool SYM = false>
__device__ __forceinline__ void compact_query(uint2 *qb, int ql, int kth, int *s_cnt, float *s_f, const float *s_mg,
                                              uint8_t *flag, uint2 *hb = nullptr, int *s_hc = nullptr, bool trust = false) {
    const int lane = threadIdx.x & 63;
    // the list is two interleaved sub-lists: even slots belong to the lane holding rows 0-3, 8-11, ... of the query's
    // column (lane < 32), odd slots to its partner (lane >= 32); each appends at its own counter (slot 2 * c + half)
    const int n_lo = s_cnt[2 * ql], n_hi = s_cnt[2 * ql + 1];
    const int n = n_lo + n_hi;
    // The list is re-read by loads the compiler does not see (one asm statement: the wave's appends drained to L2, eight
    // L1-bypassing loads, their wait).  A load hipcc can see inside the tile loop makes its wait-count pass put
    // s_waitcnt vmcnt(0) at the head of every iteration (the load may be pending along the back edge), and that drains the
    // tiles the LDS-DMA has in flight.  All kCap slots are allocated, so the loads need no predicate; slots past the
    // sub-lists' lengths are masked below (key 0 = never counted: trial >= 1).
    static_assert(kEPL == 8, "compact_query loads eight entries per lane");
    unsigned long long ev[kEPL];
    {
        const uint2 *src = qb + lane;
        asm volatile("s_waitcnt vmcnt(0)\n\t"
                     "global_load_dwordx2 %0, %8, off sc1\n\t"
                     "global_load_dwordx2 %1, %8, off offset:512 sc1\n\t"
                     "global_load_dwordx2 %2, %8, off offset:1024 sc1\n\t"
                     "global_load_dwordx2 %3, %8, off offset:1536 sc1\n\t"
                     "global_load_dwordx2 %4, %8, off offset:2048 sc1\n\t"
                     "global_load_dwordx2 %5, %8, off offset:2560 sc1\n\t"
                     "global_load_dwordx2 %6, %8, off offset:3072 sc1\n\t"
                     "global_load_dwordx2 %7, %8, off offset:3584 sc1\n\t"
                     "s_waitcnt vmcnt(0)"
                     : "=&v"(ev[0]), "=&v"(ev[1]), "=&v"(ev[2]), "=&v"(ev[3]), "=&v"(ev[4]), "=&v"(ev[5]), "=&v"(ev[6]), "=&v"(ev[7])
                     : "v"(src)
                     : "memory");
    }
    uint32_t key[kEPL], idx[kEPL];
    bool valid[kEPL];
#pragma unroll
    for (int j = 0; j < kEPL; j++) {
        const int e = j * 64 + lane;
        valid[j] = (e & 1) ? (e >> 1) < n_hi : (e >> 1) < n_lo;
        key[j] = valid[j] ? (uint32_t)ev[j] : 0u;
        idx[j] = (uint32_t)(ev[j] >> 32);
    }
    float newf = -__builtin_inff();
    if (n >= kth) {
        // a lower bound of the K-th largest key: bisection on the 16 leading key bits (sign, exponent, 7 mantissa
        // bits), the rest left at zero.  Any bound <= the true K-th best keeps the exactness argument; the 2^-7
        // relative slack keeps a few more entries and halves the cost of a compaction.
        uint32_t prefix = 0;
        for (int b = 31; b >= 16; --b) {
            const uint32_t trial = prefix | (1u << b);
            int c = 0;
#pragma unroll
            for (int j = 0; j < kEPL; j++) c += __builtin_popcountll(__builtin_amdgcn_ballot_w64(key[j] >= trial));
            if (c >= kth) prefix = trial;
        }
        newf = fkey_inv(prefix) - s_mg[ql];
    }
    // SYM: the own list is a PART of the query's candidates, so its K-th best says nothing against the warm start: a bound
    // below the current threshold (or no bound at all) leaves threshold and list as they are
    if (SYM && newf <= s_f[ql]) {
        newf = s_f[ql];
        // nothing will be dropped: the next attempt waits for 64 more entries (s_hc, unused without HIST, holds the list length that
        // allows it) instead of following every append
        if (lane == 0) s_hc[ql] = n + 64;
    }
    // trust (a history slice started from tie_warm_kernel's bound): the starting threshold is a proven lower bound of the K-th best
    // score of the rows in front of the slice -- the slice's own rows need not prove it again, and it never falls
    if (trust && newf < s_f[ql]) newf = s_f[ql];
    if (newf < s_f[ql]) {
        // Only a warm-started threshold can be above what the list proves (thresholds derived from the list never fall):
        // the K-th best of everything above it is not known to clear it by the margin, so rows may have been dropped
        // wrongly.  The query is swept again from -inf by the host (flag 2).
        if (lane == 0) {
            s_f[ql] = __builtin_inff();
            s_cnt[2 * ql] = 0;  // the list is dropped: nothing of it triggers another compaction
            s_cnt[2 * ql + 1] = 0;
            *flag = 2;
        }
        return;
    }
    int base = 0;
    int hbase = HIST ? s_hc[ql] : 0;
    bool hist_full = false;
#pragma unroll
    for (int j = 0; j < kEPL; j++) {
        const bool keep = valid[j] && (fkey_inv(key[j]) >= newf);
        const uint64_t m = __builtin_amdgcn_ballot_w64(keep);
        if (keep) qb[base + lane_rank(m)] = make_uint2(key[j], idx[j]);  // survivors packed into slots 0 .. base-1
        base += __builtin_popcountll(m);
        if (HIST) {
            const uint64_t md = __builtin_amdgcn_ballot_w64(valid[j] && !keep);
            const int nd = __builtin_popcountll(md);
            if (hbase + nd > kHistCap)
                hist_full = true;
            else if (valid[j] && !keep)
                hb[hbase + lane_rank(md)] = make_uint2(key[j], idx[j]);
            if (!hist_full) hbase += nd;
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (lane == 0) {
        s_cnt[2 * ql] = (base + 1) >> 1;  // slots 0 .. base-1 read as the two interleaved sub-lists again
        s_cnt[2 * ql + 1] = base >> 1;
        s_f[ql] = newf;
        if (HIST) s_hc[ql] = hbase;
        if (base > kOverflowAt || hist_full) {  // ties / a margin too wide for the list: stop collecting, path A decides
            s_f[ql] = __builtin_inff();
            *flag = 1;
        }
    }
}


// Maxima of MFMA results are taken by instructions the COMPILER emits (fmaxf nests become v_max3_f32): an inline-asm
// v_max3_f32 reading an accumulator right behind the MFMA that writes it gets no wait states from hipcc (asm statements are
// not padded: cdna_hip_programming.md 5.7) and reads the registers before the matrix pipe has written them -- measured:
// maxima too small, blocks with a candidate skipped, 23,000 of a million queries failing the warm start's verification.
__device__ __forceinline__ float max3f(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }
__device__ __forceinline__ float max2f(float a, float b) { return fmaxf(a, b); }

// SYM -- the symmetric form of an all-pairs sweep.  When the queries are the stored rows sym_q0 .. sym_q0 + nq themselves, the
// score of (query c, row r) is also the score of (query r, row c): the workgroup of query block C multiplies only the row tiles
// that do NOT lie in a later query block (the rows before the query range, the query blocks 0 .. C, the rows behind the range) and,
// for the tiles of the EARLIER query blocks, reads every 32 x 32 block of scores a second time along its rows: in the MFMA's D
// layout a lane holds ONE column and sixteen rows, so the second test is sixteen compares against the rows' own thresholds
// (brought into LDS with the tile).  What passes is a candidate of the ROW's query among the columns: it is staged in LDS per
// wave and appended -- in batches, by returning atomics on a per-query counter -- to that query's FOREIGN list; foreign
// thresholds are the pilot's and stay frozen (any threshold that was ever valid is a valid lower bound).  Every (query, row) pair
// is covered exactly once: by the query's own workgroup when the row's tile is not one it skips, else by the workgroup of the
// row's block (tests/test_topk_sym_schedule_cpu.py walks the schedule).  Workgroups are issued longest first (block C = grid - 1 -
// blockIdx.x sweeps C + 1 query blocks): half the MFMA work of the square sweep, and no partial last round.
template <int KP, int NCB, int EP, bool HIST, int RB, bool SYM = false>
__global__ __launch_bounds__(64 * sweep_waves(HIST, KP), (sweep_waves(HIST, KP) + 3) / 4 < 2 ? 2 : (sweep_waves(HIST, KP) + 3) / 4) void topk_sweep_kernel(SweepParams p) {
    constexpr int kWaves = sweep_waves(HIST, KP);
    constexpr int kThreads = kWaves * 64;
    constexpr int kTR = 32 * RB;
    constexpr bool SCALE = EP != EP_NONE;  // a per-row value travels with the tile
    constexpr int KPAD = KP * 16;
    constexpr bool DMA = sweep_dma(KP, HIST, RB, kWaves);
    constexpr bool PIPE = KP <= 8 && !HIST;  // row blocks software-pipelined: see the row-block loop
    static_assert(!DMA || SCALE, "the DMA sweeps mask the rows past N through the row values (NaN padding)");
    // register staging: +16 B per row, consecutive rows start 4 banks apart, ds_read_b128 conflict-free; DMA: unpadded rows,
    // the pieces of a row swizzled instead (see piece_swizzle)
    constexpr int ROWB = (int)sweep_row_bytes(KP, DMA);
    constexpr int QW = 32 * NCB;
    constexpr int BQ = QW * kWaves;
    constexpr int CHUNKS = kTR * KP * 2;  // 16-byte pieces per tile
    constexpr int CPT = (CHUNKS + kThreads - 1) / kThreads;
    constexpr int NBUF = sweep_bufs(KP, RB, BQ, kWaves, HIST, SYM);
    static_assert(!SYM || (DMA && !HIST && BQ % kTR == 0 && EP != EP_NONE), "SYM: a DMA main sweep whose query blocks are whole tiles");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char *s_tile = smem;
    float *s_rs = reinterpret_cast<float *>(smem + (size_t)NBUF * kTR * ROWB);
    float *s_fq = s_rs + NBUF * kTR;                // SYM: the thresholds of the tile's rows as queries ...
    float *s_fqr = s_fq + (SYM ? NBUF * kTR : 0);   // ... and their raw-score form (RAWF)
    float *s_bmm = s_fqr + (SYM ? NBUF * kTR : 0);  // register staging only: per buffer and 32-row block the (min, max) row scale
    int *s_cnt = reinterpret_cast<int *>(s_bmm + (DMA ? 0 : NBUF * 2 * kMaxRB));  // 2 per query: the interleaved sub-list lengths
    float *s_f = reinterpret_cast<float *>(s_cnt + 2 * BQ);
    float *s_mg = s_f + BQ;
    int *s_hc = reinterpret_cast<int *>(s_mg + BQ);
    // tile counters: s_sync[b] = waves whose part of a tile has reached buffer b (ever), s_sync[NBUF + b] = waves that
    // have finished reading one
    int *s_sync = s_hc + BQ;
    uint2 *s_stage = reinterpret_cast<uint2 *>(s_sync + 16);  // SYM: kWaves x kStageCap staged foreign candidates
    float *s_fmin = reinterpret_cast<float *>(s_stage + kWaves * kStageCap);  // SYM: per tile buffer and 32-row block the smallest row threshold

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    // SYM: longest workgroups first; of a triangle shard the blocks sym_rank, sym_rank + sym_world, ... (the grid holds exactly those)
    const int cblk = SYM ? p.sym_rank + p.sym_world * (int)(gridDim.x - 1 - blockIdx.x) : (int)blockIdx.x;
    const int64_t wgq0 = (int64_t)cblk * BQ;
    for (int t = tid; t < BQ; t += kThreads) {
        const int64_t q = wgq0 + t;
        s_cnt[2 * t] = 0;
        s_cnt[2 * t + 1] = 0;
        s_hc[t] = 0;
        s_f[t] = q < p.nq ? (p.f0 ? p.f0[q] : (HIST && p.fwarm ? p.fwarm[(int64_t)blockIdx.y * p.nq + q] : -__builtin_inff()))
                          : __builtin_inff();
        s_mg[t] = q < p.nq ? p.qmargin[q] : 0.0f;
    }
    if (tid < 2 * NBUF) s_sync[tid] = 0;
    // query operands: resident in registers for the whole sweep
    bf16x8 bfrag[NCB][KP];
#pragma unroll
    for (int cb = 0; cb < NCB; cb++) {
        int64_t q = wgq0 + w * QW + cb * 32 + (lane & 31);
        if (q >= p.nq) q = p.nq - 1;
        const uint4 *src = reinterpret_cast<const uint4 *>(p.B + q * KPAD) + (lane >> 5);
#pragma unroll
        for (int ks = 0; ks < KP; ks++) {
            uint4 v = src[ks * 2];
            bfrag[cb][ks] = *reinterpret_cast<bf16x8 *>(&v);
        }
    }
    // the operands are consumed here once, so that hipcc waits for their loads NOW: a load still pending when the tile loop is
    // entered costs a wait in every iteration (and that wait drains the LDS-DMA of the tiles in flight)
#pragma unroll
    for (int cb = 0; cb < NCB; cb++)
#pragma unroll
        for (int ks = 0; ks < KP; ks++) asm volatile("" : "+v"(bfrag[cb][ks]));

    const int64_t stride_rows = (int64_t)p.tile_stride * kTR;  // the pilot samples every tile_stride-th tile
    // A history sweep may be cut into row slices (blockIdx.y): every slice sweeps its own tiles from a cold threshold and
    // keeps its own lists; topk_tie_sort_kernel joins them (see there for why that is a superset of the unsliced history).
    const int64_t NT_all = (p.N + stride_rows - 1) / stride_rows;
    const int64_t T0 = NT_all * blockIdx.y / gridDim.y, T1 = NT_all * (blockIdx.y + 1) / gridDim.y;
    // SYM (one slice, stride 1): the tiles [skip_lo, skip_lo + skip_n) -- whole tiles of LATER query blocks -- are left to those
    // blocks' workgroups; the tiles [tr_lo, tr_hi) -- the earlier query blocks -- are read along their rows as well
    const SymSchedule sched(SYM ? p.sym_q0 : 0, SYM ? p.nq : 0, kTR, BQ, cblk);  // topk_sym.hpp
    // SYM with row slices (gridDim.y > 1: the long blocks of a triangle shard): slice y takes an even share of the tiles the block
    // multiplies, with its own candidate lists (qslice below), the foreign side unchanged
    const int64_t NTs = SYM ? sched.tiles(NT_all) : 0;
    const int64_t S0 = SYM ? NTs * blockIdx.y / gridDim.y : 0, S1 = SYM ? NTs * (blockIdx.y + 1) / gridDim.y : 0;
    const int64_t NT = SYM ? S1 - S0 : T1 - T0;
    auto tile_index = [&](int64_t tl) -> int64_t {  // the tl-th tile this workgroup multiplies
        if constexpr (SYM) return sched.tile_index(S0 + tl);
        else return T0 + tl;
    };
    const int64_t qslice = (int64_t)blockIdx.y * p.nq;  // this slice's rows of the per-query output arrays

    // ---- register staging (history sweeps, operand depths that are not a power of two) ----
    uint4 pre[DMA ? 1 : CPT];
    float pre_rs = 0.0f;
    auto load_tile = [&](int64_t tl) {
        const int64_t base_row = tile_index(tl) * stride_rows;
#pragma unroll
        for (int c = 0; c < CPT; c++) {
            const int ch = tid + c * kThreads;
            if (ch < CHUNKS) {
                const int row = ch / (KP * 2), cc = ch % (KP * 2);
                const int64_t grow = base_row + row;
                pre[DMA ? 0 : c] = grow < p.N ? reinterpret_cast<const uint4 *>(p.A + grow * KPAD)[cc] : make_uint4(0, 0, 0, 0);
            }
        }
        if (SCALE && tid < kTR) pre_rs = base_row + tid < p.N ? p.rscale[base_row + tid] : 0.0f;
    };
    auto store_tile = [&](int buf) {
#pragma unroll
        for (int c = 0; c < CPT; c++) {
            const int ch = tid + c * kThreads;
            if (ch < CHUNKS) {
                const int row = ch / (KP * 2), cc = ch % (KP * 2);
                *reinterpret_cast<uint4 *>(s_tile + (size_t)buf * kTR * ROWB + row * ROWB + cc * 16) = pre[DMA ? 0 : c];
            }
        }
        if (SCALE && tid < kTR) {
            s_rs[buf * kTR + tid] = pre_rs;
            // (min, max) of the 32 scales of this row block; rows past N carry 0 and never qualify anyway
            float mn = pre_rs > 0.0f ? pre_rs : __builtin_inff(), mx = pre_rs;
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) {
                mn = fminf(mn, __shfl_xor(mn, o, 64));
                mx = fmaxf(mx, __shfl_xor(mx, o, 64));
            }
            if ((tid & 31) == 0) {
                s_bmm[(buf * kMaxRB + (tid >> 5)) * 2 + 0] = mn;
                s_bmm[(buf * kMaxRB + (tid >> 5)) * 2 + 1] = mx;
            }
        }
    };

    // ---- LDS-DMA ----
    // Piece c (16 bytes) of row r lives at piece c ^ piece_swizzle(r) of the row's LDS image: the 16 lanes of a ds_read_b128
    // group read one piece column of 16 different rows, and the XOR spreads them over the 16 slots of the 256-byte bank row.
    constexpr int PPR = KP * 2;  // pieces per row
    auto piece_swizzle = [](int row) -> int {
        if constexpr (PPR >= 16) return row & 15;
        else if constexpr (PPR == 8) return (row >> 1) & 7;
        else if constexpr (PPR == 4) return (row >> 2) & 3;
        else return (row >> 3) & 1;
    };
    // A wave-instruction moves 64 pieces.  The two waves that share a SIMD (w and w + kWaves / 2: a workgroup's waves go round
    // the four SIMDs) take turns: the lower half of the waves moves the even tiles, the upper half the odd ones, so that
    // while one of the two spends its ~150 cycles per DMA instruction the other has the MFMA pipe to itself -- issued by all
    // eight at the top of every tile, both waves of every SIMD stood in that phase together (17 % of the sweep,
    // profiles/r03_l_probe_c4_prof.txt).  DMA instruction j of issuing wave wi covers pieces [(wi * DPW + j) * 64, +64) of
    // the tile; the row values (one dword per row) follow as instructions of 64 rows each, issued by the first kTR / 64 of them.
    static_assert(!DMA || kWaves == kWavesMain, "every DMA sweep has the main sweep's workgroup: its waves move the tiles in two halves");
    constexpr int ISS = DMA ? kWaves / 2 : 1;  // waves that move one tile
    constexpr int DPW = DMA ? CHUNKS / 64 / ISS : 0;  // tile instructions per issuing wave
    static_assert(!DMA || (CHUNKS % (64 * ISS) == 0 && kTR % 64 == 0 && kTR / 64 <= ISS), "DMA tiling");
    constexpr int RSW = DMA ? kTR / 64 : 0;              // issuing waves that also move a row-value instruction
    const int wu = __builtin_amdgcn_readfirstlane(w);    // provably wave-uniform (LDS destinations, branch conditions)
    const int wi = wu % ISS, grp = wu / ISS;             // place among the waves that move a tile; which tiles (parity)
    constexpr int ISS_OR_ALL = DMA ? ISS : kWaves;       // announcements that complete a tile
    // The DMA is issued from inline assembly: the builtin makes hipcc treat every later LDS access of the kernel (the tile
    // counters, the fragment reads) as dependent on it and put s_waitcnt vmcnt(0) in front -- which drains the very tiles
    // that are meant to stay in flight.  An asm statement is invisible to that bookkeeping (cdna_hip_programming.md 5.7);
    // the waits are dma_wait's.  M0 = LDS destination of lane 0; the statement saves and restores it.
    // Addressing: the tile's first byte is a scalar (it advances by one tile per iteration), the lane's place inside the
    // tile a 32-bit register computed once -- global_load_lds with an SGPR base and a VGPR offset.  The last tile, whose
    // rows may lie past N, clamps its rows instead (their scores are discarded through the NaN padding of the row values).
    const unsigned lds_tiles = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)s_tile;
    const unsigned lds_rs = (unsigned)(uintptr_t)(__attribute__((address_space(3))) float *)s_rs;
    const unsigned lds_fq = (unsigned)(uintptr_t)(__attribute__((address_space(3))) float *)s_fq;
    const unsigned lds_fqr = (unsigned)(uintptr_t)(__attribute__((address_space(3))) float *)s_fqr;
    constexpr bool RAWF_ = EP == EP_COARSE && DMA;  // (RAWF below)
    unsigned dsrc[DMA ? DPW : 1];  // byte offset of this lane's piece of instruction j from the tile's first byte
    if constexpr (DMA) {
#pragma unroll
        for (int j = 0; j < DPW; j++) {
            const int piece = (wi * DPW + j) * 64 + lane;
            const int row = piece / PPR, cs = piece % PPR;  // LDS position; its content is source piece cs ^ swizzle
            dsrc[j] = (unsigned)(row * (KPAD * 2) + ((cs ^ piece_swizzle(row)) << 4));
        }
    }
    auto dma_tile = [&](int64_t tl, int buf) {
        if constexpr (DMA) {
            const int64_t base_row = tile_index(tl) * stride_rows;
            const bool inside = base_row + kTR <= p.N;  // wave-uniform
            const unsigned char *tile0 = reinterpret_cast<const unsigned char *>(p.A) + base_row * (KPAD * 2);
#pragma unroll
            for (int j = 0; j < DPW; j++) {
                const unsigned dst = __builtin_amdgcn_readfirstlane(lds_tiles + (unsigned)buf * (kTR * ROWB) + (unsigned)(wi * DPW + j) * 1024u);
                unsigned keep;
                if (inside) {
                    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                                 : "=&s"(keep) : "v"(dsrc[j]), "s"(tile0), "s"(dst) : "memory");
                } else {
                    const int piece = (wi * DPW + j) * 64 + lane;
                    const int row = piece / PPR, cs = piece % PPR;
                    int64_t grow = base_row + row;
                    if (grow >= p.N) grow = p.N - 1;
                    const uint16_t *src = p.A + grow * KPAD + ((cs ^ piece_swizzle(row)) << 3);
                    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                                 : "=&s"(keep) : "v"(src), "s"(dst) : "memory");
                }
            }
            if (wi < RSW) {  // the row values are padded with NaN past N (topk_mfma_prepare): no clamp
                const float *src = p.rscale + base_row + wi * 64 + lane;
                const unsigned dst = __builtin_amdgcn_readfirstlane(lds_rs + (unsigned)(buf * kTR + wi * 64) * 4u);
                unsigned keep;
                asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
                             : "=&s"(keep) : "v"(src), "s"(dst) : "memory");
                if constexpr (SYM) {
                    // the thresholds of the tile's rows as queries (any valid address for a tile outside the query range: its
                    // values are never looked at)
                    int64_t qi = base_row - p.sym_q0 + wi * 64 + lane;
                    qi = qi < 0 ? 0 : (qi >= p.nq ? p.nq - 1 : qi);
                    const float *s1 = p.frow + qi;
                    const unsigned d1 = __builtin_amdgcn_readfirstlane(lds_fq + (unsigned)(buf * kTR + wi * 64) * 4u);
                    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
                                 : "=&s"(keep) : "v"(s1), "s"(d1) : "memory");
                    if constexpr (RAWF_) {
                        const float *s2 = p.frow_raw + qi;
                        const unsigned d2 = __builtin_amdgcn_readfirstlane(lds_fqr + (unsigned)(buf * kTR + wi * 64) * 4u);
                        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
                                     : "=&s"(keep) : "v"(s2), "s"(d2) : "memory");
                    }
                }
            }
        }
    };
    // everything this wave has issued is complete: the tile it moved is in LDS (a wave has one tile in flight at a time)
    auto dma_wait = [&]() {
        if constexpr (DMA) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    };
    auto post = [&](int *ctr) {  // DMA: this wave's part of a tile is in LDS (dma_wait came first)
        asm volatile("" ::: "memory");
        if (lane == 0) __hip_atomic_fetch_add(ctr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    };
    // SYM: the waves that moved the rows' thresholds (64 rows each) leave the smallest one of every 32-row block next to them, before
    // they announce the tile: a block whose largest score stays below it needs no row-by-row test (LDS runs a wave's operations in order)
    auto landed = [&](int b) {
        if constexpr (SYM) {
            if (wi < RSW) {
                float v = (RAWF_ ? s_fqr : s_fq)[b * kTR + wi * 64 + lane];
#pragma unroll
                for (int o = 16; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
                if ((lane & 31) == 0) s_fmin[b * kMaxRB + wi * 2 + (lane >> 5)] = v;
            }
        }
    };

    // The waves of a workgroup share every tile but do not march in step: a wave that takes the candidate path
    // used to hold the other seven at the tile's barrier -- 27 % of the sweep (profiles/r02_f_probe_topk_prof.txt).  With NBUF
    // buffers and two counters per buffer a wave only waits for what it needs: tile t complete in its buffer before it
    // multiplies it, the tile that buffer held before read by everyone before it is overwritten.
    // LDS executes a wave's operations in issue order, so a counter increment behind the wave's own LDS traffic needs no
    // fence (a workgroup-scope release would also drain the DMA in flight: s_waitcnt vmcnt(0)); the compiler is kept from
    // moving memory operations across by the asm statements' memory clobbers.
    auto arrive = [&](int *ctr) {
        if constexpr (DMA)
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wave's ds_reads of the tile have returned
        else
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");  // this wave's LDS traffic has completed
        if (lane == 0) __hip_atomic_fetch_add(ctr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    };
    auto wait_for = [&](int *ctr, int target) {
        // bounded (a few seconds): a protocol error shows as wrong rows in the parity tests, not as a hung device
        for (unsigned spins = 0; __hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < target && spins < (1u << 26); spins++)
            __builtin_amdgcn_s_sleep(1);
        if constexpr (DMA)
            asm volatile("" ::: "memory");
        else
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    };
    __syncthreads();  // the per-query words and the counters are initialised
    if constexpr (DMA) {
        if (grp == 0 && NT > 0) {
            dma_tile(0, 0);
            dma_wait();
            landed(0);
            post(&s_sync[0]);
        }
        if (grp == 1 && NT > 1) dma_tile(1, 1);  // announced at the top of tile 0
    } else {
        if (NT > 0) {
            load_tile(0);
            store_tile(0);
            arrive(&s_sync[0]);
        }
        if (NT > 1) load_tile(1);
    }

    // RAWF (EP_COARSE with the index-wide bounds of the row values): the block and quad tests compare RAW maxima with the
    // threshold divided by the extreme row value, rounded down -- fl(raw * s) >= f with s <= rs_max (f > 0), or s >= rs_min and
    // raw < 0 (f <= 0), implies raw >= fraw -- so that rows are scaled only inside a quad that holds a candidate
    constexpr bool RAWF = EP == EP_COARSE && DMA;
    auto raw_threshold = [&](float f) -> float {
        const float q = f / (f > 0.0f ? p.rs_max : p.rs_min);
        return fabsf(q) == __builtin_inff() ? q : q - fabsf(q) * 2.4e-7f;
    };
    float fth[NCB], fraw[RAWF ? NCB : 1];
    int cnt[NCB];      // length of this lane's sub-list of its query (mirrored in s_cnt around a compaction)
    uint2 *mine[NCB];  // the lane's sub-list: slots 2 * c + (lane >> 5) of its query's list (see compact_query)
#pragma unroll
    for (int cb = 0; cb < NCB; cb++) {
        const int ql = w * QW + cb * 32 + (lane & 31);
        fth[cb] = s_f[ql];
        if (RAWF) fraw[RAWF ? cb : 0] = raw_threshold(fth[cb]);
        cnt[cb] = 0;
        mine[cb] = p.cbuf + (qslice + wgq0 + ql) * kCap + (lane >> 5);
    }
    // DMA: the lane's read offsets inside a 32-row block, one per k-step (row & 15 is the same in every block of a tile)
    unsigned aoff[DMA ? KP : 1];
    if constexpr (DMA) {
        const int r = lane & 31;
#pragma unroll
        for (int ks = 0; ks < KP; ks++) aoff[ks] = (unsigned)(r * ROWB + (((ks * 2 + (lane >> 5)) ^ piece_swizzle(r)) << 4));
    }

    // SYM: what the column's own row contributes to a score read along the rows (its scale / bias; NaN for a column that must
    // not emit: a lane past nq, a column whose own tile also holds rows outside the query range -- every workgroup multiplies
    // that tile itself -- and a masked row)
    float csv[NCB];
    int stage_n = 0;  // staged foreign candidates of this wave (wave-uniform)
#pragma unroll
    for (int cb = 0; cb < NCB; cb++) {
        csv[cb] = __builtin_nanf("");
        if constexpr (SYM) {
            const int64_t q = wgq0 + w * QW + cb * 32 + (lane & 31);
            if (SymSchedule::column_emits(p.sym_q0, p.nq, kTR, q)) csv[cb] = p.rscale[p.sym_q0 + q];
            asm volatile("" : "+v"(csv[cb]));  // consumed now: no load pending when the tile loop is entered
        }
    }
    // the staged entries to their queries' foreign lists: one returning atomic per entry, issued from an asm statement together
    // with its wait (as compact_query's loads: a memory operation hipcc can see inside the tile loop costs a vmcnt(0) per tile)
    auto flush_stage = [&]() {
        if constexpr (SYM) {
            uint2 *stg = s_stage + w * kStageCap;
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            for (int e0 = 0; e0 < stage_n; e0 += 64) {
                const int e = e0 + lane;
                const bool on = e < stage_n;
                const uint2 ent = stg[on ? e : 0];
                const uint32_t rowq = ent.y & 0xfffffu, col = ent.y >> 20;
                int32_t *ctr = p.fcnt + rowq;
                int slot = 0;
                const int one = 1;
                if (on)
                    asm volatile("global_atomic_add %0, %1, %2, off sc0\n\ts_waitcnt vmcnt(0)" : "=&v"(slot) : "v"(ctr), "v"(one) : "memory");
                if (on && slot < kCapF) p.fbuf[(int64_t)rowq * kCapF + slot] = make_uint2(ent.x, (uint32_t)(p.sym_q0 + wgq0 + col));
            }
            stage_n = 0;
        }
    };
    // the fragments of the row block about to be multiplied (PIPE), read from block-0-relative address `blk` of a tile
    bf16x8 af[PIPE ? KP : 1];
    auto frag = [&](const unsigned char *blk, int ks) -> bf16x8 {
        return DMA ? *reinterpret_cast<const bf16x8 *>(blk + aoff[DMA ? ks : 0])
                   : *reinterpret_cast<const bf16x8 *>(blk + (lane & 31) * ROWB + (lane >> 5) * 16 + ks * 32);
    };
    int buf = 0, round = 0;  // tile t lives in buffer t % NBUF and is that buffer's (t / NBUF)-th tile
    for (int64_t t = 0; t < NT; t++) {
        const int nb = buf + 1 == NBUF ? 0 : buf + 1;
        if constexpr (DMA) {
            // This wave's half moves the tiles of its parity: at such a tile's top it issues tile t + 2 (into the buffer tile
            // t + 2 - NBUF was read from); at the other tiles' tops it waits for what it issued a tile ago -- everything it has
            // in flight: the appends of the last row blocks ride along, a few hundred cycles now and then -- and announces
            // tile t + 1, three row blocks ahead of its first use.
            const int b2 = nb + 1 == NBUF ? 0 : nb + 1;
            if ((int)(t & 1) == grp) {
                if (t + 2 < NT) {
                    if (t + 2 >= NBUF) wait_for(&s_sync[NBUF + b2], kWaves * (int)((t + 2) / NBUF));
                    dma_tile(t + 2, b2);
                }
            } else if (t + 1 < NT) {
                dma_wait();
                landed(nb);
                post(&s_sync[nb]);
            }
        } else {
            if (t + 1 < NT) {  // rows of tile t + 1 (loaded during tile t - 1) into the buffer tile t + 1 - NBUF was read from
                if (t + 1 >= NBUF) wait_for(&s_sync[NBUF + nb], kWaves * (round + (nb == 0 ? 1 : 0)));  // = kWaves * ((t + 1) / NBUF)
                store_tile(nb);
                arrive(&s_sync[nb]);
            }
            if (t + 2 < NT) load_tile(t + 2);
        }
        // PIPE: tile t has been waited for inside the last row block of tile t - 1 (its first fragments are in registers)
        if (!PIPE || t == 0) wait_for(&s_sync[buf], ISS_OR_ALL * (round + 1));
        const unsigned char *tb = s_tile + (size_t)buf * kTR * ROWB;
        if (PIPE && t == 0) {
#pragma unroll
            for (int ks = 0; ks < KP; ks++) af[PIPE ? ks : 0] = frag(tb, ks);
        }
        const int64_t base_row = tile_index(t) * stride_rows;
        // SYM: a tile of an earlier query block is read along its rows too (wave-uniform)
        const bool trans = SYM && sched.transposed(tile_index(t));
        // register staging zero-fills the rows past N; their scores are set to NaN below.  The DMA sweeps need nothing: the
        // row values of those rows are NaN
        const int valid = DMA ? kTR : (int)std::min<int64_t>(kTR, p.N - base_row);
        // not unrolled: four copies of the epilogue and its candidate path cost the C4 instantiation 34 spilled VGPRs
#pragma unroll 1
        for (int rb = 0; rb < RB; rb++) {
            f32x16 acc[NCB];
#pragma unroll
            for (int cb = 0; cb < NCB; cb++)
#pragma unroll
                for (int r = 0; r < 16; r++) acc[cb][r] = 0.0f;
            if constexpr (PIPE) {
                // Software pipeline over row blocks (and across tiles): the fragments of block rb are in registers when its
                // MFMAs start; each register quad is refilled with the NEXT block's fragment as soon as the last MFMA reading it
                // is issued, so the LDS round trip runs under the rest of the chain and the epilogue instead of ahead of the
                // first MFMA.  The next block of the last row block is block 0 of tile t + 1, announced a tile ago.
                const unsigned char *nx = tb + (rb + 1) * 32 * ROWB;
                if (rb + 1 == RB) {
                    nx = tb;  // last tile: a re-read nobody uses
                    if (t + 1 < NT) {
                        wait_for(&s_sync[nb], ISS_OR_ALL * (round + (nb == 0 ? 1 : 0) + 1));
                        nx = s_tile + (size_t)nb * kTR * ROWB;
                    }
                }
#pragma unroll
                for (int ks = 0; ks < KP; ks++) {
#pragma unroll
                    for (int cb = 0; cb < NCB; cb++)
                        acc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[ks], bfrag[cb][ks], acc[cb], 0, 0, 0);
                    af[ks] = frag(nx, ks);
                    __builtin_amdgcn_sched_barrier(0);
                }
            } else {
            const unsigned char *rowp = tb + (rb * 32 + (lane & 31)) * ROWB + (lane >> 5) * 16;
            const unsigned char *blkp = tb + rb * 32 * ROWB;  // DMA: + aoff[ks]
            // candidate fragments: up to 8 k-steps of ds_read_b128 in flight ahead of the MFMAs that use them
            constexpr int PF = KP < 8 ? KP : 8;
#pragma unroll
            for (int k0 = 0; k0 < KP; k0 += PF) {
                bf16x8 a[PF];
#pragma unroll
                for (int j = 0; j < PF; j++)
                    if (k0 + j < KP)
                        a[j] = DMA ? *reinterpret_cast<const bf16x8 *>(blkp + aoff[DMA ? k0 + j : 0])
                                   : *reinterpret_cast<const bf16x8 *>(rowp + (k0 + j) * 32);
                __builtin_amdgcn_sched_barrier(0);  // keep the reads ahead: hipcc otherwise sinks each next to its MFMA
#pragma unroll
                for (int j = 0; j < PF; j++)
                    if (k0 + j < KP) {
#pragma unroll
                        for (int cb = 0; cb < NCB; cb++)
                            acc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[j], bfrag[cb][k0 + j], acc[cb], 0, 0, 0);
                    }
            }
            }
            // C layout: lane holds column (= query) lane&31, rows (r&3) + 8*(r>>2) + 4*(lane>>5).
            // The epilogue shares the SIMD's issue slots with the sibling wave's MFMAs (about five ordinary instructions fit
            // beside one MFMA: MI355X_MICROARCH.md), so it is counted in instructions: 10 for the maxima of a column block,
            // 4 for the bound, 2 for the vote.
#pragma unroll
            for (int cb = 0; cb < NCB; cb++) {
                if constexpr (SYM) {
                    if (trans) {
                        // the block read along its rows: score (query = row, candidate = this lane's column) against the ROW's threshold.
                        // RAWF: raw scores against the rows' raw thresholds, the column's scale only behind that test.
                        const float4 *t4 = reinterpret_cast<const float4 *>((RAWF ? s_fqr : s_fq) + buf * kTR + rb * 32);
                        const float cv = csv[cb];
                        auto col_score = [&](float raw) -> float { return EP == EP_BIAS ? raw + cv : raw * cv; };
                        // first the block's largest score against the smallest threshold of its 32 rows (landed): most blocks end here
                        const float fmin_blk = s_fmin[buf * kMaxRB + rb];
                        float mq[4];
#pragma unroll
                        for (int g = 0; g < 4; g++) mq[g] = max2f(max3f(acc[cb][4 * g], acc[cb][4 * g + 1], acc[cb][4 * g + 2]), acc[cb][4 * g + 3]);
                        const float mraw = max2f(max3f(mq[0], mq[1], mq[2]), mq[3]);
                        if (__builtin_amdgcn_ballot_w64((RAWF ? mraw : col_score(mraw)) >= fmin_blk) != 0) {
                        // sixteen differences and their maxima by quad (the compiler turns a chain of sixteen compares into a bit mask
                        // built from v_cndmask / shifts, five instructions per score); a NaN score (a column that must not emit)
                        // is skipped by the hardware maximum, -0 from a flushed difference only opens the exact test below
                        float qd[4];
#pragma unroll
                        for (int g = 0; g < 4; g++) {
                            const float4 th = t4[2 * g + (lane >> 5)];
                            const float a0 = RAWF ? acc[cb][4 * g + 0] : col_score(acc[cb][4 * g + 0]);
                            const float a1 = RAWF ? acc[cb][4 * g + 1] : col_score(acc[cb][4 * g + 1]);
                            const float a2 = RAWF ? acc[cb][4 * g + 2] : col_score(acc[cb][4 * g + 2]);
                            const float a3 = RAWF ? acc[cb][4 * g + 3] : col_score(acc[cb][4 * g + 3]);
                            qd[g] = max2f(max3f(a0 - th.x, a1 - th.y, a2 - th.z), a3 - th.w);
                        }
                        const float dm = max2f(max3f(qd[0], qd[1], qd[2]), qd[3]);
                        if (__builtin_amdgcn_ballot_w64(dm >= 0.0f) != 0) {
                            const float4 *f4 = reinterpret_cast<const float4 *>(s_fq + buf * kTR + rb * 32);
                            const uint32_t colw = (uint32_t)(w * QW + cb * 32 + (lane & 31)) << 20;  // the column inside the workgroup's block
                            uint2 *stg = s_stage + w * kStageCap;
#pragma unroll
                            for (int g = 0; g < 4; g++) {
                                if (__builtin_amdgcn_ballot_w64(qd[g] >= 0.0f) == 0) continue;
                                const float4 fr4 = f4[2 * g + (lane >> 5)];
                                const float frow[4] = {fr4.x, fr4.y, fr4.z, fr4.w};
#pragma unroll
                                for (int e = 0; e < 4; e++) {
                                    const int r = 4 * g + e;
                                    const float sc = col_score(acc[cb][r]);  // NaN for a column that must not be emitted (csv)
                                    const bool pass = sc >= frow[e];
                                    const uint64_t m = __builtin_amdgcn_ballot_w64(pass);
                                    if (m != 0) {
                                        const int c = __builtin_popcountll(m);
                                        const uint32_t rowq = (uint32_t)(base_row - p.sym_q0) + (uint32_t)(rb * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5));
                                        if (stage_n + c <= kStageCap) {
                                            if (pass) stg[stage_n + lane_rank(m)] = make_uint2(fkey(sc), rowq | colw);
                                            stage_n += c;
                                        } else if (pass) {
                                            p.cflag[rowq] = 1;  // more hits in one block than the staging area holds: that query takes the tie path
                                            atomicAdd(p.sym_stats + 3, 1ull);
                                        }
                                    }
                                }
                            }
                            if (stage_n >= kStageFlushAt) flush_stage();
                        }
                        }
                    }
                }
                auto scale_rows = [&]() {
                    const float4 *r4 = reinterpret_cast<const float4 *>(s_rs + buf * kTR + rb * 32);
#pragma unroll
                    for (int g = 0; g < 4; g++) {
                        const float4 s = r4[2 * g + (lane >> 5)];
                        if (EP == EP_BIAS) {  // q.x - |x|^2 / 2 = (|q|^2 - |q - x|^2) / 2: same order as the distance
                            acc[cb][4 * g + 0] += s.x;
                            acc[cb][4 * g + 1] += s.y;
                            acc[cb][4 * g + 2] += s.z;
                            acc[cb][4 * g + 3] += s.w;
                        } else {
                            acc[cb][4 * g + 0] *= s.x;
                            acc[cb][4 * g + 1] *= s.y;
                            acc[cb][4 * g + 2] *= s.z;
                            acc[cb][4 * g + 3] *= s.w;
                        }
                    }
                };
                if (EP == EP_SCALE || EP == EP_BIAS) scale_rows();
                if (!DMA && valid < kTR) {  // last tile: rows past N never qualify (NaN fails every >=, the maxima skip it)
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        const int row = rb * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                        if (row >= valid) acc[cb][r] = __builtin_nanf("");
                    }
                }
                // maxima of the four register quads (rows 8 g + 4 (lane >> 5) + 0..3), then of the block: the candidate path
                // looks only into the quads whose maximum qualifies
                float gm[4];
#pragma unroll
                for (int g = 0; g < 4; g++) gm[g] = max2f(max3f(acc[cb][4 * g], acc[cb][4 * g + 1], acc[cb][4 * g + 2]), acc[cb][4 * g + 3]);
                float m = max2f(max3f(gm[0], gm[1], gm[2]), gm[3]);
                if (EP == EP_COARSE && !RAWF) {  // an upper bound of every scaled score of the block: the row values are positive
                    const float mn = s_bmm[(buf * kMaxRB + rb) * 2 + 0];
                    const float mx = s_bmm[(buf * kMaxRB + rb) * 2 + 1];
                    m = m * (m >= 0.0f ? mx : mn);
                }
                if (__builtin_amdgcn_ballot_w64(m >= (RAWF ? fraw[RAWF ? cb : 0] : fth[cb])) != 0) {
                    __builtin_amdgcn_s_setprio(3);  // the wave on this path is the one its workgroup waits for
                    if (EP == EP_COARSE && !RAWF) {
                        scale_rows();
#pragma unroll
                        for (int g = 0; g < 4; g++) gm[g] = max2f(max3f(acc[cb][4 * g], acc[cb][4 * g + 1], acc[cb][4 * g + 2]), acc[cb][4 * g + 3]);
                    }
                    float4 rs4[RAWF ? 4 : 1];  // RAWF: the row values of the four quads, in flight while the quads are tested
                    if (RAWF) {
                        const float4 *r4 = reinterpret_cast<const float4 *>(s_rs + buf * kTR + rb * 32);
#pragma unroll
                        for (int g = 0; g < 4; g++) rs4[RAWF ? g : 0] = r4[2 * g + (lane >> 5)];
                    }
                    const float f = fth[cb];
                    const float fq = RAWF ? fraw[RAWF ? cb : 0] : f;  // what a quad's maximum is compared with
                    // Every lane appends to ITS OWN sub-list of the query (even / odd slots, see compact_query), so no slot
                    // exchange between the two lanes of a query and no counting pass are needed.  f is +inf for lanes past nq
                    // and for flagged queries; rows past N are NaN.  A block that comes here holds one or two candidates among
                    // its 1024 scores: a quad is opened only if its maximum qualifies (a NaN maximum never does: the hardware
                    // maximum skips NaN operands, and a quad of four NaNs holds no candidate).
#pragma unroll
                    for (int g = 0; g < 4; g++) {
                        if (gm[g] >= fq) {
                            if (RAWF) {
                                const float4 sc = rs4[RAWF ? g : 0];
                                acc[cb][4 * g + 0] *= sc.x;
                                acc[cb][4 * g + 1] *= sc.y;
                                acc[cb][4 * g + 2] *= sc.z;
                                acc[cb][4 * g + 3] *= sc.w;
                            }
#pragma unroll
                            for (int e = 0; e < 4; e++) {
                                const int r = 4 * g + e;
                                if (acc[cb][r] >= f) {
                                    const uint32_t row = (uint32_t)(base_row + rb * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5));
                                    mine[cb][2 * cnt[cb]] = make_uint2(fkey(acc[cb][r]), row);
                                    cnt[cb]++;
                                }
                            }
                        }
                    }
                    uint64_t need = __builtin_amdgcn_ballot_w64(cnt[cb] > p.compact_at);
                    if (need) {
                        const int ql = w * QW + cb * 32 + (lane & 31);
                        s_cnt[2 * ql + (lane >> 5)] = cnt[cb];
                        need = (need | (need >> 32)) & 0xffffffffull;  // either sub-list of a query
                        do {
                            const int l = __builtin_ctzll(need);
                            need &= need - 1;
                            const int qlc = w * QW + cb * 32 + l;
                            // (see compact_query; a sub-list holds kCap / 2 entries and a block adds at most 16 to one)
                            if (SYM && s_cnt[2 * qlc] + s_cnt[2 * qlc + 1] < s_hc[qlc] && s_cnt[2 * qlc] <= kCap / 2 - 32 &&
                                s_cnt[2 * qlc + 1] <= kCap / 2 - 32)
                                continue;
                            compact_query<HIST, SYM>(p.cbuf + (qslice + wgq0 + qlc) * kCap, qlc, p.kth, s_cnt, s_f, s_mg,
                                                p.cflag + qslice + wgq0 + qlc,
                                                HIST ? p.hbuf + (qslice + wgq0 + qlc) * kHistCap : nullptr, s_hc, HIST && p.fwarm != nullptr);
                        } while (need);
                        cnt[cb] = s_cnt[2 * ql + (lane >> 5)];
                        fth[cb] = s_f[ql];
                        if (RAWF) fraw[RAWF ? cb : 0] = raw_threshold(fth[cb]);
                    }
                    __builtin_amdgcn_s_setprio(0);
                }
            }
        }
        arrive(&s_sync[NBUF + buf]);  // this wave has read tile t
        buf = nb;
        if (nb == 0) round++;
    }
    if (SYM && stage_n > 0) flush_stage();
    // final threshold + compaction of every list this wave owns
#pragma unroll
    for (int cb = 0; cb < NCB; cb++) s_cnt[2 * (w * QW + cb * 32 + (lane & 31)) + (lane >> 5)] = cnt[cb];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int l = 0; l < QW; l++) {
        const int ql = w * QW + l;
        if (wgq0 + ql >= p.nq) break;
        const int64_t qg = qslice + wgq0 + ql;
        if (s_f[ql] == __builtin_inff()) {  // flagged
            if (p.f_out && lane == 0) p.f_out[qg] = -__builtin_inff();
            continue;
        }
        compact_query<HIST, SYM>(p.cbuf + qg * kCap, ql, p.kth, s_cnt, s_f, s_mg, p.cflag + qg,
                            HIST ? p.hbuf + qg * kHistCap : nullptr, s_hc, HIST && p.fwarm != nullptr);
        if (lane == 0) {
            p.ccnt[qg] = s_cnt[2 * ql] + s_cnt[2 * ql + 1];  // packed by the final compaction: slots 0 .. count-1
            if (HIST) p.hcnt[qg] = s_hc[ql];
            if (p.f_out) p.f_out[qg] = s_f[ql] == __builtin_inff() ? -__builtin_inff() : s_f[ql];
        }
    }
}

template <int KP, int NCB, int EP, bool HIST, int RB, bool SYM = false>
int32_t launch_sweep_one(gorse_topk *h, const SweepParams &p) {
    constexpr int WV = sweep_waves(HIST, KP);
    constexpr int BQ = 32 * NCB * WV;
    const size_t lds = sweep_lds_bytes(KP, RB, BQ, WV, HIST, SYM);
    unsigned grid = (unsigned)ceil_div(p.nq, BQ);
    if (SYM && p.sym_world > 1) {  // the blocks of this triangle shard
        if ((int64_t)grid <= p.sym_rank) return GORSE_OK;
        grid = (unsigned)ceil_div((int64_t)grid - p.sym_rank, p.sym_world);
    }
    GORSE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&topk_sweep_kernel<KP, NCB, EP, HIST, RB, SYM>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    topk_sweep_kernel<KP, NCB, EP, HIST, RB, SYM>
        <<<dim3(grid, HIST ? (unsigned)std::max(p.nslices, 1) : (SYM ? (unsigned)std::max(p.sym_slices, 1) : 1u)), dim3(WV * 64), lds, h->stream>>>(p);
    GORSE_HIP_CHECK(hipGetLastError());
    return GORSE_OK;
}

template <int KP, int NCB, bool HIST, int RB, bool SYM = false>
int32_t launch_sweep_ep(gorse_topk *h, const SweepParams &p) {
    switch (p.ep) {
        case EP_SCALE: return launch_sweep_one<KP, NCB, EP_SCALE, HIST, RB, SYM>(h, p);
        case EP_BIAS: return launch_sweep_one<KP, NCB, EP_BIAS, HIST, RB, SYM>(h, p);
        case EP_COARSE: return launch_sweep_one<KP, NCB, EP_COARSE, HIST, RB, SYM>(h, p);
    }
    return fail(GORSE_ERR_INVALID, "unknown epilogue %d", p.ep);
}

template <int KP, int NCB>
int32_t launch_sweep(gorse_topk *h, const SweepParams &p, bool hist, bool sym = false) {
    if constexpr (sweep_sym_kp(KP) && NCB == kNcbMain && sweep_dma(KP, false, 4, kWavesMain)) {
        if (sym) return launch_sweep_ep<KP, NCB, false, 4, true>(h, p);
    }
    if (sym) return fail(GORSE_ERR_INVALID, "no symmetric sweep for operand depth %d", KP);
    // 128-row tiles (one tile hand-over per four MFMA row blocks) where LDS allows; the history sweep of the few flagged
    // queries keeps the 64-row form
    const bool wide = !hist && KP <= 8 && rows_per_tile(g_topk_variant) == 128;
    if (wide) {
        if constexpr (KP <= 8) return launch_sweep_ep<KP, NCB, false, 4>(h, p);
    }
    return hist ? launch_sweep_ep<KP, NCB, true, 2>(h, p) : launch_sweep_ep<KP, NCB, false, 2>(h, p);
}

}  // namespace

int32_t gorse::dispatch_sweep(gorse_topk *h, const SweepParams &p, bool hist, bool sym) {
    switch (h->kp) {
        case 1: return launch_sweep<1, kNcbMain>(h, p, hist);
        case 2: return launch_sweep<2, kNcbMain>(h, p, hist, sym);
        case 3: return launch_sweep<3, kNcbMain>(h, p, hist);
        case 4: return launch_sweep<4, kNcbMain>(h, p, hist, sym);
        case 6: return launch_sweep<6, kNcbMain>(h, p, hist);
        case 8: return launch_sweep<8, kNcbMain>(h, p, hist, sym);
        case 12: return launch_sweep<12, 1>(h, p, hist);  // 2 column blocks would spill
        case 16: return launch_sweep<16, 1>(h, p, hist);
        case 24: return launch_sweep<24, 1>(h, p, hist);
    }
    return fail(GORSE_ERR_INVALID, "unsupported operand depth %d", h->kp);
}

