/*
 * gorse_hip_test.h -- test and probe hooks of libgorse_hip.so.  NOT part of the drop-in boundary (include/gorse_hip.h is
 * what the reference's cgo files bind): these switches let the parity tests drive each of two equivalent code paths, let
 * small inputs reach paths that large ones take, and let the probes of scripts/ read phase counters.  Results never
 * depend on them; the product runs with every one at its default.
 */
#ifndef GORSE_HIP_TEST_H
#define GORSE_HIP_TEST_H

#include "gorse_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* exp flavour used by the GORSE_BPR_SEQUENTIAL schedule: 0 = device expf (default),
 * 1 = the float32 FreeBSD/math32 scheme restated in oracle/gorse_oracle.c (orc_exp_restated),
 * which makes device and oracle factors comparable bit for bit. */
void gorse_hip_test_set_exact_exp(int32_t mode);
/* Switches of the BPR Hogwild path, for the parity tests: OR of the six bits below.  Every other bit is ignored; 0 (the default)
 * is the only value the product ever runs with. */
#define GORSE_TEST_BPR_USER_RUNS (1 << 7)       /* the user-run schedule whatever the number of users (product: from 4096 users on) */
#define GORSE_TEST_BPR_PER_SAMPLE (1 << 28)     /* the per-sample schedule whatever the shape (USER_RUNS wins where both are set) */
#define GORSE_TEST_BPR_STABLE_RANK (1 << 29)    /* one thread ranks a chunk's samples in stream order: every run keeps the stream's order */
#define GORSE_TEST_BPR_THREE_KERNELS (1 << 19)  /* the bins' sort, item draws and grouping as three kernels, not bpr_bin_finish_kernel */
#define GORSE_TEST_BPR_ARRIVAL_ORDER (1 << 20)  /* a run's samples stay in arrival order: equal positives are not brought together */
#define GORSE_TEST_BPR_NO_BINS (1 << 21)        /* the chunk preparation without user bins: an atomic per sample on its user's counter */
void gorse_hip_test_set_variant(int32_t variant);
/* top-k path choice: 0 = automatic (MFMA sweep for >= 768 queries, any of the three metrics, k <= 255), 1 = always the
 * literal scan (path A), 2 = the MFMA sweep whenever its operands exist.  Both paths return identical results;
 * the hook exists so the parity tests can drive each one. */
void gorse_hip_test_set_topk_path(int32_t path);
/* Switches of the MFMA sweep and its tie path, for the parity tests: OR of the bits below.  Every other bit is ignored; 0 (the default)
 * is the only value the product ever runs with.  Each drives one of two equivalent code paths or lets a small input reach a path
 * that only a large one takes; results never depend on them. */
#define GORSE_TEST_TOPK_TILE64 (1 << 0)           /* 64 candidate rows per LDS tile of the main sweep instead of 128 (then never symmetric) */
#define GORSE_TEST_TOPK_COARSE_OFF (1 << 2)       /* cosine: every score times its row scale, whatever the norms ... */
#define GORSE_TEST_TOPK_COARSE_ON (1 << 3)        /* ... or the block-level bound first (default: when all norms lie within 2 % of each other) */
#define GORSE_TEST_TOPK_REPLAY_COUNTERS (1 << 4)  /* the tie replay counts its work; the main sweep keeps its square form */
#define GORSE_TEST_TOPK_WARM_OFF (1 << 8)         /* no warm start: no pilot sweeps, every threshold starts at -inf */
#define GORSE_TEST_TOPK_WARM_ALWAYS (1 << 9)      /* warm start, with both pilots, below its size limits of 2^17 / 2^18 rows */
#define GORSE_TEST_TOPK_PILOT_KTH2 (1 << 10)      /* the pilot takes a kth of 2: most warm starts fail their verification */
#define GORSE_TEST_TOPK_COLD_SLICES (1 << 11)     /* every row slice of the tie path's history sweep starts cold */
#define GORSE_TEST_TOPK_SLICES8 (1 << 14)         /* that sweep in eight row slices whatever the index size ... */
#define GORSE_TEST_TOPK_SLICE1 (1 << 15)          /* ... or in one (wins where both are set) */
#define GORSE_TEST_TOPK_SYM_OFF (1 << 23)         /* the square form of an all-pairs sweep where the symmetric one is eligible */
#define GORSE_TEST_TOPK_REPLAY_WAVE64 (1 << 28)   /* the tie replay with 64 queries per wave whatever the launch's size */
/* bits 29-30, row slices per query block of a triangle-sharded sweep (gorse_topk_tri_*): n = 1 / 2 / 3 = one / two / four */
#define GORSE_TEST_TOPK_TRI_SLICES(n) (((n) & 3) << 29)
#define GORSE_TEST_TOPK_MASK                                                                                                     \
    (GORSE_TEST_TOPK_TILE64 | GORSE_TEST_TOPK_COARSE_OFF | GORSE_TEST_TOPK_COARSE_ON | GORSE_TEST_TOPK_REPLAY_COUNTERS |          \
     GORSE_TEST_TOPK_WARM_OFF | GORSE_TEST_TOPK_WARM_ALWAYS | GORSE_TEST_TOPK_PILOT_KTH2 | GORSE_TEST_TOPK_COLD_SLICES |          \
     GORSE_TEST_TOPK_SLICES8 | GORSE_TEST_TOPK_SLICE1 | GORSE_TEST_TOPK_SYM_OFF | GORSE_TEST_TOPK_REPLAY_WAVE64 | GORSE_TEST_TOPK_TRI_SLICES(3))
void gorse_hip_test_set_topk_variant(int32_t variant);
/* how many queries of the last search failed the verification of their warm start and were swept again from -inf */
int32_t gorse_hip_test_topk_resweeps(gorse_topk *h, int64_t *n /*out*/);
/* whether the last search's main sweep took the symmetric form: the queries are a contiguous range of the stored rows that starts on a
 * 128-row boundary, the sweep is warm-started, and the operands are 32 / 64 / 128 bf16 values deep (GORSE_TEST_TOPK_SYM_OFF: never) */
int32_t gorse_hip_test_topk_last_symmetric(gorse_topk *h, int32_t *sym /*out*/);
/* counters of the last symmetric search: [0] queries the pilot left without a threshold (they take the tie path's sweep), [1] warm
 * starts the rescoring could not verify over both lists, [2] foreign lists that overflowed, [3] hits beyond a wave's staging area */
int32_t gorse_hip_test_topk_sym_stats(gorse_topk *h, uint64_t *out4 /*host*/);
/* the per-query flags of the last MFMA search's last chunk (the first n queries) as the host read them behind the rescoring: non-zero =
 * the query left sweep + rescoring undecided and went on to the tie path (ties among its k + 1 best exact distances, a warm start
 * that could not be verified, no pilot threshold, an overflowing list) */
int32_t gorse_hip_test_topk_get_flags(gorse_topk *h, uint8_t *flags /*host*/, int64_t n);
/* after a symmetric sweep: the entries other workgroups appended to each query's foreign list (more than 512 = the list overflowed) */
int32_t gorse_hip_test_topk_get_foreign_counts(gorse_topk *h, int32_t *counts /*host*/, int64_t n);
/* the warm-start thresholds of the last search's last chunk (the first n queries) */
int32_t gorse_hip_test_topk_get_thresholds(gorse_topk *h, float *out /*host*/, int64_t n);
/* with GORSE_TEST_TOPK_REPLAY_COUNTERS set, the tie replay (csrc/topk_tie.hip topk_tie_replay_lane_kernel) of a search counts its work; this
 * returns the sixteen counters of the handle's last such replay, over its queries: [0] s_memtime ticks summed, [1] the most of one
 * query, [2] recorded entries summed, [3] queries, [4] heap pushes, [5] gaps evaluated (T^gap), [6] those where T was not the
 * identity, [7] literal applications of T summed, [8] the most of one query, [9] the most recorded entries of one query,
 * [10] queries left undecided; [11]..[15] are zero.  (The counters of the main sweep's instrumented twin, which this hook also
 * served, left with the probe build.) */
int32_t gorse_hip_test_get_sweep_profile(gorse_topk *h, uint64_t *out16 /*host*/);
/* 1 = every query of the literal scan (path A) goes through the one-thread-per-query heap kernel; 0 (default) = the queries whose
 * k + 1 smallest distances are pairwise distinct are answered by select_fast_kernel (same results). */
void gorse_hip_test_set_scan_literal(int32_t on);
/* the scan_literal flags of the LAST scan block of the handle's last call (the first n queries of that block): 1 = select_fast_kernel
 * left the query to the literal kernel or to the reroute through the MFMA path's tie replay (ties among its k + 1 smallest
 * distances, a NaN, k + 1 > 1024, more than 2048 rows at the bound), 0 = it answered; all 1 when gorse_hip_test_set_scan_literal
 * was on.  GORSE_ERR_INVALID when that call did not scan or n exceeds the block's queries. */
int32_t gorse_hip_test_topk_scan_flags(gorse_topk *h, int32_t *flags /*host*/, int64_t n);
/* queries per block of the scan: > 0 replaces min(2^28 / N, 65535) (still at most 65535), 0 restores the rule.  Lets small inputs
 * run the block loop of the three calls.  Results never depend on it. */
void gorse_hip_test_set_scan_block(int64_t queries);
/* sparse top-k (csrc/sparse*.h*).  Results never depend on any of these.
 * slots: at most this many single-wave workgroups per launch of sparse_tile_kernel (0 = the library's 16 per CU). */
void gorse_hip_test_set_sparse_slots(int64_t max_slots);
/* groups that a query of ordinary length visits one by one with directly indexed accumulators; the groups behind them are taken
 * several at once with hashed accumulators (csrc/sparse_kernels.hpp, super-visits).  -1 (default) = the leading groups that hold
 * more than their even share of the stored entries; 0 = none (every group through the super-visit loop, which falls back to the
 * direct accumulators where one group alone has too many postings); a value >= the number of groups = no super-visits. */
void gorse_hip_test_set_sparse_head(int32_t groups);
/* The symmetric form of gorse_sparse_all_pairs over all rows (csrc/sparse_kernels.hpp, SymArgs): mode 0 = never (the walk every other
 * call takes), -1 / 1 = when the call is eligible (default), 2 = likewise, but the front (gorse_hip_test_set_sparse_front) does not deliver.  c1 / c2 / c3 > 0 replace the capacities of the three tiers of foreign lists
 * (tests overflow them on purpose: the rows then take the unsymmetric walk in a second launch); 0 = the defaults.  Results never differ. */
void gorse_hip_test_set_sparse_sym(int32_t mode, int32_t c1, int32_t c2, int32_t c3);
/* handles created AFTERWARDS: the FRONT = the longest rows in a row group of their own when they are fewer than a group holds (phantom
 * scratch ids behind them: csrc/sparse_host.hpp, RowOrder).  1 (default) = the rows longer than 1 .. 2 x the split threshold in force at
 * creation (the largest multiple that leaves 300 rows: gorse_sparse_create), > 1 = the rows longer than this, 0 = plain longest-first
 * numbering.  A symmetric all-pairs pass splits exactly the front's rows into per-group work items. */
void gorse_hip_test_set_sparse_front(int32_t front);
/* the last call of the handle: out[0] = it ran in symmetric form, [1] = rows redone after an overflow, [2] = foreign entries ranked,
 * [3] = the longest foreign list */
void gorse_hip_test_sparse_sym_stats(const gorse_sparse *h, int64_t out[4]);
/* which paths the last search / all-pairs call of the handle took (read only): out[0] = launch rounds (a call with more long queries
 * than its partial rankings and dense copies may hold takes several), [1] = heavy queries (sparse_rows_kernel), summed over the rounds,
 * [2] = the handle's row ranges of sparse_rows_kernel, [3] = its directory cells (distinct indices x row groups). */
void gorse_hip_test_sparse_path_stats(const gorse_sparse *h, int64_t out[4]);
/* rows per group of a handle created AFTERWARDS (the posting lists are cut by row group, csrc/sparse_kernels.hpp): a power of two
 * in 256 .. 16384; 0 = 2048.  A workgroup holds a group's accumulators: 5.5 bytes of LDS per row. */
void gorse_hip_test_set_sparse_tile(int32_t rows);
/* queries with more than `entries` entries are answered by one work item per row group and a merge instead of one item
 * (default 2048; <= 0 = never): lets small test inputs take that path. */
void gorse_hip_test_set_sparse_split(int64_t entries);
/* of those, queries with more than `entries` entries (default 16384; <= 0 = never) do not walk posting lists: every stored row is
 * scored against a dense copy of the query, one row per lane (sparse_rows_kernel). */
void gorse_hip_test_set_sparse_heavy(int64_t entries);
/* how products reach the LDS accumulators: 1 = ds_add_f32 (no return value, no wait), 0 = load / add / store by the same
 * wave, -1 = the library's choice (ds_add_f32 unless a product of a stored and a query value could fall below 2^-100,
 * where partial sums may be subnormal and the LDS adder's handling of those is not relied upon). */
void gorse_hip_test_set_sparse_atomic(int32_t mode);
/* Which kernel family an ALS half-sweep runs (csrc/als.hip als_form), the low two bits: 0 = by nFactors (the Gram form on MFMA
 * tiles up to 64, als_wide_kernel for 65..128, the residual sweep beyond), 1 = always the residual sweep (the reference's own
 * recurrence), 2 = always the MFMA tiles (nFactors <= 64; an error beyond).  All meet the 1e-4 relative bar; the hook lets the
 * parity tests drive each one.  Bits on top of the choice -- these and no others; any other bit is ignored:
 *    8 = als_wide_kernel builds G by fused multiply-adds instead of the MFMA, and S comes from als_gram_partial_kernel;
 *   64 = 64-bit gather addresses in the Gram kernels whatever the shape (the product takes them for factor matrices of >= 4 GB
 *        or >= 2^24 rows; otherwise 32-bit offsets from a scalar base): als_gram_mode 4, the fp32 form of als_wide_kernel;
 *  128 = every nFactors <= 64 takes the padded 16 x 16 fp32 tiles (als_gram_mode 3) instead of the forms specialised for
 *        nFactors 16 / 32 / 48 / 64;
 * 1024 = no bf16 MFMA over three-way split values: nFactors 32 / 64 take the fp32 16 x 16 tiles, 65..128 the fp32 MFMA;
 * 2048 = als_long_solve_kernel adds a long row's partial Gram matrices itself however many there are (default: rows of more
 *        than eight chunks go through als_partial_reduce_kernel first; the two are equal in every bit). */
void gorse_hip_test_set_als_path(int32_t path);
/* thresholds of the Gram-form row plan, for handles created AFTERWARDS: rows longer than long_row feedbacks
 * are cut into chunks of `chunk` entries; <= 0 restores the library's choice (round 5: by the side's size -- the even
 * share of one of ~4096 wave slots, a power of two between 256 (512 from nFactors 64 on) and 4096; chunk = the
 * threshold).  Lets small test inputs exercise the long-row path. */
void gorse_hip_test_set_als_plan(int32_t long_row, int32_t chunk);
/* probe: samples per chunk of a gorse_mf handle created AFTERWARDS (0 = the library's choice: 32 x users, clamped to
 * [4M, 128M]); the user-run schedule applies a chunk at a time. */
void gorse_hip_test_set_bpr_chunk(int64_t samples);
/* which item updates of the user-run BPR kernel may take the STORE route (csrc/bpr_update_users.hip NEG_STORE): bit 0 = the NEGATIVE item of a
 * sample, when its class is "cold", is updated by one write-through store of fma(t, lr, row) instead of d atomic dwords (the
 * reference's own unlocked write, model.go:478-488; its row is then gathered one sample ahead instead of two); < 0 = the
 * library's default.  Only bit 0 is looked at: the forms that bits 1 and 2 once asked for (the positive item by store, the store
 * adding to a row re-read in the same iteration) were measured, rejected and removed, and a value that sets them runs what bit 0
 * alone selects.  Which items are cold is fixed at gorse_mf_create (gorse_hip_test_set_bpr_cold_window). */
void gorse_hip_test_set_bpr_store_mode(int32_t store_mode);
/* floats.MM (csrc/sgemm.hip): 1 = the NN / TN / TT chains on the vector ALU whatever the shape (default: on the fp32 MFMA from 64 x 64
 * results on; both are the same l-ascending fmaf chain, bit for bit).  The second hook returns the kernel time of the last
 * gorse_hip_sgemm call in milliseconds (hipEvents around the launch, copies excluded): bench.py's `mm` object. */
void gorse_hip_test_set_sgemm_valu(int32_t on);
double gorse_hip_test_sgemm_last_ms(void);
/* which kernel family the last gorse_hip_sgemm / gorse_hip_sgemm_device call of this process launched, recorded on the host where
 * sgemm_on_device chooses it (no device code): one of NONE (m or n == 0, k == 0 outside the NT case, or the call was refused), NT
 * (one AVX512-order dot per element), VALU (sgemm_chain_kernel), MFMA64 / MFMA128 (sgemm_mfma_kernel on 64 x 64 / 128 x 128 tiles),
 * or'ed with IN_PLACE when the MFMA kernel ran on the caller's operands where they lie (whole tiles, k a multiple of 16) and with
 * NT_LONG when the NT rows were longer than the LDS staging takes (k > 512) and were read from global memory.  A test asserts the
 * form it was written for, so that a moved threshold cannot leave it testing another kernel. */
#define GORSE_TEST_SGEMM_NONE 0
#define GORSE_TEST_SGEMM_NT 1
#define GORSE_TEST_SGEMM_VALU 2
#define GORSE_TEST_SGEMM_MFMA64 3
#define GORSE_TEST_SGEMM_MFMA128 4
#define GORSE_TEST_SGEMM_IN_PLACE 0x100
#define GORSE_TEST_SGEMM_NT_LONG 0x200
int32_t gorse_hip_test_sgemm_last_form(void);
/* test hook: runs the user-run schedule's preparation of ONE chunk (user draws, counting sort of the sample ids by user, item
 * draws by run: csrc/bpr_prepare.hip bpr_launch_prepare_users) for samples [sample_base, sample_base + n) and returns the run offsets
 * (off[u] .. off[u + 1] = the positions of user u's samples; off[U] .. off[U + 1] = samples whose user draw failed) and the
 * (positive, negative) pair at every position; a pair of -1 = no negative found.  The multiset of triplets equals what
 * gorse_bpr_sample_triplets returns for the same range. */
int32_t gorse_hip_test_bpr_prepare_chunk(gorse_mf *h, int64_t n, uint64_t seed, uint64_t epoch, int64_t sample_base,
                                         int32_t *off /*U + 2, host*/, int32_t *si /*n, host*/, int32_t *sj /*n, host*/);
/* the binned preparation finishes a bin in one LDS-resident pass (csrc/bpr_prepare.hip bpr_bin_finish_kernel): *samples = the samples of a
 * bin that pass holds (a larger bin goes through it a slice at a time), *row_entries = the entries of a bin's users' rows it copies
 * into LDS at most (longer ranges are read from global memory).  GORSE_TEST_BPR_THREE_KERNELS of gorse_hip_test_set_variant: the three
 * kernels that pass replaces (sort, item draws, grouping), whatever the shape.  Results never depend on either beyond the order of the
 * samples in runs of fewer than 3 or more than 1024. */
void gorse_hip_test_bpr_finish_capacities(int32_t *samples, int32_t *row_entries);
/* the handle's counter of BPR samples given up on (no user with feedback or no negative within the draw limit), after its streams
 * drain: every sampler and preparation kernel raises it once per such sample; it is never reset by them (the evaluation's negative
 * sampler zeroes it), so a test reads it before and after. */
int32_t gorse_hip_test_bpr_fail_count(gorse_mf *h, int32_t *count /*host*/);
/* items expected to be touched (as a positive: their share of the feedback; as a negative: 1 / items) less than once per
 * `samples` samples are of class "cold" in handles created AFTERWARDS; 0 = no cold items (every update an atomic). */
void gorse_hip_test_set_bpr_cold_window(int64_t samples);
/* hot-row replicas of the Hogwild BPR schedules (csrc/bpr_fold.hpp HotRows, csrc/hot_rows.hpp).  Handles created AFTERWARDS give a hot item
 * R = the smallest power of two >= (its expected updates per sample) / unit replica rows, 1 .. 8; unit <= 0 = the library's default.
 * Results never depend on it beyond the Hogwild race itself. */
void gorse_hip_test_set_bpr_replica_unit(double unit);
/* wall-clock ticks (100 MHz) from one folder pass to the next in the update launches that follow; <= 0 = the library's default. */
void gorse_hip_test_set_bpr_fold_period(int32_t ticks);
/* after the handle's streams drain: out3[0] = folder passes of the last update launch with folders (its final pass included; folder
 * workgroup 0's count), [1] = hot items, [2] = replica rows in all (the sum of their R).  Bytes one pass moves: (out3[2] exchanged +
 * out3[1] added) x nFactors x 4. */
int32_t gorse_hip_test_bpr_fold_stats(gorse_mf *h, int64_t *out3 /*host*/);
/* the hot slots of a handle, after its streams drain: items[s] = the slot's item (ascending), replicas[s] = its R (the rows of slot s
 * follow those of slot s - 1), rep = every replica row (sum of R x nFactors floats; all zero between two update launches).  Any of the
 * three may be NULL. */
int32_t gorse_hip_test_bpr_hot_state(gorse_mf *h, int32_t *items /*host*/, int32_t *replicas /*host*/, float *rep /*host*/);
/* The accumulated tier (csrc/hot_rows.hpp acc_rows_layout, csrc/bpr_fold.hpp): on a handle that takes the user-run schedule natively, has
 * no cold item at create and whose item factors fit 4 MiB, every warm item has ONE accumulator row behind the replica rows; the
 * workers add its updates there and folder workgroups of the tier's own add the rows to Q every `periods` fold periods.  The two hooks
 * above keep reporting the hot tier only.
 * set_bpr_acc_rows: handles created AFTERWARDS get the tier where eligible (1) or never (0: the classes and launches of the library
 * without it); < 0 = the library's default.  set_bpr_acc_fold_every: fold periods between two passes of the tier's folders in the
 * update launches that follow; <= 0 = the library's default.
 * acc_state, after the handle's streams drain: items[k] = the item of the tier's k-th row (ascending), rows = the rows (their number
 * x nFactors floats; all zero between two update launches).  Either may be NULL.
 * item_classes, after the handle's streams drain: slot[item] = the class word of every item (hot_code(row, log2 R) of an item whose
 * updates go to replica or accumulator rows, -1 warm, -2 cold); out2 = {rows of the tier, cold items}.  Either may be NULL. */
void gorse_hip_test_set_bpr_acc_rows(int32_t on);
void gorse_hip_test_set_bpr_acc_fold_every(int32_t periods);
int32_t gorse_hip_test_bpr_acc_state(gorse_mf *h, int32_t *items /*host*/, float *rows /*host*/);
int32_t gorse_hip_test_bpr_item_classes(gorse_mf *h, int32_t *slot /*host, items*/, int64_t *out2 /*host*/);
/* The folds of an update launch (csrc/bpr_fold.hpp, above HotRows).  A user-run launch on a handle with the accumulated tier and the store
 * route closed has no worker that writes Q: its folders fold as Q's sole writers, with loads and stores (Q <- the row as the launch
 * found it + the slot's rows); every other launch folds with atomics.
 * fold_tier_stats, after the handle's streams drain: out6 = {folder passes of the hot tier in the last update launch with folders
 * (its final pass included; the tier's first workgroup's count), the same of the accumulated tier (0 without it), hot items, replica
 * rows in all, rows of the accumulated tier, 1 where that launch folded as sole writer / 0 with atomics}.  Atomic dwords the folds of
 * an atomic-form launch issue: hot passes x (out6[3] + out6[2]) x nFactors + tier passes x 2 x out6[4] x nFactors (its last pass
 * counts in both); of a sole-writer launch: (out6[3] + out6[4]) x nFactors, the exchanges of its last pass.
 * set_bpr_folder_timeout: wall-clock ticks (100 MHz) after which the folders of the launches that follow stop waiting for the workers
 * and make their last pass; <= 0 = the library's default (10 s).  At 1 tick they make it at once: what the workers add afterwards
 * stays in the rows, and the next launch folds it in. */
int32_t gorse_hip_test_bpr_fold_tier_stats(gorse_mf *h, int64_t *out6 /*host*/);
void gorse_hip_test_set_bpr_folder_timeout(int64_t ticks);
/* gorse_mf_recommend (csrc/recommend.hip).  slices > 0 = the threshold kernel cuts the items into this many slices across workgroups
 * (at most 8 and at most one per item; 0 = by the number of query blocks); buffer > 0 = entries of a query's survivor buffer (raised to
 * k + 2 where smaller, the smallest that can hold k + 1 entries and one more: a compaction per survivor; 0 = max(32, 2 (k + 1)));
 * literal_chunk > 0 = candidates materialised per launch of the literal path at most (0 = 2^22).  Results never depend on them. */
void gorse_hip_test_set_recommend(int32_t slices, int32_t buffer, int64_t literal_chunk);
/* gorse_fm_rank_users (csrc/fm_rank.hip), calls AFTERWARDS: round_rows > 0 = rows of a launch round at most (raised to the call's
 * batch_size where smaller: a slice is never split; 0 = by the scratch budget); sort_cap > 0 = entries of the longest list the
 * device sorts (at most 4096, the default; longer lists are sorted by the host).  Results never depend on them. */
void gorse_hip_test_set_fm_rank(int64_t round_rows, int32_t sort_cap);
/* the ranking step of gorse_fm_rank_users alone, on scores the caller supplies (any bit patterns: signed zeros, NaNs of either
 * sign and any payload, infinities): order_out as that call defines it, lists beyond the cap by the host */
int32_t gorse_hip_test_fm_rank_sort(gorse_fm *h, int64_t n_users, const int64_t *cand_indptr /*host, n_users+1*/,
                                    const float *scores /*host*/, int32_t *order_out /*host*/);
/* gorse_fm_evaluate (csrc/fm_eval.hip), calls AFTERWARDS: round_rows > 0 = rows of a launch round at most (raised to the call's
 * batch_size where smaller: a slice is never split; 0 = by the scratch budget); sort_tile > 0 = keys per workgroup of the radix
 * sort (0 = 4096).  Results never depend on them. */
void gorse_hip_test_set_fm_evaluate(int64_t round_rows, int32_t sort_tile);
/* the metric stage of gorse_fm_evaluate alone, on logits the caller supplies (any bit patterns): counts and auc_sum as that call
 * defines them */
int32_t gorse_hip_test_fm_auc(gorse_fm *h, const float *pos /*host*/, int64_t n_pos, const float *neg /*host*/, int64_t n_neg,
                              int64_t *counts /*host, GORSE_FM_EVAL_COUNTS entries*/, float *auc_sum /*host*/);
/* device milliseconds of the handle's last gorse_fm_evaluate by stage: scoring | keys, sort and per-positive counts | the chain */
int32_t gorse_hip_test_fm_evaluate_times(gorse_fm *h, double *ms3 /*host*/);
/* device milliseconds of the handle's last gorse_mf_evaluate / _resident by stage: the per-user kernel | the sum chain */
int32_t gorse_hip_test_mf_evaluate_times(gorse_mf *h, double *ms2 /*host*/);
/* the two tables the evaluation kernel reads, filled as the library fills them (no device needed): inv_log[i] = 1 / log2f(i + 2)
 * for i < n, idcg[k] = inv_log[0] + ... + inv_log[k - 1] for k <= n (n + 1 entries); n <= GORSE_MF_EVAL_MAX_TOPK */
int32_t gorse_hip_test_mf_evaluate_tables(float *inv_log /*host, n*/, float *idcg /*host, n + 1*/, int32_t n);
/* gorse_nbr_recommend (csrc/nbr_recommend.hip), calls AFTERWARDS: lds_slots > 0 = slots of the largest LDS table (at most the
 * library's 13056; a query takes the LDS path when its bound + 1 fits), so that small inputs reach the global path; query_chunk > 0 =
 * queries per launch at most, so that they run the launch loop.  0 restores the library's choice.  Results never depend on them. */
void gorse_hip_test_set_nbr(int32_t lds_slots, int64_t query_chunk);

#ifdef __cplusplus
}
#endif
#endif /* GORSE_HIP_TEST_H */
