/*
 * gorse_hip.h -- C ABI of libgorse_hip.so, the MI355X (gfx950) implementation of
 * Gorse's collaborative-filtering training and exact embedding top-k hot path.
 *
 * This is the drop-in boundary: exactly what a cgo file built with
 * `//go:build cgo && hip` inside the reference's packages model/cf, common/ann and
 * common/floats would bind (see INTEGRATION.md for the Go stubs).  The reference has
 * no FFI for this path today; its precedent is the cgo BLAS binding
 * common/blas/blas_openblas.go:19-26 (pointer to the first element of a flat Go
 * slice, synchronous call, nothing retained) and build-tag twins such as
 * model/ctr/fm.go vs fm_xla.go.  The same conventions hold here:
 *
 *   - plain C, no C++/torch types; every pointer marked "host" is caller-owned host
 *     memory that is only read/written for the duration of the call (never retained,
 *     so Go's cgo pointer rules are met); pointers marked "device" are HIP device
 *     addresses on the handle's device;
 *   - every function returns int32: 0 = ok, <0 = error (gorse_hip_last_error() gives a
 *     thread-local message).  Where the reference panics (slice length mismatch) or
 *     returns an error (ann.Bruteforce.SearchIndex out of range) the matching code is
 *     returned and nothing is modified;
 *   - one handle = one GPU.  Multi-GPU = one handle per GPU, in one process (the Go master: one goroutine
 *     per GPU) or in several; the exchange between the replicas runs INSIDE the library over RCCL
 *     (gorse_comm_*, gorse_mf_item_allreduce, gorse_mf_rows_allgather below).  The gorse_mf_item_delta_*
 *     calls remain for a caller that brings its own collective;
 *   - calls on one handle must be serialised by the caller (the Go side holds a mutex,
 *     as logics/vector_writer.go does); different handles are independent;
 *   - long calls poll a caller-supplied cancel flag between kernel launches, the
 *     equivalent of ctx.Err() checks in common/parallel/parallel.go:36-38.
 */
#ifndef GORSE_HIP_H
#define GORSE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GORSE_HIP_ABI_VERSION 1

/* return codes */
#define GORSE_OK 0
#define GORSE_ERR_INVALID (-1)   /* bad argument (a Go panic in the reference, e.g. floats.go:96-99) */
#define GORSE_ERR_HIP (-2)       /* HIP runtime / launch failure */
#define GORSE_ERR_CANCELLED (-3) /* cancel flag observed: ctx.Err() != nil, model/cf/model.go:490-493 */
#define GORSE_ERR_NO_DEVICE (-4) /* no usable gfx950 device */
#define GORSE_ERR_RANGE (-5)     /* "index out of range", common/ann/bruteforce.go:41-43 */
#define GORSE_ERR_NOMEM (-6)

/* BPR update schedules (gorse_bpr_epoch / gorse_bpr_apply_triplets `mode`) */
#define GORSE_BPR_HOGWILD_ATOMIC 0 /* Jobs > 1, NO lost item update: all samples of a chunk in flight.  User rows are  *
                                    * updated exactly (one group owns a user's run), every item row by fp32 atomics     *
                                    * (hot items through replica rows)                                                   */
#define GORSE_BPR_SEQUENTIAL 1     /* dependency-levelled: bit-faithful to the reference with Jobs = 1  */
#define GORSE_BPR_HOGWILD_RACY 2   /* write-through load/fma/store, lost updates like the CPU Hogwild   */
#define GORSE_BPR_HOGWILD_STORES 3 /* the schedule Fit runs with Jobs > 1 (the reference's own Hogwild semantics):       *
                                    * GORSE_BPR_HOGWILD_ATOMIC, except that the NEGATIVE item of a sample, when it is a  *
                                    * COLD item (expected to be touched less than once per cold window of samples, see   *
                                    * gorse_mf_set_bpr_cold_window; default 32768), is updated by the reference's own    *
                                    * unlocked load / fma / store (model.go:478-488): such a write can overwrite a       *
                                    * concurrent update of the same row, as two of the reference's workers can (measured *
                                    * at C3: 4 % of the cold rows' updates, NDCG@10 unchanged).      *
                                    * Where the handle has no cold item, or runs the per-sample schedule, it IS mode 0.  */

/* top-k element types and metrics */
#define GORSE_DTYPE_F32 0
#define GORSE_DTYPE_BF16 1      /* uint16 = upper half of the fp32 word, common/bfloats/bfloats.go:24-30 */
#define GORSE_METRIC_NEG_DOT 0  /* distance = -floats.Dot        (logics/cf.go:32-34)                     */
#define GORSE_METRIC_EUCLIDEAN 1 /* distance = floats.Euclidean  (common/ann/ann_test.go)                  */
#define GORSE_METRIC_COSINE 2   /* distance = 1 - a.b/(|a||b|)   (storage/vectors/database.go:29-33)      */
#define GORSE_METRIC_EUCLIDEAN_BF16 3 /* distance = bfloats.Euclidean (common/bfloats/bfloats.go:49-57; the summation order
                                       * of src/bfloats_avx512.c:26-59: 16 unfused partials added one after the other, fused
                                       * scalar tail); bf16 indexes only                                                    */

typedef struct gorse_mf gorse_mf;     /* one matrix-factorisation model resident on one GPU */
typedef struct gorse_topk gorse_topk; /* one exact nearest-neighbour index resident on one GPU */

/* ---- library ------------------------------------------------------------------- */
int32_t gorse_hip_abi_version(void);
const char *gorse_hip_last_error(void);
int32_t gorse_hip_device_count(int32_t *n);

/* ---- cf.MatrixFactorization state (model/cf/model.go:118-127) ------------------------
 * U users, I items, d = nFactors.  user_indptr[U+1] / user_indices[nnz] are
 * dataset.CFSplit.GetUserFeedback() flattened IN STORED ORDER (dataset/dataset.go:231-240);
 * item_indptr / item_indices are GetItemFeedback() likewise and may be NULL when only BPR
 * is run.  The library keeps its own device copies (plus a row-sorted copy of the user
 * rows for the negative sampler's membership test, model.go:461-468). */
int32_t gorse_mf_create(gorse_mf **h, int32_t device, int64_t U, int64_t I, int32_t d,
                        const int64_t *user_indptr /*host*/, const int32_t *user_indices /*host*/,
                        const int64_t *item_indptr /*host or NULL*/, const int32_t *item_indices /*host or NULL*/);
int32_t gorse_mf_destroy(gorse_mf *h);

/* BaseMatrixFactorization.UserFactor / ItemFactor as flat row-major U*d / I*d float32.
 * Either pointer may be NULL to skip that matrix. (Init draws stay on the Go side:
 * model/cf/model.go:532-540, common/util/random.go:45-60.) */
int32_t gorse_mf_set_factors(gorse_mf *h, const float *P /*host*/, const float *Q /*host*/);
int32_t gorse_mf_get_factors(gorse_mf *h, float *P /*host*/, float *Q /*host*/);

/* internalPredict for n (user, item) index pairs, model/cf/model.go:195-203:
 * out[t] = floats.Dot(UserFactor[u[t]], ItemFactor[items[t]]) in the reference's AVX512
 * operation order, 0 when either index is negative. */
int32_t gorse_mf_score(gorse_mf *h, const int32_t *u /*host*/, const int32_t *items /*host*/, int64_t n,
                       float *out /*host*/);

/* cf.Rank for many users at once, model/cf/evaluator.go:162-169: user users[t] ranks the
 * candidates cand[cand_indptr[t] .. cand_indptr[t+1]) through heap.TopKFilter(topk)
 * (common/heap/filter.go:23-59, Go container/heap tie behaviour).  rank_out is
 * n_users*topk, padded with -1; rank_len[t] = number of valid entries. */
int32_t gorse_mf_rank(gorse_mf *h, int64_t n_users, const int32_t *users /*host*/, const int64_t *cand_indptr /*host*/,
                      const int32_t *cand /*host*/, int32_t topk, int32_t *rank_out /*host*/, int32_t *rank_len /*host*/);

/* Every user's k best UNSEEN items, straight from the resident model: the bulk form of worker/pipeline.go:403-448
 * (updateCollaborativeRecommend), without its over-fetch.  For query t with user u = users[t] (users == NULL: u = t, and n_users must
 * not exceed the handle's users) the candidates are the items i of [0, I), ascending, with
 *   - item_ok[i] != 0 (item_ok == NULL: the item has at least one training feedback in the handle = IsItemPredictable, what
 *     master/tasks.go:942 publishes),
 *   - i not in u's training row held by the handle,
 *   - i not in seen_items[seen_indptr[t] .. seen_indptr[t + 1]) (seen_indptr == NULL: no such rows; a row may be unsorted, repeat an
 *     item and overlap the training row),
 * and the result row is exactly what gorse_mf_rank returns for (u, that list, k): heap.TopKFilter(k) fed in ascending item order and
 * popped descending, Go container/heap tie behaviour included.  items_out is n_users * k padded with -1, scores_out n_users * k padded
 * with 0 and holds the bits of gorse_mf_score, count_out[t] = min(k, number of candidates); each may be NULL.  u < 0 gives count 0.
 * u >= U or a seen item outside [0, I): GORSE_ERR_RANGE; k <= 0: GORSE_ERR_INVALID; everything is validated before anything is
 * launched, and an error leaves the outputs untouched.  The call waits for epochs still enqueued on the handle and leaves the
 * factors untouched.
 * Relation to the reference: its per-user list is the CacheSize + |excludeSet| nearest items minus the excluded ones, so it may hold
 * up to |excludeSet| items MORE than CacheSize -- an artefact of the over-fetch.  With k = CacheSize this call returns the prefix of
 * length CacheSize of that list.
 * A query whose k + 1 best candidate scores are pairwise different (as floats, -0 == +0) and that meets no NaN score is answered
 * by the threshold kernel (k <= 256); every other query is answered literally (candidate list -> TopKFilter on the device). */
int32_t gorse_mf_recommend(gorse_mf *h, int64_t n_users, const int32_t *users /*host, or NULL: users[t] = t*/, int32_t k,
                           const uint8_t *item_ok /*host, I bytes, or NULL*/, const int64_t *seen_indptr /*host, n_users+1, or NULL*/,
                           const int32_t *seen_items /*host*/, int32_t *items_out /*host or NULL, n_users*k, padded with -1*/,
                           float *scores_out /*host or NULL, n_users*k, padded with 0*/, int32_t *count_out /*host or NULL, n_users*/);
/* the handle's last gorse_mf_recommend: queries answered by the threshold kernel (queries with u < 0, which need no answer, are
 * counted here) / literally, and the device time of its launches (hipEvents around them, copies excluded) */
int32_t gorse_mf_recommend_stats(gorse_mf *h, int64_t *n_fast, int64_t *n_literal, double *device_ms);

/* dataset.SampleUserNegatives on the device (dataset/dataset.go:242-253 through RandomGenerator.SampleInt32,
 * common/util/random.go:108-132): for EVERY user num_candidates distinct items outside (the user's feedback in the test split
 * given here, union the user's train feedback the handle holds), in draw order -- or ALL remaining items ascending when no
 * more than num_candidates are left (random.go:115-121).  User u draws from its own Philox4x32-10 stream keyed by
 * (seed, "neg", u) through Go's Int31n (the reference's single math/rand stream, seeded 0, is not reproducible: SURVEY.md
 * 8c); the reference passes seed 0.  neg_out (host or NULL) receives U * num_candidates items padded with -1, neg_len (host
 * or NULL) the counts.  The call also leaves, resident on the device, the candidate lists Evaluate ranks
 * (model/cf/evaluator.go:47-53: for each user WITH test feedback, ascending, the test items followed by the negatives):
 * gorse_mf_rank_resident ranks them without any upload -- the Evaluate between two epochs of a Fit. */
int32_t gorse_mf_sample_user_negatives(gorse_mf *h, const int64_t *test_indptr /*host, U+1*/,
                                       const int32_t *test_indices /*host*/, int32_t num_candidates, uint64_t seed,
                                       int32_t *neg_out /*host or NULL*/, int32_t *neg_len /*host or NULL*/);
/* how many users have test feedback / how many candidates their lists hold (sizes of gorse_mf_rank_resident's outputs) */
int32_t gorse_mf_resident_candidates(gorse_mf *h, int64_t *n_users /*out*/, int64_t *n_candidates /*out*/);
/* A number that changes with every gorse_mf_sample_user_negatives on this handle (0 = no lists resident).  A handle may be lent to
 * several models in turn (host/gorse_cf.hpp ResidentDataset): a model remembers the number its own sampling returned and ranks
 * the resident lists only while it still reads the same one. */
int32_t gorse_mf_resident_generation(gorse_mf *h, uint64_t *generation /*out*/);
/* gorse_mf_rank over the resident candidate lists: users_out (host or NULL) n_users ids, rank_out n_users * topk padded with
 * -1, rank_len n_users. */
int32_t gorse_mf_rank_resident(gorse_mf *h, int32_t topk, int32_t *users_out /*host or NULL*/, int32_t *rank_out /*host*/,
                               int32_t *rank_len /*host*/);

/* cf.Evaluate's ranking and metrics on the device (model/cf/evaluator.go:35-160; csrc/mf_eval.hip): per evaluated user the rank
 * list of gorse_mf_rank (every index, ties as container/heap leaves them) and from it the six metrics NDCG, Precision, Recall, HR,
 * MAP, MRR -- in this order everywhere below -- against the user's target row: membership is targetSet.Contains(item), the
 * denominators use the number of DISTINCT targets, every operation is the reference's float32 one in its order.  sums[m] is metric
 * m's float32 running sum over the users in user order (nJobs = 1), *count the float32 number of users counted; the caller forms
 * sums[m] * (1 / count) as floats.MulConst does.  per_user (host or NULL) receives 6 x n_users values, metric-major.
 * topk outside 1 .. GORSE_MF_EVAL_MAX_TOPK: GORSE_ERR_INVALID (the heap's topk + 1 slots live in LDS) -- rank on the device and
 * walk the metrics on the host then. */
#define GORSE_MF_EVAL_MAX_TOPK 128
/* ... over the resident candidate lists gorse_mf_sample_user_negatives left, against the resident test rows: nothing is uploaded,
 * and unless per_user / rank_out / rank_len (gorse_mf_rank_resident's outputs, host or NULL) are asked for, six sums come back.
 * Nothing resident: GORSE_ERR_INVALID, as gorse_mf_rank_resident. */
int32_t gorse_mf_evaluate_resident(gorse_mf *h, int32_t topk, float *sums /*host, 6*/, float *count /*host*/,
                                   float *per_user /*host 6 x n_users, or NULL*/, int32_t *rank_out /*host or NULL*/,
                                   int32_t *rank_len /*host or NULL*/);
/* ... over lists the caller uploads (a test set with preloaded negatives): users, candidate CSR and validation as gorse_mf_rank,
 * targets as a CSR with one row per entry of users.  A user with an empty target row is skipped and not counted
 * (evaluator.go:47); its per_user column holds zeros.  A counted user with no candidates yields the reference's 0 / 0 = NaN. */
int32_t gorse_mf_evaluate(gorse_mf *h, int64_t n_users, const int32_t *users /*host*/, const int64_t *target_indptr /*host*/,
                          const int32_t *targets /*host*/, const int64_t *cand_indptr /*host*/, const int32_t *cand /*host*/,
                          int32_t topk, float *sums /*host, 6*/, float *count /*host*/, float *per_user /*host 6 x n_users, or NULL*/);
/* the handle's last evaluation: users counted, candidates scored, device time of its two kernels (events on the handle's stream) */
int32_t gorse_mf_evaluate_stats(gorse_mf *h, int64_t *users, int64_t *candidates, double *device_ms);

/* ---- BPR, model/cf/model.go:446-494 ------------------------------------------------------
 * One call = n_samples SGD steps (the reference does CountFeedback() per epoch).
 * Sampling (model.go:449-468) runs on the device from a counter-based Philox4x32-10 stream
 * keyed by (seed, epoch, sample_base + sample index) and consumed through Go's Int31n
 * algorithm; gorse_bpr_sample_triplets returns exactly the triplets an epoch call with the
 * same (seed, epoch, sample_base) applies, so a caller (or a test) can replay them.
 * loss_out (may be NULL) receives sum log1p(exp(-diff)), the reference's unused `cost`. */
int32_t gorse_bpr_epoch(gorse_mf *h, int64_t n_samples, float lr, float reg, uint64_t seed, uint64_t epoch,
                        int64_t sample_base, int32_t mode, const volatile int32_t *cancel /*host or NULL*/,
                        double *loss_out /*host or NULL*/);
/* Same, but only enqueues the work on the handle's stream (hogwild modes only). */
int32_t gorse_bpr_epoch_enqueue(gorse_mf *h, int64_t n_samples, float lr, float reg, uint64_t seed, uint64_t epoch,
                                int64_t sample_base, int32_t mode);
/* The cold window of THIS handle (GORSE_BPR_HOGWILD_STORES): item i is cold when (its share of the training feedback + 1 / I) x
 * samples < 1, i.e. when fewer than one touch of its row is expected per `samples` samples in flight.  gorse_mf_create starts
 * from 32768; 0 = no item is cold (mode 3 is then mode 0); takes effect from the next epoch call.  Returns the number of cold
 * items through n_cold (may be NULL). */
int32_t gorse_mf_set_bpr_cold_window(gorse_mf *h, int64_t samples, int64_t *n_cold /*out, may be NULL*/);
/* Which form of the GORSE_BPR_HOGWILD_ATOMIC schedule this handle runs: 1 = user runs (the chunk's samples are
 * counting-sorted by user and one 16-lane group applies all samples of a user with p_u in registers; chosen when
 * there are >= 4096 users and nFactors is 8/16/32/64/128), 0 = one group per sample.  Both apply exactly the triplets
 * gorse_bpr_sample_triplets returns, in a different (Hogwild-legal) order; GORSE_BPR_SCHEDULE=users|samples in the
 * environment overrides the choice. */
int32_t gorse_mf_bpr_schedule(gorse_mf *h, int32_t *user_runs /*out*/);
int32_t gorse_bpr_sample_triplets(gorse_mf *h, int64_t n, uint64_t seed, uint64_t epoch, int64_t sample_base,
                                  int32_t *u /*host*/, int32_t *i /*host*/, int32_t *j /*host*/);
/* Apply a host-supplied triplet stream (test hook and replay path). Triplets with a
 * negative index are skipped. */
int32_t gorse_bpr_apply_triplets(gorse_mf *h, const int32_t *u /*host*/, const int32_t *i /*host*/,
                                 const int32_t *j /*host*/, int64_t n, float lr, float reg, int32_t mode);

/* ---- ALS (eALS), model/cf/model.go:641-738 ------------------------------------------------
 * One call = one epoch: S = sum q q^T over items with feedback, user sweep, S = sum p p^T
 * over users with feedback, item sweep.  Needs item_indptr/item_indices.
 * Arithmetic: fp32 in, fp32 out, every sum in fp32.  For nFactors 32, 64 and 65..128 the PRODUCTS of the per-row Gram matrices are
 * formed on the bf16 matrix unit from an exact three-way split of each float (hi + mid + lo, all bf16): six exact partial products
 * per pair, the three smallest (below 2^-23 of the product) dropped -- as close to a float64 evaluation as the fp32 matrix unit is
 * (DESIGN.md section 4).  GORSE_ALS_GRAM=fp32 in the environment keeps every product on the fp32 unit (about 1.2x the epoch time). */
int32_t gorse_als_epoch(gorse_mf *h, float weight, float reg, const volatile int32_t *cancel /*host or NULL*/);
/* Row-sharded ALS (one process per GPU): every process holds the whole dataset and both factor
 * matrices, solves only user rows [u_begin,u_end) and item rows [i_begin,i_end) (rows are independent inside a
 * half-sweep: model.go:659, 707 hand them to parallel.Parallel), and the caller all-gathers the row blocks after
 * each half.  set_ranges rebuilds the row plans (default after create: all rows); half_epoch(side) = S over ALL
 * rows of the other side + the sweep of the owned rows of `side` (0 = users, model.go:645-690; 1 = items,
 * :693-738); gorse_als_epoch = half 0 then half 1 on the current ranges. */
int32_t gorse_als_set_ranges(gorse_mf *h, int64_t u_begin, int64_t u_end, int64_t i_begin, int64_t i_end);
int32_t gorse_als_half_epoch(gorse_mf *h, int32_t side, float weight, float reg);
/* Same, but only enqueues the kernels on the handle's stream (gorse_mf_rows_allgather is ordered behind them on that stream;
 * gorse_mf_synchronize ends the epoch): what a caller driving several handles from one thread uses, so that the devices
 * solve their row ranges at the same time. */
int32_t gorse_als_half_epoch_enqueue(gorse_mf *h, int32_t side, float weight, float reg);
/* factor rows [begin,end) of side 0 (P) / 1 (Q) -> / <- a device buffer owned by the caller */
int32_t gorse_mf_rows_export(gorse_mf *h, int32_t side, int64_t begin, int64_t end, float *dst /*device*/);
int32_t gorse_mf_rows_import(gorse_mf *h, int32_t side, int64_t begin, int64_t end, const float *src /*device*/);

/* ---- multi-GPU exchange (one process per GPU; Q replicated, users sharded) ------------------
 * mark:   Q_sync <- Q
 * export: dst[I*d] <- Q - Q_sync                 (device buffer owned by the caller)
 * import: Q <- Q_sync + src ; Q_sync <- Q        (src = all-reduced sum of every rank's export) */
int32_t gorse_mf_item_sync_mark(gorse_mf *h);
int32_t gorse_mf_item_delta_export(gorse_mf *h, float *dst /*device*/);
int32_t gorse_mf_item_delta_import(gorse_mf *h, const float *src /*device*/);
/* ---- the same exchanges with RCCL behind the boundary ------------------------------------------------
 * the reference trains in ONE process and one goroutine (master/tasks.go:879-1034), so the
 * multi-GPU path has to be callable from there: a gorse_comm is one rank of an RCCL communicator owned by this
 * library (librccl is dlopen'ed on first use).  Two ways to get the ranks:
 *   one process, N GPUs  : gorse_comm_create_local(comms, devices, N)  -- one handle + one communicator per device,
 *                          every exchange call below receives all N pairs (issued as one RCCL group);
 *   one process per GPU  : rank 0 calls gorse_comm_unique_id and ships the 128 bytes to the others (bench.py: a
 *                          torch.distributed broadcast; Go: whatever RPC the deployment has), every rank calls
 *                          gorse_comm_create(id, world, rank, device) and passes its ONE (handle, communicator) pair.
 * The collectives are enqueued on the handles' own streams between the kernels that fill and consume their buffers:
 * an exchange synchronises nothing with the host.
 *   gorse_mf_item_allreduce : Q <- Q_sync + sum over ranks (Q - Q_sync); Q_sync <- Q   (one all-reduce of I*d fp32;
 *                             gorse_mf_item_sync_mark once before the first epoch)
 *   gorse_mf_rows_allgather : after gorse_als_half_epoch(side): rank r's rows [row_splits[r], row_splits[r+1]) of P (side 0)
 *                             or Q (side 1) reach every replica (one broadcast per owner, grouped; (U or I)*d fp32)
 *   gorse_comm_allreduce_f32: n host floats summed over the ranks in place (metric partial sums of a sharded Evaluate);
 *                             one process per GPU only -- a process holding several ranks uses gorse_comm_allreduce_f32_local */
typedef struct gorse_comm gorse_comm;
#define GORSE_COMM_ID_BYTES 128
int32_t gorse_comm_unique_id(uint8_t *id /*host, GORSE_COMM_ID_BYTES*/);
int32_t gorse_comm_create(gorse_comm **c, const uint8_t *id /*host*/, int32_t world, int32_t rank, int32_t device);
int32_t gorse_comm_create_local(gorse_comm **comms /*out: n*/, const int32_t *devices /*n*/, int32_t n);
int32_t gorse_comm_destroy(gorse_comm *c);
int32_t gorse_comm_info(gorse_comm *c, int32_t *world /*out*/, int32_t *rank /*out*/);
int32_t gorse_mf_item_allreduce(gorse_mf *const *handles, gorse_comm *const *comms, int32_t n);
int32_t gorse_mf_rows_allgather(gorse_mf *const *handles, gorse_comm *const *comms, int32_t n, int32_t side,
                                const int64_t *row_splits /*host, world + 1*/);
int32_t gorse_comm_allreduce_f32(gorse_comm *c, float *buf /*host, in place*/, int64_t n);
/* gorse_comm_allreduce_f32 blocks until EVERY rank has called it: a process that owns several ranks
 * (gorse_comm_create_local) calls this instead, once, with all of them: bufs[i] = rank i's n floats. */
int32_t gorse_comm_allreduce_f32_local(gorse_comm *const *comms, int32_t n_comms, float *const *bufs /*host, in place*/, int64_t n);
/* GORSE_OK when RCCL can be opened in this process.  gorse_comm_create is a collective initialisation: every rank checks
 * this first and the ranks agree on the answers (over whatever carried the unique id) before any of them enters it. */
int32_t gorse_comm_available(void);
/* Raw device addresses of the resident factor matrices (row-major U*d, I*d). */
int32_t gorse_mf_device_ptrs(gorse_mf *h, float **P /*out: device*/, float **Q /*out: device*/);

/* ---- stream / measurement ---------------------------------------------------------------------
 * All work of a handle runs on the handle's own HIP stream(s).  Profiling mode brackets every
 * launch of the dominant kernels with hipEvents on the stream they run on and accumulates
 * (count, milliseconds) per kernel class; bench.py reads these for the roofline line. */
int32_t gorse_mf_synchronize(gorse_mf *h);
/* Epoch pacing for a Fit loop that ENQUEUES its epochs between two evaluations (gorse_bpr_epoch_enqueue).  Replaces two things the
 * reference's loop has for free (model/cf/model.go:446-503): it checks ctx per sample (:449), and it logs the epoch's duration as
 * fit_time (:496-503).
 *   gorse_mf_epoch_throttle: returns once at most max_in_flight of the epochs issued so far are unfinished on the device (0 = all
 *     done), looking at *cancel (host, may be NULL) every ~20 us while it waits: GORSE_ERR_CANCELLED as soon as the flag is set (the
 *     caller then drains with gorse_mf_synchronize, at most max_in_flight + 1 epochs).  A Fit that calls it with 2 in front of every
 *     enqueued epoch still has the next epoch's preparation running under the current update kernel, and sees a cancel within
 *     two epochs instead of within Verbose.
 *   gorse_mf_epoch_times: the DEVICE time of the BPR epochs that have finished since the last reset -- per epoch from the moment the
 *     update stream reaches it (= the end of the previous epoch's last update kernel when epochs follow each other: an epoch enqueued
 *     while its predecessor is in flight takes that one's end event as its begin, so the times of back-to-back epochs add up to the
 *     stream's time) to the end of its own last update kernel: hipEvents on the handle's stream, no host clock -- and how many epochs
 *     are still in flight. */
int32_t gorse_mf_epoch_throttle(gorse_mf *h, int32_t max_in_flight, const volatile int32_t *cancel /*host or NULL*/);
int32_t gorse_mf_epoch_times(gorse_mf *h, int64_t *epochs /*out*/, double *total_ms /*out*/, int64_t *in_flight /*out, may be NULL*/,
                             int32_t reset);
int32_t gorse_mf_set_profiling(gorse_mf *h, int32_t on);
#define GORSE_PROF_BPR_UPDATE 0
#define GORSE_PROF_BPR_SAMPLE 1 /* the sampler kernels (user draws; item draws by run) */
#define GORSE_PROF_ALS_SWEEP 2
#define GORSE_PROF_ALS_GRAM 3
#define GORSE_PROF_BPR_SORT 4 /* counting sort of a chunk's sample ids by USER (scan of the run counters + scatter) */
#define GORSE_PROF_COMM 5 /* the RCCL collectives of gorse_mf_item_allreduce / gorse_mf_rows_allgather          */
#define GORSE_PROF_NCLASSES 6
int32_t gorse_mf_get_profile(gorse_mf *h, int32_t kernel_class, int64_t *launches, double *total_ms);
int32_t gorse_mf_reset_profile(gorse_mf *h);

/* ---- exact top-k: ann.Index / ann.Bruteforce, common/ann/ann.go:21-25, bruteforce.go:24-83 ----
 * X is N x d row-major, float32 or bf16 (uint16).  Search results follow the reference
 * exactly: the k smallest distances kept in a max-heap (pq.go), Reverse(), popped ascending;
 * ties resolved as Go's container/heap resolves them; prune0 drops results with distance <= 0.
 * idx_out / dist_out are nq*k, padded with -1 / +inf; count_out[t] = valid entries. */
int32_t gorse_topk_create(gorse_topk **h, int32_t device, int64_t N, int32_t d, int32_t dtype, int32_t metric,
                          const void *X /*host*/);
int32_t gorse_topk_destroy(gorse_topk *h);
/* Bruteforce.SearchIndex for nq stored vectors q[t] (the vector itself is excluded, i != q). */
int32_t gorse_topk_search_index(gorse_topk *h, const int64_t *q /*host*/, int64_t nq, int32_t k, int32_t prune0,
                                int32_t *idx_out /*host*/, float *dist_out /*host*/, int32_t *count_out /*host*/);
/* Bruteforce.SearchVector for nq query vectors (nq x d, same dtype as the index). */
int32_t gorse_topk_search_vector(gorse_topk *h, const void *qv /*host*/, int64_t nq, int32_t k, int32_t prune0,
                                 int32_t *idx_out /*host*/, float *dist_out /*host*/, int32_t *count_out /*host*/);
/* SearchIndex for every stored vector q in [q_begin, q_end): the item-to-item bulk build.
 * Results stay on the device unless host pointers are given (either may be NULL). */
int32_t gorse_topk_all_pairs(gorse_topk *h, int64_t q_begin, int64_t q_end, int32_t k, int32_t *idx_out /*host or NULL*/,
                             float *dist_out /*host or NULL*/);
/* ---- triangle-sharded all-pairs search over W GPUs (top-k row) -----------------------------------------------------
 * gorse_topk_all_pairs over the stored rows [q_begin, q_end) takes the SYMMETRIC form of the sweep: every score of the square block
 * serves both of its queries.  Sharding the QUERY ROWS over W ranks keeps that saving on each rank's diagonal square only; these
 * calls shard the TRIANGLE instead -- rank r sweeps the query blocks (512 queries) C with C % W == r -- so the W ranks together do
 * exactly the single-rank sweep.  One handle per rank, every rank holds the whole index; the calls of one search, in order:
 *   gorse_topk_tri_begin            the search's buffers + the PILOT sweeps of this rank's slice of the queries (slice r of W, whole
 *                                   blocks); GORSE_ERR_INVALID when the search has no symmetric form (shard its query rows then)
 *   gorse_topk_tri_slice            which queries a rank's pilots cover, how many queries it owns (arithmetic: any rank can be asked)
 *   gorse_topk_tri_thresholds_get / _put   the pilot thresholds of a slice out of / into the handle: an ALL-GATHER of 4 bytes per
 *                                   query, every rank must hold all of them before ...
 *   gorse_topk_tri_sweep            ... the main sweep of this rank's blocks: own lists, and foreign lists for EVERY earlier block's rows
 *   gorse_topk_tri_pack(dest) / _pack_read   the foreign lists this rank holds for the queries `dest` owns, as one message: a count per
 *                                   owned query (-1: the sender's part overflowed), then the (key, row) entries end to end
 *   gorse_topk_tri_unpack(src, ...) a message from `src` appended to this rank's own queries' foreign lists: an ALL-TO-ALL of ~130
 *                                   entries x 8 bytes per query in all
 *   gorse_topk_tri_finish           exact rescoring + tie path for the queries this rank owns; their rows are written into the
 *                                   caller's nq x k arrays (the other rows are left alone; NULL = results stay on the device)
 * The exchange itself is the caller's (integration/go/common/ann/bruteforce_hip.go: RCCL; gorse_amd/dist.py: torch.distributed,
 * or host memory when the ranks are emulated on one device): every buffer that crosses this boundary may be HOST OR DEVICE memory.
 * Results are those of gorse_topk_all_pairs, row for row, bit for bit (tests/test_gpu_topk_tri.py). */
int32_t gorse_topk_tri_begin(gorse_topk *h, int64_t q_begin, int64_t q_end, int32_t k, int32_t rank, int32_t world);
int32_t gorse_topk_tri_slice(gorse_topk *h, int32_t rank, int64_t *lo /*out*/, int64_t *hi /*out*/, int64_t *owned /*out*/);
int32_t gorse_topk_tri_thresholds_get(gorse_topk *h, int64_t lo, int64_t hi, float *dst /*host or device*/);
int32_t gorse_topk_tri_thresholds_put(gorse_topk *h, int64_t lo, int64_t hi, const float *src /*host or device*/);
int32_t gorse_topk_tri_sweep(gorse_topk *h);
int32_t gorse_topk_tri_pack(gorse_topk *h, int32_t dest, int64_t *n_counts /*out*/, int64_t *n_entries /*out*/);
int32_t gorse_topk_tri_pack_read(gorse_topk *h, int32_t *counts /*host or device, n_counts*/, uint64_t *entries /*host or device, n_entries*/);
int32_t gorse_topk_tri_unpack(gorse_topk *h, int32_t src, const int32_t *counts, int64_t n_counts, const uint64_t *entries,
                              int64_t n_entries);
int32_t gorse_topk_tri_finish(gorse_topk *h, int32_t *idx_out /*host nq x k or NULL*/, float *dist_out /*host nq x k or NULL*/);
/* ONE process that holds all n handles (one per GPU of a node -- the Go master's mode -- or n on one device: the emulation the tests
 * run): the whole sequence above in one call, both exchanges as device-to-device copies between the handles.  hs[r] is rank r; every
 * handle holds the same index.  idx_out / dist_out: all nq x k rows (every rank writes the rows it owns), or NULL. */
int32_t gorse_topk_tri_all_pairs_local(gorse_topk **hs, int32_t n, int64_t q_begin, int64_t q_end, int32_t k, int32_t *idx_out /*host or NULL*/,
                                       float *dist_out /*host or NULL*/);
int32_t gorse_topk_synchronize(gorse_topk *h);
#define GORSE_PROF_TOPK_SCORE 0   /* path A: dist_kernel (pair-at-a-time scan in the reference's order)      */
#define GORSE_PROF_TOPK_RESCORE 1 /* path A: select_fast_kernel (+ the literal container/heap select_kernel)    */
#define GORSE_PROF_TOPK_SWEEP 2   /* path B: topk_sweep_kernel (bf16 MFMA candidate sweep + threshold filter) */
#define GORSE_PROF_TOPK_SELECT 3  /* path B: topk_rescore_kernel (exact rescoring + ranking of the lists)     */
#define GORSE_PROF_TOPK_HIST 4    /* path B: history sweep of the queries with ties in their top k+1           */
#define GORSE_PROF_TOPK_REPLAY 5  /* path B: topk_tie_sort_kernel + topk_tie_replay_kernel (literal heap replay) */
int32_t gorse_topk_set_profiling(gorse_topk *h, int32_t on);
int32_t gorse_topk_get_profile(gorse_topk *h, int32_t kernel_class, int64_t *launches, double *total_ms);
/* admissible[r] == 0 removes row r from every later search -- as if ann.Bruteforce held the admissible rows only (their ids
 * unchanged): what IsHidden and the categories filter of storage/vectors/xvec.go:386-394 need, evaluated by the caller once
 * per filter instead of an over-fetch loop around the search.  NULL = all rows (the default).  The mask is applied inside the
 * candidate sweep (a masked row scores NaN) and in the literal scan. */
int32_t gorse_topk_set_mask(gorse_topk *h, const uint8_t *admissible /*host, N bytes, or NULL*/);
/* statistics of the last all_pairs / search call: queries that took the exact fallback path */
int32_t gorse_topk_last_stats(gorse_topk *h, int64_t *n_fallback, int64_t *n_tie_resolved);

/* ---- exact sparse top-k: the sparse collections of vectors.Database --------------------------------
 * storage/vectors/database.go:90-97 (Vector.Indices / Values), xvec.go:241-247 (dimension 0 = sparse, distance Dot
 * only, Flat = exact index), filled by the IDF item-to-item / user-to-user writers of logics/vector_writer.go:192-209
 * (ascending ids, value sqrt(idf)) and queried by logics/item_to_item.go:50-88.
 * N stored vectors as CSR: indptr[N+1], indices[nnz] STRICTLY ASCENDING inside a row, values[nnz].
 * Score of (query, row) = sum over the common indices, in ascending index order, of q_value * x_value, each product
 * and each addition rounded to float32 (no fused multiply-add); a row sharing no index scores 0.  Results per query
 * are what QueryVectors returns (xvec.go:379-446): all admissible rows ranked by score, descending (equal scores in
 * ascending row order: the reference's Flat index is a third-party module whose tie order no test pins), cut to k, and
 * the rows with Score == 0 dropped AFTER the cut (xvec.go:419-421; TestSparse, database_test.go:217-224: the disjoint
 * vector is not returned).  With positive values -- all the IDF writers produce -- that is simply the k best rows
 * sharing an index with the query.  idx_out / score_out are nq*k padded with -1 / -inf, count_out[t] = valid entries. */
typedef struct gorse_sparse gorse_sparse;
int32_t gorse_sparse_create(gorse_sparse **h, int32_t device, int64_t N, const int64_t *indptr /*host*/,
                            const uint32_t *indices /*host*/, const float *values /*host*/);
int32_t gorse_sparse_destroy(gorse_sparse *h);
/* admissible[r] == 0 removes row r from every later result (IsHidden / the categories CONTAIN_ALL filter of
 * xvec.go:379-446 evaluated by the caller); NULL = all rows admissible (the default). */
int32_t gorse_sparse_set_mask(gorse_sparse *h, const uint8_t *admissible /*host, N bytes, or NULL*/);
/* nq query vectors as CSR (same ordering rule as the stored rows; indices the index never saw match nothing).
 * exclude[t] (array may be NULL, entries may be -1) is a stored row treated as absent for query t. */
int32_t gorse_sparse_search(gorse_sparse *h, int64_t nq, const int64_t *q_indptr /*host*/,
                            const uint32_t *q_indices /*host*/, const float *q_values /*host*/,
                            const int64_t *exclude /*host or NULL*/, int32_t k, int32_t *idx_out /*host*/,
                            float *score_out /*host*/, int32_t *count_out /*host*/);
/* every stored row q in [q_begin, q_end) as a query (the item-to-item / user-to-user refresh): exclude_self != 0
 * treats row q as absent from its own ranking.  Host pointers may be NULL (results stay on the device).
 * A call over ALL rows with exclude_self and no mask walks every pair of ordinary rows once and delivers the score to both
 * rankings (the same products in the same order: the same bits; csrc/sparse_kernels.hpp, SymArgs) -- results identical to
 * any other way of asking, ~2 KB of device scratch per row.  The handle keeps the work plan of its last all-pairs call. */
int32_t gorse_sparse_all_pairs(gorse_sparse *h, int64_t q_begin, int64_t q_end, int32_t k, int32_t exclude_self,
                               int32_t *idx_out /*host or NULL*/, float *score_out /*host or NULL*/,
                               int32_t *count_out /*host or NULL*/);
int32_t gorse_sparse_synchronize(gorse_sparse *h);
/* measurement: hipEvent pairs around sparse_tile_kernel (+ the merge of split queries) on the handle's stream, and the
 * work of the last call: postings = sum over its queries and their indices of the posting-list lengths (= multiply-adds
 * performed; the kernel reads 8 bytes per posting); hits = (query, row) pairs with a non-zero inner product. */
int32_t gorse_sparse_set_profiling(gorse_sparse *h, int32_t on);
int32_t gorse_sparse_get_profile(gorse_sparse *h, int64_t *launches, double *total_ms);
int32_t gorse_sparse_last_stats(gorse_sparse *h, int64_t *postings, int64_t *hits);

/* ---- floats.MM / blas.SGEMM, common/floats/floats.go:241, mm.go:19-49 ------------------------
 * Row-major C(m x n) = op(A) op(B) with the reference's own semantics: the NN, TN and TT
 * cases ACCUMULATE into C, the NT case overwrites it (mm.go:20-48, floats_avx512.c:443-480).
 * The NT case takes k <= 8192 (every such k gives floats.Dot's bits; k = 0 writes +0); a larger
 * k is GORSE_ERR_INVALID and leaves C alone.  The other three cases have no bound on k. */
int32_t gorse_hip_sgemm(int32_t device, int32_t transA, int32_t transB, int32_t m, int32_t n, int32_t k,
                        const float *a /*host*/, int32_t lda, const float *b /*host*/, int32_t ldb, float *c /*host*/,
                        int32_t ldc);
/* the same product on matrices that already lie in the memory of `device` (a caller that keeps its operands resident pays no
 * PCIe transfer); synchronous: C is complete when the call returns */
int32_t gorse_hip_sgemm_device(int32_t device, int32_t transA, int32_t transB, int32_t m, int32_t n, int32_t k,
                               const float *a /*device*/, int32_t lda, const float *b /*device*/, int32_t ldb, float *c /*device*/,
                               int32_t ldc);


/* ---- ctr.AFM: the factorization machine (model/ctr/fm.go:111-126); its item-embedding branch follows below --------------
 * n_features = dataset index length, d = nFactors in 1..128.  Parameters: bias B, linear W (n_features), pairwise V
 * (n_features x d, row-major), initialised by the caller (fm.go:247-270: the Go side draws them) and read back into the nn
 * tensors.  Samples are n x width matrices of feature indices and (already scaled) values, positions past a row's length
 * hold index 0 with value 0 (convertToTensors, fm.go:527-577); an index outside [0, n_features) is GORSE_ERR_RANGE. */
typedef struct gorse_fm gorse_fm;
#define GORSE_OPT_SGD 0  /* nn.SGD  (common/nn/optimizers.go:70-84)   */
#define GORSE_OPT_ADAM 1 /* nn.Adam (common/nn/optimizers.go:118-156) */
int32_t gorse_fm_create(gorse_fm **h, int32_t device, int64_t n_features, int32_t n_factors);
int32_t gorse_fm_destroy(gorse_fm *h);
/* set the parameters and reset the optimizer state (moments and Adam's t): what a new Fit does */
int32_t gorse_fm_set_params(gorse_fm *h, float B, const float *W /*host*/, const float *V /*host*/);
int32_t gorse_fm_get_params(gorse_fm *h, float *B /*host or NULL*/, float *W /*host or NULL*/, float *V /*host or NULL*/);
/* the training set (targets +-1); kept on the device until the next call.  n x width must not exceed 2^31 - 1
 * (GORSE_ERR_INVALID): the per-batch position lists hold int32.  For every batch size an epoch is called with, the first such
 * epoch sorts the batches' (feature, position) pairs once on the host; later epochs reuse the order. */
int32_t gorse_fm_set_train(gorse_fm *h, int64_t n, int32_t width, const int32_t *indices /*host*/, const float *values /*host*/,
                           const float *target /*host*/);
/* one epoch of AFM.Fit's inner loop (fm.go:362-378): contiguous batches of batch_size rows in dataset order (the last one
 * partial), BCEWithLogits averaged over each batch, one optimizer step per batch with weight decay wd.  cost_out (host or
 * NULL) = the fp32 sum of the batch means.  The cancel flag is read before every batch; at most 128 steps are in flight
 * when it is seen, and the call then returns GORSE_ERR_CANCELLED with the steps run so far applied. */
int32_t gorse_fm_epoch(gorse_fm *h, int32_t batch_size, int32_t optimizer, float lr, float wd,
                       const volatile int32_t *cancel /*host or NULL*/, float *cost_out /*host or NULL*/);
/* BatchInternalPredict (fm.go:156-178): logits of n rows; width may differ from the training width.  On a handle with
 * embedding fields: GORSE_ERR_INVALID (use gorse_fm_predict_embeddings). */
int32_t gorse_fm_predict(gorse_fm *h, int64_t n, int32_t width, const int32_t *indices /*host*/, const float *values /*host*/,
                         float *logits_out /*host*/);

/* ---- the item-embedding branch of ctr.AFM (fm.go:127-132; nn.Attention and nn.Linear, common/nn/layers.go:36-60, 160-190) --
 * Per embedding field of dimension D the model holds, in Parameters() order, H (d x D), Wa (D x d), ba (d), We (D x d),
 * be (d), all row-major, and adds sum_f vx_f enc_f to a row's logit, where x is the row's embedding (bf16, widened; all
 * zero where the sample has none), a = Softmax(relu(x Wa + ba) H, 1), enc = (a * x) We + be.  The Softmax is the
 * reference's: maxima and sums are applied through Tensor.sub / Tensor.div, which index them by flat index % n
 * (common/nn/op.go:760-777, tensor.go:328-379), so for a batch of n > 1 rows element (r, c) uses the maximum and sum of row
 * (r D + c) % n, forward and backward, and a row's logit depends on the other rows of its batch and on the batch length.
 * Caps: GORSE_FM_MAX_FIELDS fields, D in 1..GORSE_FM_MAX_EMBEDDING_DIM; beyond them GORSE_ERR_INVALID.
 * A handle without fields (the state after gorse_fm_create, or after n_fields = 0) is the plain factorization machine. */
#define GORSE_FM_MAX_FIELDS 8
#define GORSE_FM_MAX_EMBEDDING_DIM 4096
/* configure the fields (before gorse_fm_set_params / gorse_fm_set_embedding_params): allocates their parameters and moments as
 * zeros and drops earlier fields with their training embeddings */
int32_t gorse_fm_set_embedding_dims(gorse_fm *h, int32_t n_fields, const int32_t *dims /*host*/);
/* one field's tensors; set resets the field's moments (Adam's t is shared with B, V, W and reset by gorse_fm_set_params).
 * On get any pointer may be NULL. */
int32_t gorse_fm_set_embedding_params(gorse_fm *h, int32_t field, const float *H /*host*/, const float *Wa /*host*/,
                                      const float *ba /*host*/, const float *We /*host*/, const float *be /*host*/);
int32_t gorse_fm_get_embedding_params(gorse_fm *h, int32_t field, float *H, float *Wa, float *ba, float *We, float *be);
/* the training rows' embeddings of one field: n x D bf16 bit patterns (n of the last gorse_fm_set_train, which drops the
 * embeddings of the set before it), zero rows where a sample has none; kept on the device as bf16.  Offsets into the matrix
 * are 64-bit: n x D may exceed 2^31, and what bounds it is device memory (GORSE_ERR_NOMEM when it does not fit).
 * gorse_fm_epoch on a handle with fields runs the branch (forward, backward and the dense step of every field's tensors) and
 * returns GORSE_ERR_INVALID while a field's training embeddings are missing. */
int32_t gorse_fm_set_train_embeddings(gorse_fm *h, int32_t field, const uint16_t *emb /*host, n x D*/);
/* BatchInternalPredict with embeddings: rows are scored in slices of batch_size rows (the last one partial), as fm.go:168-176
 * does; the slice length is part of the result (see above).  emb[k] = field k's n x D bf16 matrix.  Without fields: the same
 * as gorse_fm_predict. */
int32_t gorse_fm_predict_embeddings(gorse_fm *h, int64_t n, int32_t width, const int32_t *indices /*host*/,
                                    const float *values /*host*/, const uint16_t *const *emb /*host, n_fields pointers*/,
                                    int32_t batch_size, float *logits_out /*host*/);

/* ---- ranking candidates by CTR from a resident item catalogue ---------------------------------------------------------------
 * The bulk form of the worker's per-user loop (worker/pipeline.go:451-499, rankByClickTroughRate): BatchPredict
 * (model/ctr/fm.go:180-229) builds one row per candidate, [user id, item id, user labels..., item labels...] plus the item's
 * embeddings, scores the rows in slices of batch_size, and cache.SortDocuments orders them.  Here the item side stays on the
 * device, the rows are composed there, many users are scored per launch and every user's list is sorted on the device.
 *
 * gorse_fm_set_items makes the item side resident.  Catalogue row i = indices / values [indptr[i], indptr[i + 1]): the item's
 * feature entries in the order BatchPredict appends them (the item-id entry first when the index knows the item, then the item
 * labels), values already scaled.  lead[i] = how many of its leading entries precede the user's labels in a composed row (0 or 1
 * in practice, any 0..len allowed; lead == NULL: 0 for every item).  emb[k] = field k's n_items x D_k bf16 matrix, an all-zero
 * row where the item has no embedding (convertToTensors, fm.go:555-561); emb may be NULL on a handle without fields.  The tables
 * stay on the device as bf16 and are indexed with 64-bit offsets.  n_items = 0 drops the catalogue, and so does
 * gorse_fm_set_embedding_dims (the field set changed); set_params, set_embedding_params, set_train and epoch leave it alone.
 * indptr[0] != 0, a decreasing indptr or lead[i] beyond row i: GORSE_ERR_INVALID; an index outside [0, n_features):
 * GORSE_ERR_RANGE; a catalogue that does not fit the device: GORSE_ERR_NOMEM.  Everything is validated before anything is
 * replaced: an error leaves the previous catalogue in place. */
int32_t gorse_fm_set_items(gorse_fm *h, int64_t n_items, const int64_t *indptr /*host, n_items+1*/, const int32_t *indices /*host*/,
                           const float *values /*host*/, const int32_t *lead /*host, n_items, or NULL*/,
                           const uint16_t *const *emb /*host, n_fields pointers, or NULL without fields*/);
/* Scores and ranks the candidates of n_users users.  User t's feature row = user_indices / user_values [user_indptr[t],
 * user_indptr[t + 1]) (user-id entry first when known, then the user labels; user_lead as lead above), its candidates = the
 * catalogue rows cand[cand_indptr[t] .. cand_indptr[t + 1]) (both pointers start at 0; a list may be empty, repeat an item and
 * share items with other users).  The composed row of candidate c of user t is, in this order (fm.go:183-206): the first
 * user_lead[t] entries of the user's row, the first lead[c] entries of the item's row, the rest of the user's row, the rest of
 * the item's row; entries with value 0 are skipped as the forward kernel skips them, so there is no width.  Its embedding in
 * field k is row c of table k.
 * scores_out[cand_indptr[t] + r] holds the BITS gorse_fm_predict_embeddings (without fields: gorse_fm_predict) returns for row r
 * when called on user t's materialised rows alone with the same batch_size: the same fused-multiply-add chains in the same
 * order, slices of batch_size rows per user with the reference's Softmax indexing inside each slice, a user's last slice
 * partial, and no slice shared between users.
 * order_out[cand_indptr[t] + r] = the position inside user t's list of its r-th ranked candidate: descending score; equal
 * scores (as floats, -0 == +0) by ascending position; NaN scores last, by ascending position.  cache.SortDocuments is
 * sort.Slice(score >) (storage/cache/database.go:190-194), which is not stable: this order is one it can produce, and no
 * reference test pins an order among ties.
 * Either output may be NULL.  No catalogue, batch_size <= 0, a malformed pointer array or user_lead[t] beyond the row:
 * GORSE_ERR_INVALID (also more than 2^31 - 1 candidates in one call); a candidate outside [0, n_items) or a user index outside
 * [0, n_features): GORSE_ERR_RANGE.  Everything is validated before the first launch and an error leaves the outputs untouched.
 * The cancel flag is read between launch rounds: GORSE_ERR_CANCELLED, outputs unspecified.  Parameters, optimizer state,
 * training set and training plan are untouched. */
int32_t gorse_fm_rank_users(gorse_fm *h, int64_t n_users, const int64_t *user_indptr /*host, n_users+1*/,
                            const int32_t *user_indices /*host*/, const float *user_values /*host*/,
                            const int32_t *user_lead /*host, n_users, or NULL*/, const int64_t *cand_indptr /*host, n_users+1*/,
                            const int32_t *cand /*host*/, int32_t batch_size, const volatile int32_t *cancel /*host or NULL*/,
                            float *scores_out /*host or NULL*/, int32_t *order_out /*host or NULL*/);
/* the handle's last gorse_fm_rank_users: rows scored, slices, launch rounds, lists longer than the device sort's cap (sorted by
 * the host with the same comparator), and the device time of its launches (hipEvents on the handle's stream, copies excluded).
 * Any pointer may be NULL. */
int32_t gorse_fm_rank_stats(gorse_fm *h, int64_t *rows, int64_t *slices, int64_t *rounds, int64_t *host_sorted, double *device_ms);

/* ---- evaluating the ranker from a resident test split ------------------------------------------------------------------------
 * EvaluateClassification (model/ctr/evaluator.go:46-153) partitions the test rows into positives and negatives, scores each side
 * with one BatchInternalPredict call, and forms Precision, Recall, Accuracy and AUC from the logits.  Fit calls it at epoch 0 and
 * at every Verbose-th epoch on the same rows.  Here the split stays on the device and only counts come back.
 *
 * gorse_fm_set_test keeps n rows (n x width indices / values padded with index 0 / value 0, as gorse_fm_predict takes them, and
 * emb[k] = field k's n x D_k bf16 matrix) in the order the reference scores them: the rows with target > 0 first, in dataset
 * order, then the others (a target of exactly 0 is a negative), in dataset order.  The partition and the gather of the embedding
 * rows happen once, here; the embeddings stay bf16 and are indexed with 64-bit offsets.  Everything is validated before
 * anything is replaced and an error leaves the previous split in place: an index outside [0, n_features) is GORSE_ERR_RANGE,
 * n >= 2^31 GORSE_ERR_INVALID, a split that does not fit the device GORSE_ERR_NOMEM.  n = 0 drops the split, and so does
 * gorse_fm_set_embedding_dims; set_params, set_embedding_params, set_train, epoch, set_items and rank_users leave it alone.  It
 * lives in buffers of its own: training and predict read nothing of it. */
int32_t gorse_fm_set_test(gorse_fm *h, int64_t n, int32_t width, const int32_t *indices /*host*/, const float *values /*host*/,
                          const float *target /*host, n*/,
                          const uint16_t *const *emb /*host, n_fields pointers, or NULL without fields*/);
/* Scores the resident split and forms the metrics' counts on the device.  The positives are sliced into batches of batch_size
 * rows from the first positive (the last slice partial), the negatives afresh from the first negative: the reference's Softmax
 * indexing makes the slice part of the result, and every logit carries the BITS gorse_fm_predict_embeddings (without fields:
 * gorse_fm_predict) returns for that row when called on the positive rows alone, or on the negative rows alone, with the same
 * batch_size.
 * counts[0..GORSE_FM_EVAL_COUNTS): n_pos, n_neg, positives with logit > 0, negatives with logit > 0, negatives with logit < 0,
 * NaN logits, and pairs_less = the exact sum over the positives of the negatives strictly below it (compared as floats,
 * -0 == +0).  auc_sum = the reference's own running sum (evaluator.go:139-148): the same per-positive counts added one after the
 * other in float32, the positives in ascending order of logit.  NaN logits take part in neither.  logits_out (may be NULL): the n
 * logits in the order the rows were given to gorse_fm_set_test; nothing else travels to the host.
 * No resident split or batch_size <= 0: GORSE_ERR_INVALID.  The cancel flag is read between launch rounds: GORSE_ERR_CANCELLED,
 * outputs unspecified.  Parameters, optimizer state, training set, training plan and item catalogue are untouched. */
#define GORSE_FM_EVAL_COUNTS 7
int32_t gorse_fm_evaluate(gorse_fm *h, int32_t batch_size, const volatile int32_t *cancel /*host or NULL*/,
                          int64_t *counts /*host, GORSE_FM_EVAL_COUNTS entries*/, float *auc_sum /*host*/,
                          float *logits_out /*host or NULL*/);
/* the handle's last gorse_fm_evaluate: rows scored, slices, launch rounds, and the device time of its launches (hipEvents on the
 * handle's stream, copies excluded).  Any pointer may be NULL. */
int32_t gorse_fm_evaluate_stats(gorse_fm *h, int64_t *rows, int64_t *slices, int64_t *rounds, double *device_ms);

/* ---- training and evaluating from (user, item) samples -------------------------------------------------------------------------
 * The reference keeps a CTR data set in sample form (model/ctr/data.go:152-267): one label row per user and per item, one
 * embedding per item, and per sample only (Users[i], Items[i], Target[i]); Dataset.Get composes the feature row and looks the
 * embedding up by item.  These two calls take that form.  The item side is the resident catalogue of gorse_fm_set_items;
 * the user side (a CSR in the form gorse_fm_rank_users takes; user_lead NULL = 0) is copied to the device and kept with the set.
 * Sample i is the row gorse_fm_rank_users composes for user user[i] and catalogue row item[i] -- user lead | item lead |
 * user rest | item rest, zero-valued entries skipped -- and its embedding in field k is row item[i] of catalogue table k, read
 * in place.  Per sample three numbers travel; no n x width rows and no n x D embeddings are built anywhere.
 *
 * gorse_fm_epoch trains whichever training set was set last (this one or gorse_fm_set_train's, each replaces the other) and
 * gorse_fm_evaluate scores whichever test split was set last; signatures, stats and cancel behaviour are theirs.  Every bit --
 * each epoch's cost, B, W, V and every field tensor after any number of SGD or Adam steps, the seven counts, auc_sum and
 * logits_out -- equals what gorse_fm_set_train + gorse_fm_set_train_embeddings / gorse_fm_set_test produce from the
 * materialised rows: the composed rows zero-padded to any width, the embeddings gathered per sample.  gorse_fm_set_test_samples
 * keeps EvaluateClassification's order (target > 0 first, then the rest, each side in sample order); logits_out comes back in
 * the order given.
 *
 * Both sets index the catalogue: gorse_fm_set_items (replacing or dropping it) and gorse_fm_set_embedding_dims drop a
 * sample-form training set and test split, and gorse_fm_epoch / gorse_fm_evaluate then return GORSE_ERR_INVALID saying so.
 * gorse_fm_set_train_embeddings on a sample-form set is GORSE_ERR_INVALID.  set_params, set_embedding_params, rank_users and
 * evaluate leave the training set alone.
 * Everything is validated before anything is replaced and an error leaves the previous set in place.  GORSE_ERR_INVALID: no
 * catalogue, n <= 0 for training (n = 0 drops the test split), a malformed user_indptr, user_lead[t] beyond its row, n >= 2^31;
 * a batch whose nonzero entries exceed 2^31 - 1 is refused by gorse_fm_epoch.  GORSE_ERR_RANGE: user[i] outside [0, n_users),
 * item[i] outside [0, n_items), a user feature outside [0, n_features).  GORSE_ERR_NOMEM: it does not fit the device.
 * Per-sample context labels (Dataset.ContextLabels) are out of scope: a set that has them keeps the padded route
 * (gorse_fm_set_train / gorse_fm_set_test on materialised rows). */
int32_t gorse_fm_set_train_samples(gorse_fm *h, int64_t n_users, const int64_t *user_indptr /*host, n_users+1*/,
                                   const int32_t *user_indices /*host*/, const float *user_values /*host*/,
                                   const int32_t *user_lead /*host, n_users, or NULL*/, int64_t n, const int32_t *user /*host, n*/,
                                   const int32_t *item /*host, n*/, const float *target /*host, n*/);
int32_t gorse_fm_set_test_samples(gorse_fm *h, int64_t n_users, const int64_t *user_indptr /*host, n_users+1*/,
                                  const int32_t *user_indices /*host*/, const float *user_values /*host*/,
                                  const int32_t *user_lead /*host, n_users, or NULL*/, int64_t n, const int32_t *user /*host, n*/,
                                  const int32_t *item /*host, n*/, const float *target /*host, n*/);

/* ---- neighbourhood recommenders (logics/recommend.go:244-348) --------------------------
 * recommendItemToItem and recommendUserToUser for many users at once.  Both are a two-hop weighted walk over two tables the handle
 * holds on the device:
 *     item-to-item: hop 1 = the user's positive feedback, newest first, unweighted; hop 2 = each item's neighbour list, weighted
 *     user-to-user: hop 1 = the user's neighbour list, weighted;                   hop 2 = each neighbour's positive feedback, unweighted
 * which: GORSE_NBR_HOP1 or GORSE_NBR_HOP2.  A table is a CSR of n_rows rows: indices[] and, when weights != NULL, one float32
 * raw similarity per entry.  The entry's weight as a double is
 *     w = (double)raw * scale;   if (transform == GORSE_NBR_RECIP) w = 1.0 / (1.0 - w);        (item_to_item.go:64-87, user_to_user.go:63-80)
 * weights == NULL: every w is exactly 1.0 (transform and scale ignored).  Hop-1 indices name hop-2 rows, hop-2 indices items of
 * [0, n_items).  gorse_nbr_set_table on a slot replaces the previous table.  indptr[0] != 0, a decreasing indptr, a non-finite raw
 * weight or scale, a weighted hop-2 table that repeats an index inside one row: GORSE_ERR_INVALID (an unweighted table may repeat,
 * as feedback rows do, and so may a weighted hop-1 table: those are successive lists); a negative index or a hop-2 index outside
 * [0, n_items): GORSE_ERR_RANGE.  An error leaves the previous table in place. */
#define GORSE_NBR_HOP1 0
#define GORSE_NBR_HOP2 1
#define GORSE_NBR_RAW 0
#define GORSE_NBR_RECIP 1
#define GORSE_NBR_MAX_K 256
typedef struct gorse_nbr gorse_nbr; /* one pair of neighbour tables resident on one GPU */
int32_t gorse_nbr_create(gorse_nbr **h, int32_t device, int64_t n_items);
int32_t gorse_nbr_destroy(gorse_nbr *h);
int32_t gorse_nbr_set_table(gorse_nbr *h, int32_t which, int64_t n_rows, const int64_t *indptr /*host, n_rows+1*/,
                            const int32_t *indices /*host*/, const float *weights /*host or NULL*/, int32_t transform, double scale);
/* For query t with hop-1 row r = rows[t] (rows == NULL: r = t, and n_queries must not exceed the hop-1 rows) the sum of item j is
 * formed exactly as the reference forms scores[id] += score (recommend.go:268-272, :334-339): s_j starts absent; for each position p
 * of row r in stored order, with entry (src, w1), and for each position q of hop-2 row src in stored order, with entry (j, w2):
 *     s_j = (s_j absent ? 0.0 : s_j) + w1 * w2
 * in IEEE double, the product a separate multiply, never fused.  (One of w1 and w2 is 1.0 in both of the reference's uses, so the
 * product is exact there; the general case is defined as written.)
 * An item is a candidate when it was reached at least once and is not in seen_items[seen_indptr[t] .. seen_indptr[t + 1])
 * (seen_indptr == NULL: no such rows; a row may be unsorted, repeat an item and name items that are never reached).  A sum of zero
 * or below is still a candidate.  The result row holds the min(k, candidates) candidates that come first in the total order:
 * larger sum first, equal sums (-0 == +0) by ascending item index, a NaN sum after every number (NaN sums among themselves by
 * ascending item index).  The reference pushes its map into TopKFilter in Go's map iteration order and so pins nothing among equal
 * sums (its own test uses ElementsMatch, logics/recommend_test.go:391-394); this call fixes the order.
 * items_out is n_queries * k padded with -1, scores_out n_queries * k padded with 0 and holds the sums' bits, count_out[t] =
 * min(k, candidates); each may be NULL.  rows[t] < 0 gives count 0.
 * GORSE_ERR_RANGE: a hop-1 index outside the hop-2 table's rows, a seen item outside [0, n_items), rows[t] beyond the hop-1 table.
 * GORSE_ERR_INVALID: k outside 1 .. GORSE_NBR_MAX_K, a table that is not set, a malformed seen_indptr.  Everything is validated
 * before anything is launched, and an error leaves the outputs untouched.
 * A query whose accumulator (the items it can reach, at most n_items, plus its seen row) fits an open-addressing table in LDS is
 * answered there; the others by the same code over a table in global scratch sized by that bound. */
int32_t gorse_nbr_recommend(gorse_nbr *h, int64_t n_queries, const int32_t *rows /*host, hop-1 row per query, or NULL: rows[t] = t*/,
                            int32_t k, const int64_t *seen_indptr /*host, n_queries+1, or NULL*/, const int32_t *seen_items /*host*/,
                            int32_t *items_out /*host or NULL, n_queries*k, padded with -1*/,
                            double *scores_out /*host or NULL, n_queries*k, padded with 0*/, int32_t *count_out /*host or NULL*/);
/* the handle's last gorse_nbr_recommend: queries answered over an LDS table (queries with rows[t] < 0 are counted here) / over a
 * table in global scratch, and the device time of its launches (hipEvents around them, copies excluded) */
int32_t gorse_nbr_recommend_stats(gorse_nbr *h, int64_t *n_lds, int64_t *n_global, double *device_ms);
/* A neighbour table built on the device from a similarity search's device-resident results: what QueryItemToItem / QueryUserToUser
 * (item_to_item.go:72-86, user_to_user.go:63-80) make of a search, for every row at once, without the lists crossing to the host.
 * Row r of the new table belongs to source s = sources[r] (sources == NULL: s = r); s < 0 gives an empty row, a source may repeat.
 * The list L of source s:
 *     from_topk:   what gorse_topk_search_vector returns for stored row s as a query vector with k = n + 1 and prune0 = 0, under the
 *                  index's current mask (the row itself is not excluded by the search); an entry's raw weight is -dist as a float
 *     from_sparse: what gorse_sparse_search returns for stored row s as the query with exclude == NULL and k = n + 1; raw = the score
 * Walk L in order; skip the entry whose index is s; when positive_only != 0 skip entries with raw <= 0 (a NaN is kept); stop after n
 * kept entries.  The kept (index, raw) pairs in that order are row r; the table is weighted, transform and scale are stored as
 * gorse_nbr_set_table stores them.  The table equals, bit for bit, the one a caller builds from those public searches on the host.
 * GORSE_ERR_INVALID: a NULL handle, an unknown which or transform, n_rows < 0, n outside 1 .. GORSE_NBR_MAX_LIST, a non-finite
 * scale, handles on different devices, a kept raw weight that is not finite.  GORSE_ERR_RANGE: sources[r] >= the index's rows;
 * which == GORSE_NBR_HOP2 and more index rows than the handle's n_items.  GORSE_ERR_NOMEM: the staging (n_rows * n pairs) does not
 * fit.  An error leaves the previous table in place. */
#define GORSE_NBR_MAX_LIST 1023 /* n + 1 is the k of the search: the sparse search serves k <= 1024 */
int32_t gorse_nbr_set_table_from_topk(gorse_nbr *h, int32_t which, gorse_topk *index, int64_t n_rows,
                                      const int64_t *sources /*host, n_rows, or NULL: sources[r] = r*/, int32_t n,
                                      int32_t positive_only, int32_t transform, double scale);
int32_t gorse_nbr_set_table_from_sparse(gorse_nbr *h, int32_t which, gorse_sparse *index, int64_t n_rows,
                                        const int64_t *sources /*host or NULL*/, int32_t n,
                                        int32_t positive_only, int32_t transform, double scale);
/* the table a slot holds, host-built or device-built; an unset slot: GORSE_ERR_INVALID.  Outputs may be NULL; weights must be NULL
 * for an unweighted table. */
int32_t gorse_nbr_table_info(gorse_nbr *h, int32_t which, int64_t *n_rows, int64_t *nnz, int32_t *weighted);
int32_t gorse_nbr_get_table(gorse_nbr *h, int32_t which, int64_t *indptr /*host, n_rows+1*/,
                            int32_t *indices /*host, nnz, or NULL*/, float *weights /*host, nnz, or NULL*/);

/* ---- the candidate chain: RecommendSequential for many users at once (logics/recommend.go:135-156) ---------------------------
 * The worker's offline pass (worker/pipeline.go:124-306) runs the configured recommenders in order; each is filtered by the user's
 * exclude set, and its results join the exclude set before the next one runs; candidates whose item is gone are dropped
 * (pipeline.go:228-243) and the rest is ranked by the CTR model.  A gorse_cand keeps the exclusion rows and the candidate rows of
 * n_queries users on the device for such a pass: the device stages (gorse_mf_recommend, gorse_nbr_recommend) read their seen rows
 * from it and leave their results in it, the list recommenders (latest, non-personalized, external) are a filter over it, and
 * gorse_fm_rank_cand takes its candidates from it.  Per stage one row pointer (8 bytes per query) crosses to the host.
 * All attached handles must number the items alike, 0 .. n_items - 1: that is the caller's responsibility, and mapping between
 * index spaces is out of scope.  This is the reference's limit = 0 form; the early stop of limit > 0 is not provided.
 *
 * gorse_cand_begin starts a pass (dropping the previous one, finished or not).  Row t of the CSR (excl_indptr from 0; NULL: no
 * rows) is what NewRecommender puts into excludeSet for query t; a row may be unsorted and repeat an item.  The rows are kept
 * twice: the BASE rows, sorted ascending once, and the CURRENT rows, which start as a copy.  capacity = the candidates one query
 * can come to hold.
 * A stage gives query t a list L_t in its final order (limit = 0).  Entries whose item is in t's current row are dropped; then
 * entries with keep[item] == 0 (recommendUserToUser's data-store filter, recommend.go:317-345: it sits behind the top-k, so what
 * it drops is neither a candidate nor excluded later; keep == NULL keeps all); the first k survivors are appended to t's
 * candidates with the stage's number (0, 1, ...), and their items are merged into t's current row: ascending, repeats kept.  A
 * list that repeats an item keeps both copies (lo.Filter does not deduplicate, and the set is updated after the list).
 *     add_mf      recommendCollaborative behind updateCollaborativeRecommend (pipeline.go:197-204): L_t = the row
 *                 gorse_mf_recommend(mf, users, k, item_ok, seen = the BASE rows) returns -- the exclude set is taken at
 *                 pipeline.go:200, before RecommendSequential has added anything -- and the score is the float widened to double.
 *                 The filter then applies the current rows: as the first stage it drops nothing.  users[t] < 0 (users == NULL:
 *                 user t): nothing for query t.
 *     add_nbr     L_t = the row gorse_nbr_recommend(nbr, rows, k, seen = the CURRENT rows) returns, with the sums' bits; the walk
 *                 excludes, as recommendItemToItem does.  rows[t] < 0: nothing for query t.
 *     add_shared  recommendLatest / recommendNonPersonalized: one list of n_list <= 65536 entries for every query, scores passed
 *                 through untouched.
 *     add_lists   one host list per query (a CSR, indptr from 0), for external recommenders or lists read back from a cache.
 * gorse_cand_finish compacts the candidates into a CSR, dropping entries with keep[item] == 0 (the item-exists filter of
 * pipeline.go:228-243), and closes the pass: gorse_cand_get and gorse_fm_rank_cand need a finished pass, and a further add_* is
 * GORSE_ERR_INVALID until the next begin.  gorse_cand_get returns that CSR (scores as doubles, the stage number per entry; any
 * output may be NULL); gorse_cand_get_exclusion the current rows, at any time of a pass; gorse_cand_info the pass's queries, stages
 * so far, candidates (before finish: appended so far) and current exclusion entries; gorse_cand_stats one stage's device time:
 * the stage's own search (gorse_mf_recommend_stats / gorse_nbr_recommend_stats; 0 for a list stage) and the chain's kernels
 * (filter, scan, append, merge).
 * Everything is validated before anything is launched or replaced, and an error leaves the chain exactly as it was (after a
 * GORSE_ERR_NOMEM / GORSE_ERR_HIP inside gorse_cand_begin the chain has no pass).
 * GORSE_ERR_INVALID: k outside 1 .. GORSE_CAND_MAX_K; a stage that could overflow capacity (the candidates so far are bounded by
 * the sum of the stages' k); more than GORSE_CAND_MAX_STAGES stages; no pass begun, or the pass finished; a malformed pointer
 * array; n_list > 65536; a stage handle on another device, or one whose item count (the model's I, the tables' n_items, the
 * catalogue's n_items) differs from the chain's n_items.  GORSE_ERR_RANGE: an item outside [0, n_items) in any input, a user or
 * row outside the stage handle's range -- the stage call's own rules apply and its message is passed through. */
#define GORSE_CAND_MAX_K 256      /* per stage; the merge sorts a stage's new items in LDS */
#define GORSE_CAND_MAX_STAGES 255 /* the stage number of a candidate is one byte */
typedef struct gorse_cand gorse_cand; /* one pass's exclusion and candidate rows resident on one GPU */
int32_t gorse_cand_create(gorse_cand **c, int32_t device, int64_t n_items);
int32_t gorse_cand_destroy(gorse_cand *c);
int32_t gorse_cand_begin(gorse_cand *c, int64_t n_queries, const int64_t *excl_indptr /*host, n_queries+1, or NULL*/,
                         const int32_t *excl_items /*host*/, int32_t capacity);
int32_t gorse_cand_add_mf(gorse_cand *c, gorse_mf *mf, const int32_t *users /*host, n_queries, or NULL*/, int32_t k,
                          const uint8_t *item_ok /*host, n_items, or NULL*/, const uint8_t *keep /*host, n_items, or NULL*/);
int32_t gorse_cand_add_nbr(gorse_cand *c, gorse_nbr *nbr, const int32_t *rows /*host, n_queries, or NULL*/, int32_t k,
                           const uint8_t *keep /*host, n_items, or NULL*/);
int32_t gorse_cand_add_shared(gorse_cand *c, int64_t n_list, const int32_t *items /*host*/, const double *scores /*host*/,
                              int32_t k, const uint8_t *keep /*host, n_items, or NULL*/);
int32_t gorse_cand_add_lists(gorse_cand *c, const int64_t *indptr /*host, n_queries+1*/, const int32_t *items /*host*/,
                             const double *scores /*host*/, int32_t k, const uint8_t *keep /*host, n_items, or NULL*/);
int32_t gorse_cand_finish(gorse_cand *c, const uint8_t *keep /*host, n_items, or NULL*/);
int32_t gorse_cand_info(gorse_cand *c, int64_t *n_queries, int32_t *n_stages, int64_t *n_candidates, int64_t *n_excluded);
int32_t gorse_cand_get(gorse_cand *c, int64_t *indptr_out /*host, n_queries+1*/, int32_t *items_out, double *scores_out,
                       uint8_t *stage_out);
int32_t gorse_cand_get_exclusion(gorse_cand *c, int64_t *indptr_out /*host, n_queries+1*/, int32_t *items_out);
int32_t gorse_cand_stats(gorse_cand *c, int32_t stage, double *stage_ms /*the stage's own search*/,
                         double *chain_ms /*filter, scan, append, merge*/);
/* gorse_fm_rank_users with the candidates taken from a finished pass: user t's list is row t of the chain's CSR (what
 * gorse_cand_get returns), read on the device; n_users = the pass's queries.  scores_out / order_out are indexed by that CSR and
 * hold the bits and the order gorse_fm_rank_users gives on the same lists; gorse_fm_rank_stats covers the call.  Errors as
 * gorse_fm_rank_users; no finished pass, a chain on another device or with another n_items than the catalogue: GORSE_ERR_INVALID. */
int32_t gorse_fm_rank_cand(gorse_fm *h, gorse_cand *c, const int64_t *user_indptr /*host, n_queries+1*/,
                           const int32_t *user_indices /*host*/, const float *user_values /*host*/,
                           const int32_t *user_lead /*host, n_queries, or NULL*/, int32_t batch_size,
                           const volatile int32_t *cancel /*host or NULL*/, float *scores_out /*host or NULL*/,
                           int32_t *order_out /*host or NULL*/);

/* ---- replacement: the user's historical items back among the candidates, their ranked scores decayed ------------------------
 * worker/pipeline.go:573-643, for recommend.replacement.enable_replacement.  Per feedback of query t the caller gives the item and
 * its kind: GORSE_CAND_KIND_POSITIVE when the feedback type matches a positive type, GORSE_CAND_KIND_READ when it does not but
 * matches a read type (matching the type expressions is string work and stays with the caller; other feedback is left out).
 * gorse_cand_add_replacement needs a finished pass and runs once per pass.  A history row may be unsorted, repeat an item and hold
 * an item with both kinds.  On the device row t becomes its distinct items, ascending, one kind each (positive wins), without the
 * items of keep[item] == 0 (ItemCache.GetSlice, pipeline.go:661-686: the item exists and is not hidden; NULL keeps all): the pass's
 * REPLACEMENT ROW of query t, resident until the next begin, and what gorse_cand_get_replacement returns.  Its items that are not
 * among t's finished candidates are appended behind them, ascending (the reference appends in Go map order, which nothing pins),
 * with score bits +0.0 and stage GORSE_CAND_STAGE_REPLACEMENT.  The grown rows ARE the finished pass from then on: gorse_cand_get,
 * gorse_cand_info and gorse_fm_rank_cand read them.  The exclusion rows are not touched.  One row pointer (8 bytes per query) comes
 * back.  gorse_cand_replacement_stats: entries appended, positive and read entries of the replacement rows, device milliseconds
 * (zeros on a pass without the stage, where gorse_cand_get_replacement returns empty rows).
 * Everything is validated before anything is launched or replaced, and an error (GORSE_ERR_NOMEM included) leaves the finished
 * pass exactly as it was.  GORSE_ERR_INVALID: no finished pass, a second call in one pass, a malformed pointer, a kind other than
 * 1 or 2.  GORSE_ERR_RANGE: an item outside [0, n_items).
 *
 * gorse_fm_rank_cand_decayed scores exactly as gorse_fm_rank_cand (the same bits in scores_out), then decays and sorts on the
 * device (applyReplacementDecay, pipeline.go:617-643): a candidate whose item is in its query's replacement row -- appended or
 * found by a recommender on its own -- gets final = (double)score * positive_decay or * read_decay by its kind (one IEEE double
 * multiply), every other one final = (double)score.  order_out[f_ptr[t] + r] = the position in t's list of its r-th entry under:
 * descending final; equal doubles (-0 == +0) in gorse_fm_rank_cand's order; NaN last, in gorse_fm_rank_cand's order -- one of the
 * outcomes the reference's unstable sort.Slice admits, chosen once.  On a pass without a replacement stage order_out is
 * gorse_fm_rank_cand's and final_out the widened float.  A decay that is not > 0 (config.go:403-404, validate:"gt=0"):
 * GORSE_ERR_INVALID; every other error as gorse_fm_rank_cand.  gorse_fm_rank_stats covers the call, the decay and the sort. */
#define GORSE_CAND_STAGE_REPLACEMENT 255 /* stage numbers of real stages are 0 .. 254 */
#define GORSE_CAND_KIND_POSITIVE 1
#define GORSE_CAND_KIND_READ 2
int32_t gorse_cand_add_replacement(gorse_cand *c, const int64_t *hist_indptr /*host, n_queries+1, from 0*/,
                                   const int32_t *hist_items /*host*/, const uint8_t *hist_kind /*host, 1 or 2 per entry*/,
                                   const uint8_t *keep /*host, n_items, or NULL*/);
int32_t gorse_cand_get_replacement(gorse_cand *c, int64_t *indptr_out /*host, n_queries+1*/, int32_t *items_out,
                                   uint8_t *kind_out); /* any may be NULL */
int32_t gorse_cand_replacement_stats(gorse_cand *c, int64_t *n_added, int64_t *n_positive, int64_t *n_read, double *device_ms);
int32_t gorse_fm_rank_cand_decayed(gorse_fm *h, gorse_cand *c, const int64_t *user_indptr /*host, n_queries+1*/,
                                   const int32_t *user_indices /*host*/, const float *user_values /*host*/,
                                   const int32_t *user_lead /*host, n_queries, or NULL*/, int32_t batch_size,
                                   const volatile int32_t *cancel /*host or NULL*/, double positive_decay, double read_decay,
                                   float *scores_out /*host or NULL: the ranker's bits*/,
                                   double *final_out /*host or NULL: decayed*/, int32_t *order_out /*host or NULL*/);

#ifdef __cplusplus
}
#endif
#endif /* GORSE_HIP_H */
