// fm_resident.hip -- scoring rows that stay on the device: the one path gorse_fm_rank_users (fm_rank.hip: the rows composed from
// the call's users and the resident item catalogue) and gorse_fm_evaluate (fm_eval.hip: the rows of the resident test split)
// share.  Both hand over a plan (fm_eval_plan.hpp: BatchInternalPredict's slices, many of them per launch round) and a row source;
// score_rounds runs, round by round,
//   fm_forward_kernel<G, NF, Src, kLogit | kLogitVx>   one G-lane group per row: the FM logit, and vx when the model has fields;
//                                                      ComposedRows reads a user's entries through the scalar unit where a
//                                                      wave's rows all belong to one user
//   att_{score,exp,enc}_kernel<SliceRows>              per field the branch's three forward launches over the round's slices:
//                                                      every row carries its slice's first row and length, the Softmax's maxima
//                                                      and sums are indexed by row0 + (local_r D + c) % len, and x is read in
//                                                      place from the field's resident table, row item[r]
// -- the kernels gorse_fm_predict_embeddings launches one slice at a time (fm_internal.hpp), so the same bits.  It works in the
// handle's one RoundScratch and touches no buffer of training or of gorse_fm_predict*.
#include "fm_internal.hpp"

namespace gorse {
namespace fm {

template <class Src>
int32_t score_rounds(gorse_fm *h, const RoundPlan &plan, Src src, const DevBuf<uint16_t> *tables, const volatile int32_t *cancel,
                     RoundScratch &rs, float *logit) {
    const int32_t *seg = plan.desc.p, *item = seg + plan.n, *row0 = item + plan.n, *len = row0 + plan.n;
    for (int64_t k = 0; k <= plan.rounds(); k++) {  // the cancel flag is read before every round and once after the last
        if (cancel && *cancel) {
            GORSE_HIP_CHECK(hipStreamSynchronize(h->s));
            return fail(GORSE_ERR_CANCELLED, "cancelled");
        }
        if (k == plan.rounds()) break;
        const int64_t r0 = plan.round_begin[(size_t)k], nr = plan.round_begin[(size_t)k + 1] - r0;
        FwdArgs<Src> f{};
        f.src = src;
        f.src.round(seg, item, r0);
        f.V = h->V.p, f.W = h->W.p, f.B = h->B.p;
        f.nrows = nr, f.d = h->d;
        f.out = logit + r0, f.vx = rs.vx.p;
        if (h->n_fields == 0) {
            GORSE_TRY(launch_forward<kLogit>(h->s, f));
            continue;
        }
        GORSE_TRY(launch_forward<kLogitVx>(h->s, f));
        const SliceRows rows{item + r0, row0 + r0, len + r0};
        for (int e = 0; e < h->n_fields; e++) {
            AttArgs a = field_args(h, e);
            a.x = tables[e].p;
            a.nrows = nr;
            a.h = rs.h.p, a.s = rs.s.p, a.rmax = rs.rmax.p, a.rsum = rs.rsum.p;
            a.vx = rs.vx.p, a.logit = logit + r0;
            GORSE_TRY(branch_forward(h->s, a, rows));
        }
    }
    return GORSE_OK;
}

template int32_t score_rounds<ComposedRows>(gorse_fm *, const RoundPlan &, ComposedRows, const DevBuf<uint16_t> *,
                                            const volatile int32_t *, RoundScratch &, float *);
template int32_t score_rounds<PaddedRows>(gorse_fm *, const RoundPlan &, PaddedRows, const DevBuf<uint16_t> *,
                                          const volatile int32_t *, RoundScratch &, float *);

}  // namespace fm
}  // namespace gorse
