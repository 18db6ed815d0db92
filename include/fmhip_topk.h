/*
 * fmhip_topk.h — top-K recommendation with a trained factorization machine (libfmhip.so).
 *
 * What the reference's own demo trains its model FOR (S/driver.scala:73-113: MovieLens users x items, scored through
 * FMModel.predict, S/fm/FMModel.scala:34): "which K of these M items does the model rank highest for this user?".  Scoring
 * one joined sparse row per (user, item) pair through fmhip_predict re-gathers the same V rows B x M times; the FM score of
 * a pair splits exactly instead,
 *
 *     score(c, d) = predict(c) + predict(d) - w0 + sum_f q_f(c) * q_f(d),     q_f(r) = sum_i v_fi x_ri  (S/fm/lib/ALS.scala:146-150)
 *
 * (with s_f(r) = sum_i (v_fi x_ri)^2 the interaction term of the joined row is 1/2 sum_f [(q_f(c) + q_f(d))^2 - s_f(c) - s_f(d)],
 * S/fm/FMModel.scala:48-63; expand the square), so one forward pass over the B context rows, one over the M candidate rows
 * and a [B x Kp] . [Kp x M] product do the whole job, and the best K per context are selected while the product is formed:
 * the B x M scores never exist in memory.
 *
 * Same library and conventions as fmhip.h (plain C, int status, fmhip_last_error, never throws), which this header includes.
 *
 *  - threads: both calls are SCORING calls in the sense of fmhip.h — re-entrant, the model's lock taken shared, each call on
 *    a stream and in a workspace of its own, ordered behind whatever the model's own stream has queued.
 *  - a lazily decayed model scores correctly; the scores do not depend on the model's loss or optimizer.
 *  - memory: the device workspace is O((B_chunk + M) * Kp + B_chunk * K * splits) — the candidates' table, one chunk of
 *    contexts (a batch of the contexts' dataset), the chunk's partial lists — never O(B * M).  NOTHING is cached between
 *    calls: the candidates' table is rebuilt by every call (the model may have changed) and freed when the call returns.
 *  - determinism: the score of a pair is ONE fixed fp32 expression, (yhat(c) + (yhat(d) - w0)) + dot, dot = an fmaf chain
 *    over the padded factor slots in ascending order starting from 0 (-0 is returned as +0), whatever tile, chunk or
 *    candidate split the pair falls into.  Results are bit-identical run to run, a context scored alone gets the bits it
 *    gets inside a batch, and fmhip_topk's scores are fmhip_pair_scores' bit for bit.
 */
#ifndef FMHIP_TOPK_H
#define FMHIP_TOPK_H
#include "fmhip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FMHIP_TOPK_MAX 128   /* largest K */

/* score(c, d) = predict(c) + predict(d) - w0 + sum_f q_f(c) q_f(d)  — which IS FMModel.predict (S/fm/FMModel.scala:34-63) of the
 * row "c's entries, then d's" whenever the two rows share no feature id (user fields vs item fields) — for every context row c
 * of `contexts` and every candidate row d of `candidates`; per context the K candidates with the highest score.
 *   idx   [n_contexts * k]  candidate ROW NUMBERS, best first; equal scores: lower row number first; NaN scores rank
 *                           below every number (after -Inf).  Fewer than k candidates left: the tail is -1.
 *   score [n_contexts * k]  nullable; the scores of idx (the tail: -Inf)
 *   excl_ptr [n_contexts+1], excl [excl_ptr[n_contexts]]  nullable pair: per context the candidate row numbers that must
 *                           not be returned (what the user has already rated), ascending and distinct within a context
 * When c and d DO share a feature id the joined row would hold it twice; the score is then still, by definition, the
 * right-hand side above.  Both datasets may be of either kind (fmhip_rows_create*, or a training dataset); labels are
 * ignored.  Both must be on the model's device and within its width (FMHIP_ERR_SHAPE); n_candidates must fit an int32.
 * FMHIP_ERR_INVALID: a NULL handle or idx; k < 1 or k > FMHIP_TOPK_MAX; one of excl_ptr / excl NULL and the other not;
 * excl_ptr negative or decreasing; an excluded number outside [0, n_candidates) or not ascending.  n_contexts == 0 or
 * n_candidates == 0 is not an error (nothing written / all -1). */
int fmhip_topk(fmhip_model_t m, fmhip_dataset_t contexts, fmhip_dataset_t candidates, int32_t k,
               const int64_t *excl_ptr, const int32_t *excl, int32_t *idx, double *score);

/* The same scores in full for the contexts [c0, c1): out[(c - c0) * n_candidates + d].  For evaluation code that wants
 * the whole block (ranking metrics) and for testing the product on its own; the caller bounds the size by its choice of c1 - c0. */
int fmhip_pair_scores(fmhip_model_t m, fmhip_dataset_t contexts, fmhip_dataset_t candidates, int64_t c0, int64_t c1,
                      double *out);

#ifdef __cplusplus
}
#endif
#endif /* FMHIP_TOPK_H */
