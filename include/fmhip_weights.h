/*
 * fmhip_weights.h — per-row example weights (libfmhip.so): weighted training on every SGD path, and weighted scores.
 *
 * Click logs with down-sampled negatives (keep 1 in 20, weight it 20), class imbalance, recency decay, per-customer importance,
 * pairwise ranking whose pairs are not equally important (LambdaRank-style |delta NDCG|, confidence on implicit feedback): all of
 * them are one number per row.  Duplicating rows serves integer weights only and multiplies the data.
 *
 * THE RULE.  A dataset may carry one weight c_r >= 0 per row.  For a weighted dataset every training path forms
 *
 *     e_r <- c_r * e_r(loss)      g_theta = sum_{r in batch} e_r h_r(theta)      theta <- theta - eta (g_theta / |batch| + lambda_theta theta)
 *
 * the gradient of (1 / |batch|) sum_r c_r l_r — fmhip.h's training section with the residual scaled, and nothing else: everything
 * after the forward sees only e.
 *  - |batch| stays the batch's ROW count, not sum c: c == 1 is then the unweighted rule, and a data-parallel step needs no new
 *    collective.  (To normalise by sum c, scale the weights to mean 1.)
 *  - under FMHIP_PAIRING_ADJACENT (fmhip_pairing.h) the pair's weight is row 2j's: e_2j = c_2j g_j, e_2j+1 = -c_2j g_j.  The pair's
 *    residuals still sum to exactly zero; row 2j+1's weight is stored and not read.
 *  - AdaGrad takes the weighted gradient as it takes any other.
 *  - the training statistics (fmhip_stats of a step or an epoch) are those of the residual trained on, as under pairing:
 *    sum_e = sum c e, sse = sum (c e)^2, rows = the row count, nonfinite = the rows whose prediction is not finite.
 *  - a row of weight 0 has the residual +0 whatever its label and its prediction (a non-finite one included: it is still counted in
 *    nonfinite): it changes no bit of any parameter.  It still counts in |batch|.
 *  - weights are stored fp32 on the device, like y.  They must be finite (at most FLT_MAX) and >= 0: anything else is FMHIP_ERR_INVALID, the message
 *    names the first offending row, and the check runs before any HIP call (it needs no device).
 *  - it applies to every training call the loss applies to — fmhip_sgd_step / _epoch, fmhip_batch_grad, fmhip_step_compute /
 *    _forward / _backward / _apply, both losses, both pairings, both optimizers, the dense, sharded and touched fmhip_dp_* modes (the
 *    ranks' datasets may differ in being weighted).  The training forward of a weighted dataset runs in two launches (the q-mode
 *    forward, then a finish that forms the weighted residual); a dataset without weights takes exactly the path it always took.
 *  - FMHIP_ERR_UNSUPPORTED for a weighted dataset, the model left unchanged: FMHIP_EXCHANGE_PIPELINED (at fmhip_dp_plan, on EVERY
 *    rank as soon as SOME rank's dataset is weighted), the two-pass forward (fmhip_step_forward_pass) and fmhip_als_epoch.
 *  - fmhip_predict(_rows), fmhip_rmse, fmhip_logloss, fmhip_residual, fmhip_term_q, fmhip_auc, fmhip_pair_logloss, fmhip_topk,
 *    fmhip_pair_scores and fmhip_rank keep their meaning on ANY dataset: they ignore the weights, bit for bit.  The weighted scores
 *    are fmhip_weighted_scores below.  A weighted AUC is not provided.
 *
 * Same library and conventions as fmhip.h (plain C, int status, fmhip_last_error, never throws), which this header includes.
 *  - threads: the constructors and fmhip_dataset_weights touch no model; fmhip_weighted_scores is a SCORING call in the sense of
 *    fmhip.h — re-entrant, the model's lock taken shared, a stream and a workspace of its own.
 *  - determinism: results are bit-identical run to run, and do not depend on how the work is launched.
 */
#ifndef FMHIP_WEIGHTS_H
#define FMHIP_WEIGHTS_H
#include "fmhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* fmhip_dataset_create_opts with one weight per row.  weight == NULL: today's unweighted dataset.  opts == NULL: one batch and the
 * library's layout defaults; else as fmhip_dataset_create_opts (struct_size checked). */
int fmhip_dataset_create_weighted(int device, int64_t n_rows, const int64_t *row_ptr, const int32_t *col, const double *val,
                                  const double *y, const double *weight /* nullable, n_rows */,
                                  const fmhip_dataset_opts *opts /* nullable */, fmhip_dataset_t *out);
/* fmhip_rows_create (rows + labels only, for scoring) with one weight per row.  weight == NULL: fmhip_rows_create. */
int fmhip_rows_create_weighted(int device, int64_t n_rows, const int64_t *row_ptr, const int32_t *col, const double *val,
                               const double *y, const double *weight /* nullable, n_rows */, fmhip_dataset_t *out);

/* The weights of a dataset, read back.  has (nullable): 1 if it is weighted, else 0.  sum (nullable): the fp64 sum, in row order, of
 * the weights as stored (fp32); n_rows for an unweighted dataset.  out (nullable, n_rows doubles): the weights as stored; 1.0 for
 * every row of an unweighted dataset. */
int fmhip_dataset_weights(fmhip_dataset_t d, int *has, double *sum, double *out /* nullable, n_rows */);

typedef struct fmhip_weighted_result {
    int32_t struct_size;       /* in: sizeof(fmhip_weighted_result) */
    int32_t reserved;
    double  sum_w;             /* sum c (fp64 over the stored fp32 weights) */
    double  rmse;              /* sqrt(sum c (yhat - y)^2 / sum c) */
    double  mae;               /* sum c |yhat - y| / sum c */
    double  logloss;           /* sum c l / sum c, l the row's log-loss of fmhip_logloss: t = [y > 0], softplus(yhat) - t yhat */
    int64_t rows;              /* rows scored (all of them, weight 0 included) */
    int64_t nonfinite;         /* rows whose prediction is not finite (whatever their weight) */
} fmhip_weighted_result;

/* Weighted scores of the model's predictions (fmhip_predict) over a WEIGHTED dataset of either kind, whatever the model's loss,
 * pairing or optimizer; a lazily decayed model scores correctly.  Every row's terms are formed and summed in fp64.  A row of
 * weight 0 adds nothing, whatever its prediction.  sum c == 0 (or no rows): FMHIP_OK, NaN for the three ratios.
 * FMHIP_ERR_INVALID: an unweighted dataset; out == NULL or out->struct_size != sizeof(fmhip_weighted_result). */
int fmhip_weighted_scores(fmhip_model_t m, fmhip_dataset_t d, fmhip_weighted_result *out);

#ifdef __cplusplus
}
#endif
#endif /* FMHIP_WEIGHTS_H */
