/*
 * fmhip_pairing.h — pairwise ranking with a factorization machine (libfmhip.so): training on the DIFFERENCE of adjacent rows
 * (BPR / RankNet) and scoring held-out pairs.
 *
 * fmhip_topk.h serves a ranking — the K items a user's score puts first.  A recommender trained on implicit feedback has no
 * meaningful labels to fit row by row, only preferences ("this user took item A, not item B"); its objective is pairwise,
 * -log sigma(yhat_preferred - yhat_other).  That objective needs no new data path: it only changes how the residual e is formed,
 * from the margin of TWO rows instead of one.  Everything downstream of e is linear in it and is the training step of fmhip.h as
 * it stands.  Choosing which `other` row to pair with a preferred one (negative sampling) is the caller's job
 * here; fmhip_bpr.h draws it on the device over a block of contexts and a block of candidates.
 *
 * Same library and conventions as fmhip.h (plain C, int status, fmhip_last_error, never throws), which this header includes.
 *
 *  - threads: fmhip_model_set_pairing changes the model (exclusive lock, like fmhip_model_set_loss); fmhip_pair_logloss is a
 *    SCORING call in the sense of fmhip.h — re-entrant, the model's lock taken shared, a stream and a workspace of its own.
 *  - determinism: results are bit-identical run to run; a model switched to ADJACENT and back trains bit-identically to one never
 *    touched.
 */
#ifndef FMHIP_PAIRING_H
#define FMHIP_PAIRING_H
#include "fmhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* How the rows of a batch form the examples the model TRAINS on — a second switch beside the loss (pairwise ranking: BPR / RankNet,
 * for preference data without meaningful labels).  NONE: every row is an example.  ADJACENT: rows 2j and 2j+1 of a batch are ONE
 * example and the model's loss is applied to their difference — margin d_j = yhat_2j - yhat_2j+1, target dy_j = y_2j - y_2j+1,
 *   squared:  g_j = d_j - dy_j          logistic:  g_j = sigma(d_j) - [dy_j > 0]   (BPR when the preferred row comes first with the
 *                                                  larger label, -log sigma(yhat_preferred - yhat_other); RankNet in general)
 * and the rows' residuals are e_2j = g_j, e_2j+1 = -g_j in the same sum g_theta = sum e_r h_r(theta) of fmhip.h's training section.  |batch| in the update
 * stays the batch's ROW count (a pair contributes two rows).  sum e is exactly 0: stats.sum_e and fmhip_batch_grad's gw0 are 0.0 and
 * w0 moves by reg0 only; stats.sse = sum e_r^2 = 2 sum g_j^2; stats.nonfinite counts the rows whose yhat is not finite.  Empty rows
 * are legal (yhat = w0).  Pairs must not straddle batches: a training call on a dataset with an odd n_rows, or with several batches
 * and an odd batch_rows, returns FMHIP_ERR_INVALID (the message says which) and changes nothing.
 * It applies to every training call the loss applies to — fmhip_sgd_step / _epoch, fmhip_batch_grad, fmhip_step_compute / _forward /
 * _backward / _apply, both optimizers, the dense, sharded and touched fmhip_dp_* modes (fmhip_dp_plan agrees it over the ranks with
 * the loss and fails on every rank if they differ; a model whose pairing changes after the plan contributes zeros and returns
 * FMHIP_ERR_INVALID; every rank's own batches must be even, which each rank checks for itself: keep the ranks' shards even).
 * FMHIP_ERR_UNSUPPORTED for a paired model: FMHIP_EXCHANGE_PIPELINED (at fmhip_dp_plan, on every rank), the two-pass forward
 * (fmhip_step_forward_pass) and fmhip_als_epoch.  The scoring calls (fmhip_predict(_rows), fmhip_rmse, fmhip_logloss,
 * fmhip_pair_logloss, fmhip_residual, fmhip_term_q, fmhip_topk, fmhip_pair_scores) do not depend on it.  A new model is NONE;
 * fmhip_model_set_params, fmhip_model_init_normal, fmhip_model_set_loss and fmhip_model_set_optimizer do not reset it.  Any other
 * value: FMHIP_ERR_INVALID. */
enum fmhip_pairing { FMHIP_PAIRING_NONE = 0, FMHIP_PAIRING_ADJACENT = 1 };
int fmhip_model_set_pairing(fmhip_model_t m, int pairing);

/* Pairwise ranking score of the pairs (rows 2j, 2j+1) of `d`, whatever the model's loss or pairing; d_j = yhat_2j - yhat_2j+1,
 * dy_j = y_2j - y_2j+1.  logloss: the mean over pairs of softplus(-d_j) if dy_j > 0, else softplus(d_j) (each in fp64, summed in
 * fp64).  concordance (nullable): the share of pairs with (d_j > 0) == (dy_j > 0), a pair with d_j == 0 counting one half — the
 * pairwise AUC the logistic pair loss optimises.  A model that cannot tell the rows of a pair apart scores log 2 and 0.5.
 * stats (nullable): sum_e = 0, sse over e = +-(sigma(d_j) - [dy_j > 0]), rows, nnz, nonfinite (rows with a non-finite yhat).
 * An odd n_rows (or odd batches), NULL logloss: FMHIP_ERR_INVALID. */
int fmhip_pair_logloss(fmhip_model_t m, fmhip_dataset_t d, double *logloss, double *concordance /* nullable */,
                       fmhip_stats *stats /* nullable */);

#ifdef __cplusplus
}
#endif
#endif /* FMHIP_PAIRING_H */
