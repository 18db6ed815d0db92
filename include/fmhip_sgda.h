/*
 * fmhip_sgda.h — SGDA (libfmhip.so): mini-batch SGD whose regularisers are learned during training, one per (feature group, factor),
 * by gradient steps on a held-out set (Rendle, "Learning recommender systems with adaptive regularization", WSDM 2012; libFM's
 * `-method sgda -validation`).  The fp32 SGD path's "nothing to tune": users, items and a bag of words stop sharing one lambda, and
 * nobody grid-searches regw / regv.  With eta_lambda = 0 and no validation set it is SGD with a FIXED regulariser per group.
 *
 * THE RULE.  A feature i (0 .. num_attribute: the model's n + 1 rows) has a group a = group[i] in [0, G).  State: lambda_w[a] and
 * lambda_v[f][a], all >= 0; reg0 stays the caller's scalar.  One step takes a train batch B and a validation batch C:
 *   1. theta' = theta - eta (g_B / |B| + lambda_{group, factor} theta) — fmhip_step_compute + the dense update of fmhip_step_apply, the
 *      same fp32 operations in the same order, lambda looked up per row; w0 steps with reg0.  The launch keeps theta in a shadow
 *      table (one more copy of the model).
 *   2. the gradient of C at theta' (fmhip_step_compute's path): h_w[i] = G_w[i] / |C|, h_v[i,f] = (G_V[i,f] - v'[i,f] G_b[i]) / |C|.
 *   3. d theta' / d lambda = -eta theta:  S_w[a] = sum_{i in a} w_i h_w[i],  S_v[f][a] = sum_{i in a} v_{i,f} h_v[i,f]  over the OLD
 *      theta;  lambda <- max(0, lambda + eta_lambda eta S).  With |B| = |C| = 1 this is libFM's sgd_theta_step + sgd_lambda_step.
 * The sums are fixed-order reductions over a plan made with the handle (the features in a stable order by group, cut into chunks of
 * 128 that never straddle a group; fp32 inside a chunk, the chunks added in fp64): no atomics, the same bits on every run.  The
 * packed gradient is all zero when a step with a validation batch returns (its head too); a step without one leaves it as
 * fmhip_step_apply does.
 *
 * An epoch visits the train batches in `order`; step t takes validation batch t mod (the validation set's batches), t the handle's
 * step counter, which runs on over epochs.  Nothing inside an epoch synchronises with the host.
 *
 * A pending lazy-decay scale is folded into the tables before a step; the tables stay at scale 1 under this learner.
 * Same library and conventions as fmhip.h (plain C, int status, fmhip_last_error, never throws), which this header includes; every
 * call takes the model's lock.  The handle borrows the model: destroy the handle first.
 * FMHIP_ERR_UNSUPPORTED: a model under AdaGrad or FTRL-Proximal or set to pairs (at create and at every step), a weighted dataset,
 * fmhip_dp_plan on a model that has a live handle.
 * Not here: include/sparkfm.hpp and the JNI shim, AdaGrad / FTRL under adaptive lambda, the data-parallel exchanges (fmhip_dp_*),
 * relational data, example weights, the BPR trainer, a rows-only update (every step walks the whole model).
 */
#ifndef FMHIP_SGDA_H
#define FMHIP_SGDA_H
#include "fmhip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FMHIP_SGDA_MAX_GROUPS 4096

typedef struct fmhip_sgda *fmhip_sgda_t;

/* group: n = num_attribute + 1 ids in [0, n_groups).  Every lambda_w starts at init_lambda_w, every lambda_v at init_lambda_v.
 * FMHIP_ERR_INVALID: a NULL table or out pointer, n_groups < 1, an init_lambda that is negative or not finite (all before the model
 * is looked at), a NULL model, n != num_attribute + 1, an id outside [0, n_groups) (the message names the feature).
 * FMHIP_ERR_UNSUPPORTED: n_groups > FMHIP_SGDA_MAX_GROUPS (before the model is looked at); the model's rule (above) */
int fmhip_sgda_create(fmhip_model_t m, const int32_t *group, int64_t n, int32_t n_groups, double init_lambda_w, double init_lambda_v,
                      fmhip_sgda_t *out);
int fmhip_sgda_destroy(fmhip_sgda_t h);
/* One step: train batch `batch`, validation batch `val_batch` of `val` (NULL: steps 2 and 3 are skipped — then eta_lambda must be 0).
 * stats_train / stats_val (nullable; a non-NULL one synchronises): the batch's residual statistics as fmhip_sgd_step reports them,
 * the train batch's at theta, the validation batch's at theta'.
 * FMHIP_ERR_INVALID: val made by fmhip_rows_create (it has no transposes), val == NULL with eta_lambda != 0, a batch out of range */
int fmhip_sgda_step(fmhip_sgda_t h, fmhip_dataset_t train, int64_t batch, fmhip_dataset_t val, int64_t val_batch, double eta,
                    double eta_lambda, double reg0, fmhip_stats *stats_train, fmhip_stats *stats_val);
/* order: NULL, or a permutation of the train batches.  stats_train sums the epoch's train batches, stats_val the validation batches
 * it used (rows counts them with repeats): the validation loss of the epoch for free.  Both nullable */
int fmhip_sgda_epoch(fmhip_sgda_t h, fmhip_dataset_t train, fmhip_dataset_t val, double eta, double eta_lambda, double reg0,
                     const int64_t *order, fmhip_stats *stats_train, fmhip_stats *stats_val);
/* lw: G values; lv: k * G values, lv[f * G + a].  get: either may be NULL.  set: both given, every value finite and >= 0
 * (FMHIP_ERR_INVALID otherwise, the handle unchanged); the values are stored in fp32 */
int fmhip_sgda_get_lambda(fmhip_sgda_t h, double *lw, double *lv);
int fmhip_sgda_set_lambda(fmhip_sgda_t h, const double *lw, const double *lv);
/* S_w [G] and S_v [f * G + a] of the last step that had a validation batch, in fp64 (zeros before one).  Either may be NULL */
int fmhip_sgda_last_sums(fmhip_sgda_t h, double *sw, double *sv);
/* n_groups: G; counts: G values, the features of every group; steps: the steps taken.  All nullable */
int fmhip_sgda_info(fmhip_sgda_t h, int32_t *n_groups, int64_t *counts, int64_t *steps);

#ifdef __cplusplus
}
#endif
#endif /* FMHIP_SGDA_H */
