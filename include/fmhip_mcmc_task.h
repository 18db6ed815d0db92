/*
 * fmhip_mcmc_task.h — the MCMC learner's tasks (libfmhip.so): binary classification by the probit link with truncated-normal latent
 * targets (Albert, Chib: "Bayesian analysis of binary and polychotomous response data", 1993; libFM's default for -task c), and the
 * regression task's clamp of the test predictions.  It includes fmhip_mcmc.h, whose handle, rule and calls it extends: a latent
 * target y* drawn per row at the start of each epoch and handed to the sweep in the place of y turns the regression sampler into
 * the probit sampler — no column walk changes.
 *
 * THE RULE.  Labels: t_r = [y_r > 0] (fmhip_logloss's convention), s_r = +1 if t_r is 1, else -1.  One epoch of a CLASSIFICATION
 * handle, t = the epochs this handle has completed:
 *   1. yhat_r as fmhip_mcmc.h's step 1 computes it;
 *   2. the latent target —  t = 0: y*_r = s_r (libFM's start: no draw);
 *      t > 0, sample = 1: a = -s_r yhat_r, z ~ N(0,1) conditioned on z > a (below), y*_r = yhat_r + s_r z;
 *      t > 0, sample = 0: z = E[z | z > a] = phi(a) / (erfc(a / sqrt 2) / 2), and a + 1 / a for a > 30, where the quotient's terms
 *      head for the subnormals (libFM's ALS for classification);
 *   3. e_r = yhat_r - y*_r, and from here fmhip_mcmc.h's epoch with y* where it read y: the bias step, the residuals again, every
 *      group's lambda_g, mu_g and sweep;
 *   4. alpha is NOT drawn: it stays what the state holds — 1 unless fmhip_mcmc_set_state changed it, as in libFM; stream 2 is unused;
 *   5. stats.train_rmse is that of the latent residuals.
 *
 * THE TRUNCATED NORMAL is drawn by rejection from stream 5: attempt j = 0, 1, ... of row r takes the Philox block of counter
 * (r, j, t, 5), u1 = u53(x0, x1), u2 = u53(x2, x3); no fused multiply-add.
 *     a <= 0: z = sqrt(-2 ln u1) cos(2 pi u2) (fmhip_mcmc.h's normal of that block), accepted if z > a — at least every second is;
 *     a > 0:  Robert's exponential proposal, l = (a + sqrt(a^2 + 4)) / 2, z = a - ln(u1) / l, accepted if u2 <= exp(-(z - l)^2 / 2)
 *             — at least 0.76 of the attempts are.
 * At attempt 63 the proposal is taken unconditionally (a <= 0: as |z|, which is > a), so the loop is bounded by construction.
 *
 * TEST ROWS.  Classification: a draw's prediction is the probability p_r = erfc(-yhat_r / sqrt 2) / 2 = Phi(yhat_r); it is what
 * joins the running sum and what `last` holds.  Regression with clip: each draw's yhat_r is clamped to [clip_lo, clip_hi] before
 * it joins the sum and `last` (libFM clamps to the train labels' range; here the caller asks for it, and gives the range).
 *
 * Afterwards the model holds the last draw, as ever: its score is the probit score, whose probability is Phi(yhat), NOT the
 * logistic sigmoid — fmhip_auc and an accuracy at the threshold 0 apply to it, fmhip_logloss does not.  The task belongs to the
 * handle, not to the model: a model set to the logistic loss is still refused.
 * Not here: libFM's attribute groups, relational / weighted / multi-batch data, a scoring call.
 */
#ifndef FMHIP_MCMC_TASK_H
#define FMHIP_MCMC_TASK_H
#include "fmhip_mcmc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FMHIP_MCMC_REGRESSION 0
#define FMHIP_MCMC_CLASSIFICATION 1

typedef struct {
    int32_t task;               /* FMHIP_MCMC_REGRESSION / FMHIP_MCMC_CLASSIFICATION */
    int32_t clip;               /* regression only: 1 = clamp every draw's test prediction to [clip_lo, clip_hi] */
    double clip_lo, clip_hi;
} fmhip_mcmc_task_opts;

/* regression, no clip */
int fmhip_mcmc_task_opts_default(fmhip_mcmc_task_opts *task_opts);
/* fmhip_mcmc_create with a task; the handle is fmhip_mcmc.h's, and its epoch, get_state, set_state, reset_average, predictions and
 * destroy serve it unchanged.  task_opts NULL: exactly fmhip_mcmc_create.  FMHIP_ERR_INVALID: an unknown task, clip with the
 * classification task, a clip range that is not finite with clip_lo < clip_hi; otherwise whatever fmhip_mcmc_create refuses, in
 * the same words */
int fmhip_mcmc_create_task(fmhip_model_t m, fmhip_dataset_t train, fmhip_dataset_t test /* nullable */, const fmhip_mcmc_opts *opts /* nullable */,
                           const fmhip_mcmc_task_opts *task_opts /* nullable */, fmhip_mcmc_t *out);
/* out: the train set's n_rows doubles — the targets y* the last epoch trained on; before the first epoch, and on a regression
 * handle, the labels */
int fmhip_mcmc_latent_targets(fmhip_mcmc_t s, double *out);

#ifdef __cplusplus
}
#endif
#endif /* FMHIP_MCMC_TASK_H */
