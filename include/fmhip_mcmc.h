/*
 * fmhip_mcmc.h — the MCMC learner (libfmhip.so): Bayesian FM by Gibbs sampling (Freudenthaler, Schmidt-Thieme, Rendle: "Bayesian
 * Factorization Machines", 2011; libFM's default learner) on the ALS column walk.  The reference's ALS.scala is a cut-down copy of
 * that learner — its methods are still called drawTheta and drawGlobalBias — with the noise precision fixed at 1, the prior means at
 * 0 and the draw left out; this header puts back what it dropped.  There is no learning rate and nothing to tune: the regularisers
 * lambda and the noise precision alpha are SAMPLED, and the prediction is the average over the draws.
 *
 * THE RULE.  N train rows; T = the features the ALS walk trains (ids < num_attribute, quirk Q1 kept, with a stored entry), m = |T|;
 * groups g = 0 (w) and g = 1 + f (factor f).  State: alpha, lambda_g, mu_g (start: 1, init_lambda, 0).  One conditional serves
 * w0, w_i and v_if (operations in this order, no fused multiply-add):
 *
 *     prec   = lambda + alpha * sum h^2
 *     mean   = -(alpha * (sum e*h - theta * sum h^2) - mu * lambda) / prec
 *     theta' = mean + z / sqrt(prec)                 z: the coordinate's own N(0,1)
 *     theta  <- theta' if it is finite and differs from theta (ALS.scala:190-192), then e_r += h_r (theta' - theta)
 *
 * One epoch = one Gibbs sweep:
 *   1. e = yhat - y;   2. alpha ~ Gamma((alpha_0 + N) / 2, rate (beta_0 + sum e^2) / 2);
 *   3. w0 with h = 1, lambda = reg0, mu = 0; the residuals again with the new bias (as fmhip_als_epoch);
 *   4. for g = 0, then every factor:  lambda_g ~ Gamma((alpha_lambda + m + 1) / 2, rate (beta_lambda + sum_T (theta_i - mu_g)^2 +
 *      gamma_0 (mu_g - mu_0)^2) / 2) with the old mu_g;  mu_g ~ N((sum_T theta_i + gamma_0 mu_0) / (m + gamma_0),
 *      1 / ((m + gamma_0) lambda_g)) with the new lambda_g;  every i in T ascending, h = x (w) or x q - x^2 v (v);
 *   5. with a test set: yhat_test of this draw joins a running fp64 sum, the draw count goes up by one.
 * sample = 0 makes no draw at all: the state stays what the caller set and no noise term is added.  With alpha = 1, mu = 0,
 * lambda_0 = regw, lambda_1.. = regv the epoch then leaves THE BITS fmhip_als_epoch leaves (libFM's ALS = MCMC without sampling).
 *
 * RANDOM NUMBERS are counter-based — Philox4x32-10 keyed by (seed & 0xffffffff, seed >> 32), counter (index, group, t, stream),
 * t = the epochs this handle has completed — so every kernel shape and launch schedule sees the same draw:
 *     u53(a, b) = (((a << 32 | b) >> 11) + 0.5) * 2^-53;  uniform = u53(x0, x1);  normal = sqrt(-2 ln u53(x0, x1)) cos(2 pi u53(x2, x3))
 *     stream 0: coordinate noise (index = feature id, group = g)     1: w0's noise (0, 0)     2: alpha's gamma
 *     stream 3: lambda_g's gamma (group = g)                          4: mu_g's normal (0, g)
 * A gamma is Marsaglia-Tsang without the squeeze: attempt j takes the normal of index 2j and the uniform of index 2j + 1.
 *
 * Same library and conventions as fmhip.h (plain C, int status, fmhip_last_error, never throws), which this header includes.
 *  - the handle BORROWS the model, the train set and the test set: they must outlive it.  It owns the epoch's noise, the state and
 *    the test rows' running sum.
 *  - fmhip_mcmc_epoch CHANGES the model (its lock exclusive) and is synchronous; afterwards the model holds the last draw exactly
 *    as after fmhip_als_epoch (fp64 masters + the fp32 device copy).  One call per handle at a time.
 *  - FMHIP_ERR_UNSUPPORTED, the model unchanged: everything fmhip_als_epoch refuses, with the same words (a multi-batch dataset,
 *    one with a hot block or row blocks, a repeated feature in a row, a weighted dataset, a model set to the logistic loss or to
 *    pairs), and a test set without fp64 rows (fmhip_rows_create, multi-batch).  FMHIP_ERR_INVALID: a test set wider than the
 *    model, a prior that is not finite and > 0 (mu_0: finite; reg0: finite and >= 0).
 *  - determinism: bit-identical run to run for a given seed; the draws do not depend on the walk the sweep takes.
 * Classification (the probit link) and clipping to the label range: fmhip_mcmc_task.h, over this handle.
 * libFM's attribute groups (a lambda and a mu per feature group): fmhip_mcmc_groups.h.  Relational data, swept by blocks:
 * fmhip_mcmc_relational.h.  Not here: weighted data.
 */
#ifndef FMHIP_MCMC_H
#define FMHIP_MCMC_H
#include "fmhip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fmhip_mcmc *fmhip_mcmc_t;

typedef struct {
    uint64_t seed;
    int32_t sample;             /* 0: no draws (the conditional means under the state as set) */
    double reg0, init_lambda;   /* the bias's regulariser; every lambda_g's start */
    double alpha_0, beta_0, alpha_lambda, beta_lambda, gamma_0, mu_0;
} fmhip_mcmc_opts;

typedef struct {
    double alpha;               /* the noise precision the epoch drew (or kept) */
    double train_rmse;          /* of the residuals the epoch started from */
    int64_t iterations;         /* epochs completed, this one included */
} fmhip_mcmc_stats;

/* seed 0, sample 1, reg0 0, init_lambda 1, libFM's priors: alpha_0 = beta_0 = alpha_lambda = beta_lambda = gamma_0 = 1, mu_0 = 0 */
int fmhip_mcmc_opts_default(fmhip_mcmc_opts *opts);
/* test: NULL, or the rows whose predictions are averaged over the draws.  opts: NULL = the defaults */
int fmhip_mcmc_create(fmhip_model_t m, fmhip_dataset_t train, fmhip_dataset_t test /* nullable */, const fmhip_mcmc_opts *opts /* nullable */,
                      fmhip_mcmc_t *out);
int fmhip_mcmc_destroy(fmhip_mcmc_t s);
int fmhip_mcmc_epoch(fmhip_mcmc_t s, fmhip_mcmc_stats *stats /* nullable */);
/* lambda, mu: k + 1 doubles each (group 0 = w, 1 + f = factor f); every out pointer is nullable */
int fmhip_mcmc_get_state(fmhip_mcmc_t s, double *alpha, double *lambda, double *mu, int64_t *iterations);
/* alpha and every lambda finite and > 0, every mu finite */
int fmhip_mcmc_set_state(fmhip_mcmc_t s, double alpha, const double *lambda, const double *mu);
/* forget the draws averaged so far: burn-in ends here */
int fmhip_mcmc_reset_average(fmhip_mcmc_t s);
/* mean / last: the test set's n_rows doubles each, nullable — the average over the `draws` epochs since the last reset (0 draws:
 * zeros), the last draw's predictions */
int fmhip_mcmc_predictions(fmhip_mcmc_t s, double *mean, double *last, int64_t *draws);

#ifdef __cplusplus
}
#endif
#endif /* FMHIP_MCMC_H */
