/*
 * fmhip_mcmc_groups.h — the MCMC learner's attribute groups (libfmhip.so): a regulariser lambda and a prior mean mu per FEATURE
 * GROUP, as in libFM's MCMC (its -meta file) and the reference's fm/bs/Metadata.scala (attrGroup, numAttrGroups, numAttrPerGroup).
 * Users, items, context fields and a bag of words do not share a scale; with one lambda per parameter group none of them is fitted,
 * with one per (parameter group, feature group) each is.  It includes fmhip_mcmc_task.h, whose handles — regression and
 * classification alike — it extends.
 *
 * THE RULE.  A handle gets a table group[i] in [0, G) for every i < num_attribute.  State: alpha, lambda[g][a], mu[g][a], g = 0 (w),
 * 1 + f (factor f), a the attribute group; stored row-major, [(k + 1) x G]; start: init_lambda and 0 everywhere.  T_a = the trained
 * features of group a (the column slots with id < num_attribute: quirk Q1's last slot never counts), m_a = |T_a|.  One epoch is
 * fmhip_mcmc.h's sweep with step 4 changed — for g = 0, then every factor:
 *     for a = 0 .. G-1:  lambda_ga ~ Gamma((alpha_lambda + m_a + 1) / 2, rate (beta_lambda + sum_{T_a} (theta_i - mu_ga)^2 +
 *                        gamma_0 (mu_ga - mu_0)^2) / 2) with the old mu_ga;
 *                        mu_ga ~ N((sum_{T_a} theta_i + gamma_0 mu_0) / (m_a + gamma_0), 1 / ((m_a + gamma_0) lambda_ga)) with the new
 *                        lambda_ga  (m_a = 0: the same formulas with sums of 0 — a draw from the prior);
 *     every i in T ascending, as ever, its conditional taking lambda[g][group[i]] and mu[g][group[i]].
 * alpha, the bias step, the coordinates' noise, the probit targets and the test rows' accumulation are fmhip_mcmc.h's.
 *
 * RANDOM NUMBERS keep the counter (index, group, t, stream): the hyper-parameter draws put g + (a << 16) into the group word of
 * stream 3 (lambda) and stream 4 (mu).  a = 0 is fmhip_mcmc.h's draw, so G = 1 is that sampler in every random number — and a
 * handle with G = 1 runs exactly its launches.  G <= FMHIP_MCMC_MAX_GROUPS and k <= 256 keep the word unambiguous.
 *
 * The sums the draws need come from one launch of fixed-order reductions over a plan made when the groups are set (the trained
 * slots in a stable order by group, cut into chunks that never straddle a group); the host adds a (g, a)'s partials in chunk order:
 * the result does not depend on the CU count or the launch schedule, and an epoch still has one host sync.
 * Not here: groups for fmhip_als_epoch (sample = 0 through this handle is per-group-regularised ALS), relational / weighted /
 * multi-batch data.  (The fp32 SGD path has its own regulariser per feature group, fixed or learned on a validation set: fmhip_sgda.h.)
 */
#ifndef FMHIP_MCMC_GROUPS_H
#define FMHIP_MCMC_GROUPS_H
#include "fmhip_mcmc_task.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FMHIP_MCMC_MAX_GROUPS 4096

/* group: n = the model's num_attribute ids in [0, n_groups).  Only before the handle's first epoch.  Every lambda becomes
 * init_lambda and every mu 0.  FMHIP_ERR_INVALID, the handle unchanged: a NULL table, n != num_attribute, n_groups < 1, an id outside
 * [0, n_groups) (the message names the feature), a call after the first epoch.  FMHIP_ERR_UNSUPPORTED: n_groups >
 * FMHIP_MCMC_MAX_GROUPS */
int fmhip_mcmc_set_groups(fmhip_mcmc_t s, const int32_t *group, int64_t n, int32_t n_groups);
/* n_groups: G (1 on a handle that never had groups); counts: G values, m_a — the trained features of group a.  Both nullable */
int fmhip_mcmc_group_info(fmhip_mcmc_t s, int32_t *n_groups, int64_t *counts /* nullable */);
/* lambda, mu: (k + 1) * G doubles each, [g * G + a]; every out pointer is nullable */
int fmhip_mcmc_get_group_state(fmhip_mcmc_t s, double *alpha, double *lambda, double *mu, int64_t *iterations);
/* alpha and every lambda finite and > 0, every mu finite.  fmhip_mcmc_get_state / fmhip_mcmc_set_state serve a handle while G = 1;
 * with G > 1 they return FMHIP_ERR_INVALID and name these two calls */
int fmhip_mcmc_set_group_state(fmhip_mcmc_t s, double alpha, const double *lambda, const double *mu);

#ifdef __cplusplus
}
#endif
#endif /* FMHIP_MCMC_GROUPS_H */
