/*
 * fmhip_mcmc_relational.h — the MCMC learner over relational data (libfmhip.so): the Gibbs sweep of fmhip_mcmc.h on the BLOCKS of a
 * relational dataset (fmhip_relational.h), without the flat rows it stands for — Rendle, "Scaling Factorization Machines to
 * Relational Data" (VLDB 2013), whose subject is ALS / MCMC on blocks.  A block column holds one entry per block row, not one per
 * data row that references it: a sweep walks k * (nnz(blocks) + O(N * parts)) entries instead of k * nnz(expand()).
 *
 * THE RULE is fmhip_mcmc.h's — the conditional, the priors, the epoch's order, the counters of the random numbers, quirk Q1 — with
 * the column sums taken from per-block-row caches.  N data rows; parts p = 0 .. P-1: the relations in order, then the plain part
 * under the identity mapping; j_p(r) = the block row of data row r; n_p[j] = the data rows that map to block row j.  Device state,
 * all fp64: e[N], Q[k][N] with Q_f[r] = sum_p q_p[j_p(r)][f], and per part q_p[J_p] of the factor in hand.
 *
 * T, the trained features: ids < num_attribute with a stored entry in a block row that some data row maps to (n_p[j] > 0) —
 * expand()'s T exactly.  Any other column is skipped like Q1's slot: its parameter keeps its bits and it does not count in m.
 *
 * RESIDUALS (k_als_residual and k_als_q_all per block over labels of zero, then one kernel per data row), in this order:
 *     yhat = w0;  for p ascending: yhat += yhat_p[j_p] - w0
 *     for f ascending: run = q_0[j_0][f], cross = 0;  for p = 1 ..: cross += run * q_p[j_p][f], run += q_p[j_p][f];
 *                      yhat += cross;  Q_f[r] = run
 *     e_r = yhat - y_r          (probit: fmhip_mcmc_task.h's draw around yhat, counter (row, attempt, t, 5))
 * The bias step takes sum e_r and N; the residuals are then formed again with the new bias.
 *
 * THE SWEEP.  For parameter group g = 0 (w), then every factor f: the parts in ascending order of their id ranges — the flat
 * sweep's ascending feature order, which is why the ranges must not interleave.  The plain part takes the flat walk's own
 * per-group pass over e and Q_f (h = x Q_f[r] - x^2 theta).  A relation takes, with theta the column's parameter, x = x_ji and
 * every sum over a column's entries in the walk's fixed order (one wave per column: lane l adds entries l, l + 64, ..., then
 * fmhip's wave sum; one workgroup: thread t adds t, t + size, ..., then its block sum):
 *   caches, once per (part, group), each a sum over the rows r -> j ascending (lists beyond FMHIP_RELATIONAL_SUM_CUT rows in
 *   chunks of that many, the chunks' sums added in order; one writer per address, no atomics):
 *     q_r = Q_f[r] - q_p[j]        E[j] = sum e_r    A[j] = sum q_r    B[j] = sum q_r * q_r    C[j] = sum e_r * q_r
 *   w:       sum h^2 += (x * x) * n[j]                                sum e*h += x * E[j]
 *            d = theta' - theta;  E[j] += n[j] * (x * d);  D[j] += x * d
 *            after the part:  e_r += D[j_p(r)]
 *   factor:  u = q_p[j] - x * theta
 *            sum h^2 += (x * x) * ((n[j] * (u * u) + (2 * u) * A[j]) + B[j])        sum e*h += x * (u * E[j] + C[j])
 *            d = theta' - theta, xd = x * d, u as above from the old q_p[j]:
 *            E[j] += xd * (n[j] * u + A[j]);  C[j] += xd * (u * A[j] + B[j]);  S1[j] += xd * u;  S2[j] += xd;  q_p[j] += xd
 *            after the part:  e_r += S1[j] + S2[j] * q_r;  Q_f[r] += S2[j]
 * theta <- theta' by ALS.scala:190-192's is_updatable, as the flat walk keeps it (no update: the caches are not touched).
 * No fused multiply-add anywhere.  The two walks — a wave per column of a level of the block's own schedule; one workgroup over
 * all columns in order — are chosen by the flat walk's rule (n_levels * 16 <= n_cols, FMHIP_ALS_LEVELS) and differ in the order
 * of a column's sum only.  There is no chip-wide two-launch step here: a block column of FMHIP_ALS_LONG (8192) entries or more
 * takes the 1024-thread workgroup walk behind its level's launch.
 *
 * HYPER-PARAMETERS.  sum theta and sum (theta - mu)^2 run over T per part (64 chunks of the part's columns, added in order), the
 * parts then in walk order.  part_groups = 0: one lambda and one mu per parameter group, fmhip_mcmc.h's state.  part_groups = 1:
 * A PART IS AN ATTRIBUTE GROUP — lambda and mu are (k + 1) x P laid out as in fmhip_mcmc_groups.h ([g * P + p], p the part's place
 * in the order GIVEN: what RelationalData.meta() names), drawn with its counters (g + (p << 16)); the group counts are the trained
 * features per part.  Read and set them with fmhip_mcmc_get_group_state / _set_group_state; fmhip_mcmc_set_groups is refused.
 * NOISE is keyed by (feature id, parameter group, t, stream) as ever: a relational run with seed s draws the numbers the flat run
 * on the expanded rows draws, and the two differ by rounding only.
 *
 * The handle is an ordinary fmhip_mcmc_t: _epoch (one host synchronisation, as ever), _get_state / _set_state, _reset_average,
 * _predictions, _latent_targets and _destroy work on it unchanged.  It borrows the model and the relational datasets.
 * FMHIP_ERR_UNSUPPORTED, the model unchanged, each message naming the item: parts whose id ranges interleave (the two parts and
 * the offending feature); a relational dataset of more than one batch; for any part everything fmhip_als_epoch refuses (a repeated
 * feature in a block row, a hot block or row blocks, weights); a model set to the logistic loss or to pairs.  A general group table
 * is not supported: only "a part is a group".  FMHIP_ERR_INVALID: both test sets given, a test set wider than the model.
 */
#ifndef FMHIP_MCMC_RELATIONAL_H
#define FMHIP_MCMC_RELATIONAL_H
#include "fmhip_mcmc_task.h"
#include "fmhip_mcmc_groups.h"
#include "fmhip_relational.h"

#ifdef __cplusplus
extern "C" {
#endif

/* test_relational / test_flat: at most one of the two (both NULL: no test set).  A relational test set is scored in fp64 by the
 * residual rule above; it normally shares the train set's blocks under other mappings.  opts, task_opts: NULL = the defaults. */
int fmhip_mcmc_create_relational(fmhip_model_t m, fmhip_relational_t train, fmhip_relational_t test_relational /* nullable */,
                                 fmhip_dataset_t test_flat /* nullable */, const fmhip_mcmc_opts *opts /* nullable */,
                                 const fmhip_mcmc_task_opts *task_opts /* nullable */, int32_t part_groups, fmhip_mcmc_t *out);

#ifdef __cplusplus
}
#endif
#endif /* FMHIP_MCMC_RELATIONAL_H */
