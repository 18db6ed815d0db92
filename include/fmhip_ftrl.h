/*
 * fmhip_ftrl.h — FTRL-Proximal with L1 (libfmhip.so): a third update rule for every SGD step path, and the sparsity it produces.
 *
 * Wide click models (2^25 hashed features, logistic loss) are usually trained with FTRL-Proximal (McMahan et al., "Ad click
 * prediction: a view from the trenches"; the `ftrl` optimizer of xLearn and alphaFM): per-coordinate rates like AdaGrad's, plus an
 * L1 term that leaves most of the model EXACTLY zero.  L2 (regw, regv of the other rules) only shrinks.
 *
 * THE RULE.  Per scalar parameter theta (w0, every w_i, every v_{f,i}) the model keeps two fp32 states shaped like the parameter
 * tables: zeta — the rule's z pre-multiplied by the step size — and n, the sum of squared gradients.  A training call's arguments
 * mean: eta = alpha, the step size; reg0 / regw / regv = lambda_2, the L2 of the closed form (NOT a decay).  The rule's own settings
 * are beta >= 0 and the L1 of the linear weights and of the factors, l1w, l1v >= 0 (w0 has no L1).  With g the plain mean gradient of
 * fmhip.h's training section, g_theta / |batch|, nothing folded in:
 *
 *     g == 0:   theta, zeta, n unchanged — exactly, whatever l1 and lambda_2 are
 *     n'     = n + g^2,   r = sqrt(n'),   r0 = sqrt(n)
 *     zeta'  = zeta + eta g - (r - r0) theta                      (r - r0 formed as g^2 / (r + r0): no cancellation)
 *     theta' = |zeta'| <= eta l1  ?  +0  :  -(zeta' - sign(zeta') eta l1) / (beta + r + eta lambda_2)
 *
 *  - zeta = alpha z instead of z: nothing in the state depends on alpha, so eta may change from step to step and the state can be
 *    made when the rule is set.  With l1 = lambda_2 = 0 the rule is AdaGrad with eps = beta: theta' = theta - eta g / (beta + sqrt(n')).
 *  - the g == 0 case is what the rule buys a wide model: a feature no row of the batch holds keeps every bit of its parameters and
 *    its state under ANY regularisation, so the update of the touched rows only (fmhip_sgd_step on a batch that touches at most half
 *    of the model) and FMHIP_EXCHANGE_TOUCHED are exact with l1, regw, regv > 0 — bit for bit the dense update.  AdaGrad with
 *    regularisation rewrites the whole model each step.
 *  - its price: for a parameter touched for the FIRST time (its zeta is still the proximal centre of the init, which knows nothing of
 *    l1 and lambda_2) the rule is discontinuous at g = 0 — any g != 0, however small, applies the L1 / L2 shrink of a first touch,
 *    g == 0 applies nothing.  A touched parameter's g is zero in exact arithmetic only in narrow cases (the factors of a feature
 *    seen only in rows that hold nothing else; w0 under FMHIP_PAIRING_ADJACENT, whose residuals sum to exactly zero), and there
 *    floating point may say either; both follow the rule, and from the next touch on the parameter is at its closed form, where
 *    the rule is continuous.
 *  - the tables stay at scale 1; there is no lazy decay under this rule.
 *  - arithmetic: fp32, correctly rounded square roots and divisions, one writer per element, fixed order: bit-identical run to run
 *    and on every path.
 *  - it applies to every training call the loss applies to — fmhip_sgd_step / _epoch, fmhip_step_compute / _forward / _backward /
 *    _apply, fmhip_relational_sgd_*, fmhip_bpr_step / _epoch, both losses, both pairings, weighted datasets, and the dense,
 *    pipelined and touched fmhip_dp_* modes; fmhip_dp_plan agrees the rule's four settings over the ranks by their bits, as it agrees
 *    AdaGrad's.  Equal state CONTENTS on every rank are the caller's job, as equal parameters are.
 *  - FMHIP_ERR_UNSUPPORTED: FMHIP_EXCHANGE_SHARDED (each rank's state would hold its own share only) — at fmhip_dp_plan and at any
 *    step, on every rank.
 *
 * THE STATE.  fmhip_model_set_ftrl makes it: n = initial_accumulator everywhere, zeta = -theta (beta + sqrt(n)) — the proximal centre
 * at the current parameters, so that an initialised V ~ N(0, sigma) survives until the gradients say otherwise.  On a model under
 * this rule fmhip_model_set_params(_f32), fmhip_model_init_normal and fmhip_als_epoch re-derive zeta from the new parameters and the
 * current n in the same way: theta and zeta never disagree.  fmhip_model_set_params(_f32) and fmhip_als_epoch do so for every
 * parameter whose fp32 value CHANGED; one whose bits stay keeps its zeta — a caller that writes the model's own values back (a host
 * mirror that uploads its fields before every call, as include/sparkfm.hpp's does) loses no state.  The state is two more copies of
 * the model on the device.
 *
 * Same library and conventions as fmhip.h (plain C, int status, fmhip_last_error, never throws), which this header includes.
 *  - threads: the setters take the model's lock exclusively; fmhip_model_get_ftrl_state and fmhip_model_nonzeros take it shared.
 */
#ifndef FMHIP_FTRL_H
#define FMHIP_FTRL_H
#include "fmhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The third update rule's number: what a model under FTRL-Proximal reports (a changed-rule message of a data-parallel step, say).
 * It is NEVER accepted by fmhip_model_set_optimizer, which keeps answering FMHIP_ERR_INVALID for it: the rule has four settings of
 * its own and is set by fmhip_model_set_ftrl. */
enum { FMHIP_OPT_FTRL = 2 };

/* Puts the model under FTRL-Proximal.  A pending lazy-decay scale is folded first; zeta and n are allocated, n filled with
 * initial_accumulator and zeta derived from the current parameters (above).  The SAME four settings again (bit-equal) on a model
 * already under the rule are a no-op that keeps the state — learners call this before every epoch; different settings re-initialise
 * it.  fmhip_model_set_optimizer(SGD or ADAGRAD) on such a model frees the FTRL state first; this call on an AdaGrad model replaces
 * its accumulators.  The loss and the pairing are untouched.
 * FMHIP_ERR_INVALID, checked before the model is looked at: beta, initial_accumulator, l1w or l1v not finite or < 0;
 * beta + sqrt(initial_accumulator) == 0 (the first step would divide by zero). */
int fmhip_model_set_ftrl(fmhip_model_t m, double beta, double initial_accumulator, double l1w, double l1v);

/* The state, for checkpoints: the layout of fmhip_model_get_params — z0 / n0 of w0, zw[i] / nw[i] of w_i (n + 1 entries each),
 * zv[f + i*k] / nv[f + i*k] of v_{f,i} ((n + 1) * k each).  get: any pointer may be NULL.  set: zw, zv, nw, nv must not be NULL;
 * every n must be finite and >= 0, every zeta finite (checked before the model is looked at for the two scalars, before any copy for
 * the arrays; the message names the first offending entry).  Parameters and state written back into a model made with the same
 * settings continue the run bit for bit.  FMHIP_ERR_INVALID on a model that is not under FTRL-Proximal
 * (fmhip_model_get/set_optimizer_state of fmhip_experimental.h likewise keep refusing a model that is not under AdaGrad). */
int fmhip_model_get_ftrl_state(fmhip_model_t m, double *z0, double *zw, double *zv, double *n0, double *nw, double *nv);
int fmhip_model_set_ftrl_state(fmhip_model_t m, double z0, const double *zw, const double *zv,
                               double n0, const double *nw, const double *nv);

/* Exact counts over the model as it is on the device, under any rule (a lazily decayed model counts the same: a scale moves no zero):
 * w_nonzero — linear weights w_i != 0 of the n + 1; v_nonzero — factors v_{f,i} != 0 of the (n + 1) * k; features_all_zero — features
 * i whose w_i and whole row v_{.,i} are zero (a serving table can drop them).  -0 counts as zero.  Any pointer may be NULL. */
int fmhip_model_nonzeros(fmhip_model_t m, int64_t *w_nonzero, int64_t *v_nonzero, int64_t *features_all_zero);

#ifdef __cplusplus
}
#endif
#endif /* FMHIP_FTRL_H */
