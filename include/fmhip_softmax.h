/*
 * fmhip_softmax.h — the sampled-softmax loss for the BPR trainer (fmhip_bpr.h): the n_neg negatives of one interaction compete in
 * ONE loss, -log softmax(s+ | s+, s-_1 .. s-_n), instead of forming n_neg independent pairs.  It is the "softmax" loss of the
 * two-tower recommenders (Covington, Adams, Sargin: "Deep neural networks for YouTube recommendations", RecSys 2016) with the
 * log-Q correction of a sampled softmax under a non-uniform proposal (Bengio, Senecal: "Adaptive importance sampling to accelerate
 * training of a neural probabilistic language model", IEEE TNN 2008; Yi et al.: "Sampling-bias-corrected neural modeling for large
 * corpus item recommendations", RecSys 2019).  Only the residual changes (fmhip_pairing.h): everything after it is the pair step.
 *
 * A handle has a softmax switch (off in a new handle) and a log-Q request (off).  With the switch off every call takes the path it
 * took before this header existed: the same launches, the same bits.
 *
 * THE RULE.  Interaction j of a batch holds the pairs p = j n + q, q = 0 .. n - 1, n = n_neg: rows 2p (the positive i+, the same in
 * all n pairs) and 2p + 1 (negative i-_q).  After the step's forwards, all in fp32:
 *     d_q  = yhat[2p] - yhat[2p + 1]
 *     a_q  = -d_q - (lq[i-_q] - lq[i+])                  (the subtraction of the two lq first; without the correction a_q = -d_q
 *                                                          and no lq is read)
 *     mx   = max(0, a_0, .., a_{n-1})
 *     Z    = exp(-mx) + sum_q exp(a_q - mx)
 *     pi_q = exp(a_q - mx) / Z
 *     g_q  = -pi_q,   e[2p] = g_q,   e[2p + 1] = -g_q
 *     loss_j = mx + log Z                                 (= -log softmax of the positive, whose logit is 0 on this scale)
 * The step minimises (1 / |B|) sum_j loss_j over a batch, |B| its ROW count as for every pair rule, so that n_neg = 1 without the
 * correction is the logistic pair rule g = -sigma(-d) up to rounding.  The positive's block row occurs n times in the batch, once
 * per pair, and its residuals add up to -sum_q pi_q in the relational step's segmented sum; the gather sums, both blocks'
 * backwards and the SGD / AdaGrad update are the pair step's as they stand (fmhip_model_set_optimizer).  The model's loss
 * (fmhip_model_set_loss) is neither read nor changed while the switch is on.
 *
 * ORDER.  The fp32 order of mx and Z is fixed by n alone, never by the grid or by where the interaction lies in its batch, so
 * results are bit-identical run to run.  With G = the least power of two >= n, 64 at most: lane l of a group of G takes
 * q = l, l + G, .. ascending — a running fmaxf from -inf, then the sum of expf(a_q - mx) from 0 — and the lanes are combined by an
 * xor tree (strides G/2 .. 1; both sides of a stride add the same two floats, so every lane holds the same result);
 * mx = fmaxf(0, that maximum), Z = expf(-mx) + that sum.
 *
 * NON-FINITE.  If any d_q of an interaction is not finite, every g_q of that interaction is 0 and the P rows of its pairs are
 * exact zeros: the interaction adds nothing to any gradient, to the loss or to top1.  Its rows with a non-finite prediction
 * still count in the statistics' non-finite slot.
 *
 * DUPLICATES.  The sampler draws with replacement: the same row may be the negative of several pairs of one interaction.  They
 * are kept as drawn, each with its own term in Z.
 *
 * STATISTICS of a step are the pair rule's: rows = 2 pairs, sum_e exactly 0, sse = 2 sum g^2.
 *
 * THE LOG-Q CORRECTION.  lq[i] = (float) log(w_i / S), w the handle's proposal weights (fmhip_proposal.h), S their sum, index
 * ascending, in fp64 on the host; M floats, uploaded.  The table is rebuilt when the proposal or the switch changes, before the
 * next step reads it.  Under the uniform proposal lq would be constant: the table is not built, the term is not evaluated, and
 * the bits are those of logq = 0.  It corrects for the PROPOSAL's probabilities w_i / S — not for the rejection of a context's
 * positives, which renormalises them per context and is left out, nor for the candidate choice of the best-of-C rule.
 *
 * WHICH CALLS CHANGE.  With the switch on, fmhip_bpr_step, fmhip_bpr_epoch and fmhip_redraw_step train the rule above.  The
 * samplers are untouched: uniform and best-of-C draws (fmhip_bpr_adaptive.h; the softmax then runs over each pair's kept
 * candidate), both redraw modes (fmhip_redraw.h) and the proposal compose with it.  WARP (fmhip_warp.h) does not: each switch is
 * refused while the other is on.  fmhip_bpr_pair_logloss is unchanged.
 *
 * Same library and conventions as fmhip.h (plain C, int status, fmhip_last_error, never throws); threads as fmhip_bpr.h, and
 * fmhip_softmax_loss is a scoring call like fmhip_bpr_pair_logloss.
 */
#ifndef FMHIP_SOFTMAX_H
#define FMHIP_SOFTMAX_H
#include "fmhip_proposal.h"

#ifdef __cplusplus
extern "C" {
#endif

/* enabled, logq: 0 or not 0 (logq is kept while the proposal is uniform and takes effect once it is weighted).  Refused with
 * FMHIP_ERR_INVALID, the handle unchanged, when enabling while the WARP switch is on, or while a batch would split an interaction
 * (batch_pairs % n_neg != 0 with more than one batch).  Correspondingly fmhip_warp_set(h, 1, ..) is refused while this switch is
 * on.  Every call drops the standing probabilities.  Waits for the steps queued so far. */
int fmhip_softmax_set(fmhip_bpr_t h, int enabled, int logq);
int fmhip_softmax_get(fmhip_bpr_t h, int *enabled, int *logq);

/* The mean over the interactions of loss_j of the current draw under m, whatever the switch; corrected when the correction is
 * in force (fmhip_softmax_logq).  top1: the share of interactions whose positive has the strictly largest corrected logit (every a_q < 0).
 * loss, top1, stats: nullable.  stats: rows, sum_e = 0, sse = 2 sum pi^2, nnz, nonfinite.  A batch that splits an interaction:
 * FMHIP_ERR_INVALID. */
int fmhip_softmax_loss(fmhip_model_t m, fmhip_bpr_t h, double *loss, double *top1, fmhip_stats *stats);

/* out[p] = pi of pair p as the last step of p's batch left it, n_pairs floats.  FMHIP_ERR_INVALID unless every batch has had a
 * step since fmhip_softmax_set. */
int fmhip_softmax_probs(fmhip_bpr_t h, float *out);

/* The M floats of lq; FMHIP_ERR_INVALID when the correction is not in force (switch off, logq off or a uniform proposal). */
int fmhip_softmax_logq(fmhip_bpr_t h, float *out);

#ifdef __cplusplus
}
#endif
#endif /* FMHIP_SOFTMAX_H */
