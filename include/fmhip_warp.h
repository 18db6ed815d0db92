/*
 * fmhip_warp.h — WARP for the BPR trainer (fmhip_bpr.h): the third rule of the family beside uniform negatives and the best of C
 * candidates (fmhip_bpr_adaptive.h).  Per pair the sampler looks through the handle's C candidates for the FIRST one that violates
 * a margin against the pair's positive, estimates the positive's rank from how many candidates that took, and the step trains a
 * hinge weighted by that rank.  (Weston, Bengio, Usunier: "WSABIE: Scaling up to large vocabulary image annotation", IJCAI 2011;
 * the loss the LightFM library made popular for implicit feedback.)  Pairs the model ranks correctly cost nothing, pairs it ranks
 * badly count more.
 *
 * A handle has a WARP switch (off in a new handle) and a margin m >= 0 (1 by default).  The number of trials is the handle's
 * candidate count C = n_cand, 1 <= C <= 64 (fmhip_bpr_set_candidates).
 *
 * DRAWING.  Candidate c = 0 .. C-1 of pair p at epoch t is the adaptive sampler's candidate (fmhip_bpr_adaptive.h, DRAWING), bit for
 * bit: never a positive of its context, candidate 0 the uniform sampler's draw.  WARP draws nothing of its own.
 *
 * SCORING.  The score of candidate row i for context row u is the adaptive sampler's
 *     s = yq_i[i] + <q_u[u], q_i[i]>                                     (fp32)
 * and the positive's score s+ is the same expression at the pair's positive row, formed by the same code in the same order — a
 * lane's 4-term fused chain, then an xor tree over the Kp / 4 lanes of a row — with floats >= k of the context's slice cleared.
 * q and yq are what one forward over each block leaves under the model AS IT STANDS WHEN THE DRAW IS MADE.
 *
 * CHOOSING.  thr = s+ - (float)m, one fp32 subtraction.  Candidate c VIOLATES iff s_c > thr: a strict test, so a tie is no violation
 * and a NaN on either side never violates.  N = 1 + the lowest violating c, or 0 when none of the C violates.  The pair's negative
 * is the violator's row, or candidate 0's row when N = 0.
 *
 * WEIGHT.  W[n] = (float) H(max(1, floor((M - 1) / n))) for n = 1 .. C, where M is the candidates block's row count and
 * H(r) = sum_{j = 1 .. r} 1 / j, summed in fp64 with j ascending on the host; the table (at most 64 floats) is uploaded, so host and
 * device agree by construction.  The pair's weight is c_p = W[N], or 0 when N = 0.  This is the paper's L(k) = sum 1 / j at the
 * estimated rank floor((M - 1) / N); the exact number of negatives of the pair's context is not used.
 *
 * THE STEP minimises (1 / |B|) sum_p c_p max(0, m - (yhat+_p - yhat-_p)) over a batch, |B| its ROW count as for every pair rule:
 *     d = yhat_2p - yhat_2p+1,   g = (d < (float)m) ? -1 : 0,   g <- c_p g,   e_2p = g,   e_2p+1 = -g
 * The hinge is judged AT THE STEP on the current model: a pair an earlier batch already fixed gives no gradient, whenever its draw
 * was made.  The weights c_p and the kept rows are the draw's: once per epoch by default, or under the model of the batch's own
 * step with the per-batch redraw (fmhip_redraw.h).  A NaN d gives g = 0 and is counted in the
 * statistics' non-finite slot.  The statistics are the pair rule's: sum_e exactly 0, sse = 2 sum g^2.  SGD and AdaGrad as the
 * model is set (fmhip_model_set_optimizer); the model's loss (fmhip_model_set_loss) is neither read nor changed while WARP is on.
 *
 * WHICH CALLS CHANGE.  With the switch on: fmhip_bpr_epoch runs the WARP resample, then the batches with the hinge;
 * fmhip_bpr_step trains the hinge on the standing WARP draw and is refused (FMHIP_ERR_INVALID) when there is none since the switch
 * was last set; fmhip_bpr_resample and fmhip_bpr_resample_adaptive are refused the same way and leave the handle as it was.
 * fmhip_bpr_pair_logloss is unchanged: it scores the current pairs with the logistic rule.  With the switch off every call takes
 * the path it took before this header existed: the same launches, the same bits.
 *
 * Same library and conventions as fmhip.h (plain C, int status, fmhip_last_error, never throws); threads as fmhip_bpr.h.
 */
#ifndef FMHIP_WARP_H
#define FMHIP_WARP_H
#include "fmhip_bpr_adaptive.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fmhip_warp_stats {
    int64_t pairs;    /* pairs drawn (n_pairs) */
    int64_t violated; /* pairs with a violator among their C candidates (N > 0) */
    int64_t trials;   /* the sum of N over them */
} fmhip_warp_stats;

/* enabled: 0 or not 0.  margin negative or not finite: FMHIP_ERR_INVALID, the handle unchanged.  Takes effect with the next
 * resample; every call drops the standing WARP draw (weights and trial counts), so a step needs a new one. */
int fmhip_warp_set(fmhip_bpr_t h, int enabled, double margin);
int fmhip_warp_get(fmhip_bpr_t h, int *enabled, double *margin);

/* Redraws every pair's negative at epoch t >= 0 by the rule above under model m, writes the pairs' weights and trial counts and
 * rebuilds the candidates relation's inverse map (one synchronisation).  The switch must be on.  The model as for
 * fmhip_bpr_resample_adaptive: its lazily decayed tables are folded to scale 1, its parameters are not changed.  stats: nullable. */
int fmhip_warp_resample(fmhip_model_t m, fmhip_bpr_t h, int64_t t, fmhip_warp_stats *stats);

/* The standing WARP draw, read back: out[p] = c_p and out[p] = N_p for the n_pairs pairs (the rows: fmhip_bpr_negatives).
 * FMHIP_ERR_INVALID when no WARP draw stands. */
int fmhip_warp_weights(fmhip_bpr_t h, float *out);
int fmhip_warp_trials(fmhip_bpr_t h, int32_t *out);

#ifdef __cplusplus
}
#endif
#endif /* FMHIP_WARP_H */
