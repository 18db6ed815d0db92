/*
 * fmhip_proposal.h — the distribution the BPR trainer (fmhip_bpr.h) draws its candidate rows from: uniform over the candidates
 * block, or in proportion to a weight per row.  Drawing negatives in proportion to count^0.75 is word2vec's noise distribution
 * (Mikolov et al., "Distributed representations of words and phrases and their compositionality", NIPS 2013) and the popularity
 * sampler of the implicit-feedback toolkits: under a skewed catalogue a uniform negative is almost always an easy tail row.
 *
 * A handle has a proposal: uniform on a new handle — every call then does what it did before this header existed, the same random
 * numbers, the same launches, the same bits — or a weighted one, given as M weights, M the candidates block's rows.  The proposal
 * is the sampler's third axis, beside the choice rule (keep the draw, the best of C: fmhip_bpr_adaptive.h, WARP's first violator:
 * fmhip_warp.h) and the redraw mode (fmhip_redraw.h), and composes with both: every candidate of every rule comes from it, in
 * fmhip_bpr_resample, fmhip_bpr_resample_adaptive, fmhip_warp_resample, fmhip_redraw_step, both modes of fmhip_bpr_epoch and the
 * two record calls.
 *
 * THE TABLE.  A weighted proposal is stored as an alias table (Walker 1977; Vose 1991) of M packed 8-byte buckets
 * {uint32 thresh, int32 alias}, which the device reads with one 8-byte load.  The host builds it once, in fp64, when the proposal
 * is set:
 *   S = the sum of the weights, index ascending; q_i = w_i / S * M.
 *   The small list holds the i with q_i < 1, the large list the others, both index-ascending; both are stacks: the last entry is
 *   taken first.  While neither is empty: l = small's last and g = large's last are taken off; bucket l becomes
 *   {floor(q_l * 2^32) clamped to 2^32 - 1, g}; q_g = (q_g + q_l) - 1; g goes onto small if q_g < 1 and back onto large otherwise.
 *   A bucket left on either list is never redirected: {2^32 - 1, its own index} — both sides of the draw's comparison give its own
 *   row, so no threshold of 2^32 is needed.
 * The probability the table gives row i is (thresh_i + the sum over the buckets j != i with alias_j = i of (2^32 - thresh_j)) /
 * (M 2^32), a bucket with alias_j = j counting as 2^32; it is w_i / S to within 2^-30 for M <= 4096.
 *
 * THE DRAW.  Attempt a = 0 .. 31 of candidate c of pair p at epoch t takes the Philox block of counter
 * (p, (c << 4) | (a >> 1), t, stream 6) and of it the words x0 = x[2 (a & 1)], x1 = x[2 (a & 1) + 1]: j = (x0 * M) >> 32, the row is
 * x1 < thresh[j] ? j : alias[j], accepted if it is not among the context's positives.  Two attempts a block and 16 blocks a
 * candidate: the c << 4 spacing of the uniform rule, which is why there are 32 attempts and not 64.  All 32 rejected: the uniform
 * rule's forced walk from the last row on, row = (row + 1) mod M until it is not listed, and the pair counts as forced.  A drawn
 * row is never a positive.  Every weight is positive, so fmhip_bpr_create's guarantee — a negative exists for every context —
 * carries over as it is.  Integer arithmetic only: host and device agree bit for bit, run after run.
 *
 * Equal weights give the uniform DISTRIBUTION and not the uniform rule's bits: the weighted draw spends two words an attempt.
 *
 * WARP.  The rank estimate floor((M - 1) / N) behind WARP's weights (fmhip_warp.h) assumes a uniform proposal.  It is kept
 * unchanged under a weighted one, where it estimates the rank among proposal-weighted items.
 *
 * Same library and conventions as fmhip.h (plain C, int status, fmhip_last_error, never throws); threads as fmhip_bpr.h.
 */
#ifndef FMHIP_PROPOSAL_H
#define FMHIP_PROPOSAL_H
#include "fmhip_redraw.h"

#ifdef __cplusplus
extern "C" {
#endif

/* weights: M doubles, every one finite and > 0 (their sum finite), or NULL for the uniform proposal.  Anything else:
 * FMHIP_ERR_INVALID naming the first bad row, the handle unchanged.  Takes effect with the next draw; the standing draw is left
 * as it is, and so is which WARP draw stands (fmhip_redraw.h: counted from fmhip_warp_set).  Waits for the draws queued so far. */
int fmhip_proposal_set(fmhip_bpr_t h, const double *weights);
/* *weighted: 0 under the uniform proposal, 1 under a weighted one */
int fmhip_proposal_get(fmhip_bpr_t h, int *weighted);
/* The table of the weighted proposal, M entries each (either array nullable); FMHIP_ERR_INVALID under the uniform proposal. */
int fmhip_proposal_table(fmhip_bpr_t h, uint32_t *thresh, int32_t *alias);

#ifdef __cplusplus
}
#endif
#endif /* FMHIP_PROPOSAL_H */
