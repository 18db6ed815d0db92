/*
 * fmhip_bpr_adaptive.h — adaptive negatives for the BPR trainer (fmhip_bpr.h): per pair the sampler draws C candidates and keeps the
 * one the current model scores highest.  (Zhang, Chen, Wang, Yu: "Optimizing top-N collaborative filtering via dynamic negative
 * item sampling", SIGIR 2013; Rendle, Freudenthaler: "Improving pairwise learning for item recommendation from implicit feedback",
 * WSDM 2014.)  Uniform negatives are soon scored far below the positive, sigma(yhat- - yhat+) is then about 0 and the pair's
 * gradient vanishes; the best of a handful of candidates keeps the pairs informative.
 *
 * A handle has a candidate count C = n_cand, 1 <= C <= FMHIP_BPR_MAX_CANDIDATES (64); a new handle has C = 1.
 *
 * DRAWING.  Candidate c = 0 .. C-1 of pair p at epoch t is the uniform sampler's rule (fmhip_bpr.h) with the counter's group word
 * offset: attempt a = 0 .. 63 takes word a & 3 of the Philox4x32-10 block of counter (p, (c << 4) | (a >> 2), t, stream 6) under
 * key `seed`; row = (word * M) >> 32, accepted if it is no positive of the pair's context; all 64 rejected: the forced walk from
 * the last row.  A candidate is NEVER a positive of its context.  Candidate 0 is the uniform sampler's draw bit for bit.  The
 * candidates are independent of one another: the same row may be drawn more than once.
 *
 * SCORING.  The score of candidate row i for context row u is
 *     s = yq_i[i] + <q_u[u], q_i[i]>                                     (fp32)
 * with q and yq what one forward over each block leaves under the model AS IT STANDS WHEN THE DRAW IS MADE (the relational
 * step's: yhat(u, i) = yq_u + yq_i - w0 + <q_u, q_i>).  yq_u[u] - w0 is the same for all candidates of a pair and is left out.  The
 * dot product is summed in an order the model's padded factor count alone fixes — never the launch shape — so the same model bits,
 * seed and t give the same rows run to run and device to device.
 *
 * CHOOSING.  The kept row is the FIRST strict maximum: candidate 0 starts as the incumbent and candidate c replaces it if its score
 * is strictly greater than the incumbent's.  Ties keep the earlier candidate; a NaN score never replaces the incumbent (and a NaN
 * incumbent is never replaced).
 *
 * WHEN.  fmhip_bpr_resample_adaptive draws every pair at once: the negatives are the hardest against the model at the moment of the
 * call, and a handle in its default redraw mode makes that call once per epoch — with one batch per epoch (batch_pairs = 0) exact
 * dynamic negative sampling, with several the later batches train on choices made before the earlier batches' updates.  The
 * per-batch redraw (fmhip_redraw.h) draws each batch's pairs under the model as it stands at that batch's step.
 *
 * WHICH CALLS ARE ADAPTIVE.  fmhip_bpr_resample_adaptive always; fmhip_bpr_epoch when the handle's n_cand > 1 (with n_cand = 1 it
 * runs exactly what it ran before this header existed).  fmhip_bpr_resample, which takes no model, and the draw inside
 * fmhip_bpr_create stay UNIFORM — candidate 0 — whatever n_cand is.
 *
 * Same library and conventions as fmhip.h (plain C, int status, fmhip_last_error, never throws); threads as fmhip_bpr.h (a resample
 * is a training call of the handle and of the model).
 */
#ifndef FMHIP_BPR_ADAPTIVE_H
#define FMHIP_BPR_ADAPTIVE_H
#include "fmhip_bpr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FMHIP_BPR_MAX_CANDIDATES 64

typedef struct fmhip_bpr_adaptive_stats {
    int64_t attempts; /* attempts over all candidates of all pairs (>= n_cand * pairs) */
    int64_t forced;   /* candidates whose 64 attempts were all rejected */
    int64_t replaced; /* pairs whose kept candidate is not candidate 0 */
} fmhip_bpr_adaptive_stats;

/* n_cand outside [1, FMHIP_BPR_MAX_CANDIDATES]: FMHIP_ERR_INVALID.  Takes effect with the next resample. */
int fmhip_bpr_set_candidates(fmhip_bpr_t h, int32_t n_cand);
int fmhip_bpr_get_candidates(fmhip_bpr_t h, int32_t *n_cand);

/* Redraws every pair's negative at epoch t >= 0 as the best of the handle's n_cand candidates under model m, and rebuilds the
 * candidates relation's inverse map (one synchronisation).  The model must hold the blocks' features (as for fmhip_bpr_step); its
 * lazily decayed tables are folded to scale 1, its parameters are not changed.  With n_cand = 1 the mapping, attempts and forced
 * are fmhip_bpr_resample's and replaced is 0.  stats: nullable. */
int fmhip_bpr_resample_adaptive(fmhip_model_t m, fmhip_bpr_t h, int64_t t, fmhip_bpr_adaptive_stats *stats);

#ifdef __cplusplus
}
#endif
#endif /* FMHIP_BPR_ADAPTIVE_H */
