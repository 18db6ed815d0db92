/*
 * fmhip_redraw.h — when the BPR trainer (fmhip_bpr.h) redraws its negatives: once per epoch, or before every batch under the model
 * as it then stands.  Dynamic negative sampling (fmhip_bpr_adaptive.h) and WSABIE's WARP (fmhip_warp.h) both draw at every update;
 * a draw made once per epoch lets batch b train on choices that were hardest for a model b updates old.
 *
 * A handle has a redraw mode: FMHIP_REDRAW_EPOCH (a new handle's; every call does what it did before this header existed — the same
 * random numbers, the same launches, the same bits) or FMHIP_REDRAW_BATCH.  The mode governs fmhip_bpr_epoch alone;
 * fmhip_redraw_step works in either.
 *
 * THE PER-BATCH EPOCH.  Batch b holds the pairs [p0, p1) = rows [row0, row0 + rows) / 2.  At epoch t the batches are visited in the
 * given order, and for each one, on the model's stream and with no host synchronisation in between:
 *   1. both blocks' forwards run once under the model AS IT STANDS NOW — the step's own; the draw reads their q rows and scores;
 *   2. the handle's sampler (uniform at n_cand = 1, the best of n_cand above, WARP when its switch is on) runs over the pairs
 *      [p0, p1) only, with the counters it always uses: attempt a of candidate c of pair p takes its words from the block of counter
 *      (p, (c << 4) | (a >> 2), t, stream 6).  A pair's candidate ROWS are therefore the rows the per-epoch draw at t gives; only the
 *      scores — and with them the choice, WARP's weight c_p and trial count N_p — come from the later model.  It writes the
 *      negatives' entries of these pairs (and their weights and trial counts under WARP) and nothing of any other pair;
 *   3. the candidates relation's inverse map of batch b is rebuilt; its four counts stay on the device;
 *   4. the rest of the step runs: the gather of the candidates relation reads its counts from the device, each clamped to the
 *      capacity of the batch's slices, on grids sized for the worst case.  What a work item sums and where it writes is fixed by the
 *      data, so the step's bits do not depend on where the counts were read.
 * The epoch ends in ONE synchronisation, which brings back every batch's counts (checked as after a per-epoch draw: FMHIP_ERR_HIP
 * with the counts in the message) and the sampler's counters per batch.
 *
 * fmhip_redraw_step without statistics synchronises nothing.  A call that needs the host's copy of the counts (fmhip_bpr_step,
 * fmhip_bpr_debug_inverse) or reads the draw from the host (fmhip_bpr_negatives, fmhip_warp_weights, fmhip_warp_trials) first
 * waits for the draws queued so far and fetches the counts, with one synchronisation.
 *
 * The uniform sampler does not read the model: a uniform handle ends a per-batch epoch with the same model bits and the same
 * negatives as a per-epoch one.
 *
 * WARP.  A per-batch WARP draw judges the hinge, picks the violator and sets the weight on the same model state the step trains.
 * A WARP draw stands (fmhip_bpr_step, fmhip_warp_weights, fmhip_warp_trials) once every batch has been drawn since the switch was
 * last set, by a whole-set resample or batch by batch; fmhip_redraw_step itself needs no standing draw, it makes its batch's.
 *
 * Same library and conventions as fmhip.h (plain C, int status, fmhip_last_error, never throws); threads as fmhip_bpr.h.
 */
#ifndef FMHIP_REDRAW_H
#define FMHIP_REDRAW_H
#include "fmhip_warp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FMHIP_REDRAW_EPOCH 0 /* default: what every handle does without this header */
#define FMHIP_REDRAW_BATCH 1

/* The counters of the sampler that drew; those of the other samplers are 0.  uniform: attempts, forced; best of C: attempts,
 * forced, replaced; WARP: violated, trials.  pairs: the pairs drawn. */
typedef struct fmhip_redraw_stats {
    int64_t pairs;
    int64_t attempts;
    int64_t forced;
    int64_t replaced;
    int64_t violated;
    int64_t trials;
} fmhip_redraw_stats;

/* mode: FMHIP_REDRAW_EPOCH or FMHIP_REDRAW_BATCH; any other value: FMHIP_ERR_INVALID, the handle unchanged.  Takes effect with the
 * next fmhip_bpr_epoch. */
int fmhip_redraw_set(fmhip_bpr_t h, int mode);
int fmhip_redraw_get(fmhip_bpr_t h, int *mode);

/* One step of the loop above: draws the pairs of `batch` at epoch t >= 0 under m with the handle's sampler, rebuilds that batch's
 * inverse map and trains it.  Works in either mode.  stats: the step's, as fmhip_bpr_step's; draw: the sampler's counters over the
 * batch's pairs.  Both nullable; either one not NULL synchronises. */
int fmhip_redraw_step(fmhip_model_t m, fmhip_bpr_t h, int64_t t, int64_t batch, double eta, double reg0, double regw, double regv,
                      fmhip_stats *stats, fmhip_redraw_stats *draw);

/* The sampler's counters summed over the batches of the last fmhip_bpr_epoch run in FMHIP_REDRAW_BATCH mode; FMHIP_ERR_INVALID if
 * there was none. */
int fmhip_redraw_epoch_stats(fmhip_bpr_t h, fmhip_redraw_stats *out);

#ifdef __cplusplus
}
#endif
#endif /* FMHIP_REDRAW_H */
