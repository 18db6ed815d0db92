/*
 * fmhip_bpr.h — the BPR trainer (libfmhip.so): pairwise ranking on implicit feedback over a block of contexts (users) and a block
 * of candidates (items), the negatives drawn on the device afresh for every epoch.  (Rendle, Freudenthaler, Gantner, Schmidt-Thieme:
 * "BPR: Bayesian Personalized Ranking from Implicit Feedback", UAI 2009.)
 *
 * fmhip_pairing.h trains pairs of adjacent rows of a flat dataset and leaves the choice of the `other` row to the caller;
 * fmhip_relational.h trains single rows over blocks.  This handle joins the two: it takes the two blocks fmhip_topk and fmhip_rank
 * take and a list of observed (context row, candidate row) interactions, and trains
 *
 *     -log sigma(yhat(u, i+) - yhat(u, i-))        (the model's loss logistic; squared: the squared pair loss of fmhip_pairing.h)
 *
 * on the relational step.  No joined row and no per-epoch dataset is ever built.
 *
 * THE LAYOUT IT STANDS FOR.  With n_pairs = n_neg * n_inter, pair p belongs to interaction p / n_neg (the interactions in the
 * order given to create).  The handle is a relational dataset of N = 2 n_pairs rows over two relations:
 *     y_2p = 1, y_2p+1 = 0      contexts: map[2p] = map[2p+1] = u_p      candidates: map[2p] = i+_p (fixed), map[2p+1] = i-_p (redrawn)
 * A batch is batch_pairs consecutive pairs (2 batch_pairs rows; batch_pairs <= 0 or > n_pairs: one batch).
 *
 * THE SAMPLER.  Attempt a = 0 .. 63 of pair p at epoch t takes word a & 3 of the Philox4x32-10 block of counter
 * (p, a >> 2, t, stream 6) under key `seed`; the candidate row is c = (word * M) >> 32, M the candidates' rows, accepted if c is
 * not among the positives of the pair's context (every candidate row an interaction names for it).  All 64 rejected: from the last
 * c on, c = (c + 1) mod M until c is no positive — the pair counts as `forced`.  A drawn row is NEVER a positive of its context.
 * The draw is integer arithmetic and does not depend on the model: the same (seed, t) gives the same rows on any device.
 *
 * THE STEP is fmhip_relational_sgd_step's with the pair residual: after both blocks' forward, Q_r and yhat_r per row, then
 * e_2p = g_p, e_2p+1 = -g_p with g of fmhip_pairing.h, then the segmented sums, the blocks' backward and the dense update of the
 * model's optimizer (SGD or AdaGrad).  The calls are pairwise by construction: they neither read nor change the model's pairing
 * flag (fmhip_model_set_pairing).  The candidates relation's inverse map is rebuilt on the device after every resample (one
 * synchronisation per resample, none per step).
 *  - the statistics are those of the pair rule: rows = 2 * pairs, sum_e exactly 0, sse = 2 sum g^2.
 *  - create refuses, each with a message that names the item: a weighted or scoring-only block (FMHIP_ERR_UNSUPPORTED); a block with
 *    more than one batch, a feature id the two blocks share, an interaction that names a row outside either block, a context whose
 *    positives are ALL candidate rows (no negative exists), fewer than 2 candidate rows, n_neg < 1, 2 n_pairs >= 2^31
 *    (FMHIP_ERR_INVALID).
 *  - the handle BORROWS the two blocks: they must outlive it.
 *  - threads: as fmhip_relational.h — one training call (or resample) per handle at a time; fmhip_bpr_pair_logloss is a scoring
 *    call (re-entrant, the model's lock shared) and only reads the handle.
 *  - determinism: results are bit-identical run to run and do not depend on how the work is launched.
 *
 * Same library and conventions as fmhip.h (plain C, int status, fmhip_last_error, never throws).
 */
#ifndef FMHIP_BPR_H
#define FMHIP_BPR_H
#include "fmhip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fmhip_bpr *fmhip_bpr_t;

typedef struct fmhip_bpr_sample_stats {
    int64_t attempts; /* attempts over all pairs (>= pairs) */
    int64_t forced;   /* pairs whose 64 attempts were all rejected */
} fmhip_bpr_sample_stats;

/* contexts / candidates: single-batch training datasets (labels unused).  inter_ctx / inter_cand: n_inter >= 1 interactions, in
 * training order.  The negatives are drawn at t = 0 before the call returns. */
int fmhip_bpr_create(int device, fmhip_dataset_t contexts, fmhip_dataset_t candidates, int64_t n_inter, const int32_t *inter_ctx,
                     const int32_t *inter_cand, int32_t n_neg, int64_t batch_pairs, uint64_t seed, fmhip_bpr_t *out);
int fmhip_bpr_destroy(fmhip_bpr_t h);
/* every out pointer is nullable */
int fmhip_bpr_info(fmhip_bpr_t h, int64_t *n_pairs, int64_t *dimension, int64_t *batch_pairs, int64_t *n_batches, int32_t *n_neg);

/* redraws every pair's negative at epoch t >= 0 and rebuilds the candidates relation's inverse map; stats: nullable */
int fmhip_bpr_resample(fmhip_bpr_t h, int64_t t, fmhip_bpr_sample_stats *stats);
/* out: n_pairs candidate rows, the current draw */
int fmhip_bpr_negatives(fmhip_bpr_t h, int32_t *out);

/* One step on batch `batch` of the current draw / one epoch: resample at t, then every batch (order: NULL = ascending, else
 * n_batches batch indices).  Asynchronous as fmhip_sgd_step. */
int fmhip_bpr_step(fmhip_model_t m, fmhip_bpr_t h, int64_t batch, double eta, double reg0, double regw, double regv,
                   fmhip_stats *stats /* nullable */);
int fmhip_bpr_epoch(fmhip_model_t m, fmhip_bpr_t h, int64_t t, double eta, double reg0, double regw, double regv,
                    const int64_t *order /* nullable */, fmhip_stats *stats /* nullable */);

/* mean pair log-loss and concordance of the current pairs, as fmhip_pair_logloss defines them; concordance, stats: nullable */
int fmhip_bpr_pair_logloss(fmhip_model_t m, fmhip_bpr_t h, double *logloss, double *concordance, fmhip_stats *stats);

#ifdef __cplusplus
}
#endif
#endif /* FMHIP_BPR_H */
