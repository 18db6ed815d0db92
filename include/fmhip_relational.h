/*
 * fmhip_relational.h — relational data (libfmhip.so): block-structure FM training and scoring (Rendle, "Scaling Factorization
 * Machines to Relational Data", VLDB 2013) — what the reference's S/fm/bs stub and FM.withRelation were heading for.
 *
 * A recommender's rows are joins: (user, item) with the user's whole feature row — id, demographics, the rated-items history —
 * and the item's whole feature row copied into every example.  The flat dataset repeats each user's row once per rating; its
 * step gathers (nnz_user + nnz_item) parameter rows per example.  A RELATIONAL dataset keeps each side once:
 *
 *   - a RELATION is a BLOCK — an ordinary training fmhip_dataset_t of J_b rows, created with batch_rows = 0 (one batch) and
 *     labels 0 — and a MAPPING int32[N] with entries in [0, J_b): data row r uses block row mapping[r];
 *   - a relational dataset is N labels, m >= 1 relations (at most FMHIP_RELATIONS_MAX), an optional PLAIN PART — an ordinary
 *     training dataset of the same N rows batched by the same batch_rows: a block under the identity mapping, the reference's
 *     "additional features" — and batch_rows.
 * It stands for the flat dataset whose row r holds relation 0's entries of block row mapping_0[r], then relation 1's, ..., then
 * the plain part's row r.  Feature ids are global; `dimension` is the largest over all parts.
 *
 * THE RULE.  With q_b[j], yhat_b[j] a block row's factor sums and prediction (fmhip_term_q, fmhip_predict of the block):
 *
 *     Q_r    = sum_b q_b[j_b(r)]
 *     yhat_r = w0 + sum_b (yhat_b[j_b(r)] - w0) + sum_{b < b'} <q_b[j_b(r)], q_b'[j_b'(r)]>
 *     P_b[j] = sum_{r: j_b(r) = j} e_r Q_r        e_b[j] = sum_{r: j_b(r) = j} e_r
 *     G_V[i] = sum_j x_ji P_b[j] - v_i sum_j x_ji^2 e_b[j]        G_w[i] = sum_j x_ji e_b[j]        (i a feature of block b)
 *
 * — the flat dataset's prediction and gradient, with every block row walked once per step instead of once per reference.  e_r is
 * the residual of the model's loss (fmhip_model_set_loss); the update is the model's optimizer's (SGD or AdaGrad), always the
 * dense pass: a relational step walks whole blocks, so there is no rows-only, lazy-decay or fused update.
 *  - the parts' feature sets must be pairwise DISJOINT (every part's backward stores its gradient rows; the reference likewise
 *    gives each relation its own attribute range): FMHIP_ERR_INVALID at create, the message names the first shared feature and
 *    the two parts.
 *  - create also refuses, each with a message that names the item: a mapping entry outside [0, J_b) (FMHIP_ERR_INVALID), a block
 *    created for scoring only (fmhip_rows_create), a block with more than one batch, a weighted block or plain part
 *    (FMHIP_ERR_UNSUPPORTED), a plain part whose row count or batching disagrees (FMHIP_ERR_INVALID).  The checks of the
 *    mappings and of the feature sets run on the host.
 *  - FMHIP_ERR_UNSUPPORTED from the training calls, the model unchanged: a model set to pairs (fmhip_model_set_pairing).
 *  - the handle BORROWS its blocks and its plain part: they must outlive it.  It owns device copies of the labels and the mappings,
 *    per (batch, relation) the inverse map (the block rows the batch touches and, for each, the batch's rows that point at it,
 *    ascending — O(N m + touched block rows) in all), and the training workspace (per block: q rows, predictions, P_b, e_b).
 *  - the statistics of a step or an epoch are those of the residuals e_r over the data rows; nnz counts the stored nonzeros the
 *    step walks (every block once, the plain part's batch).
 *
 * Same library and conventions as fmhip.h (plain C, int status, fmhip_last_error, never throws), which this header includes.
 *  - threads: create / destroy / info touch no model.  _sgd_step / _sgd_epoch CHANGE the model (its lock exclusive) and use the
 *    handle's workspace: one training call per relational handle at a time.  (They are asynchronous like fmhip_sgd_step; a step that
 *    follows on ANOTHER model's stream waits on the device for the handle's previous step, so two models may take turns on one handle
 *    without a synchronise in between.)  _predict / _rmse / _logloss are SCORING calls in the
 *    sense of fmhip.h — re-entrant, the model's lock shared, a stream and a workspace of their own — and only read the handle.
 *  - determinism: results are bit-identical run to run and do not depend on how the work is launched (every address has one writer: P_b is a
 *    segmented sum in ascending row order, lists beyond FMHIP_RELATIONAL_SUM_CUT rows in chunks of that many, the chunks'
 *    sums added in order).
 */
#ifndef FMHIP_RELATIONAL_H
#define FMHIP_RELATIONAL_H
#include "fmhip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FMHIP_RELATIONS_MAX 8
#define FMHIP_RELATIONAL_SUM_CUT 256

typedef struct fmhip_relational *fmhip_relational_t;

/* y: n_rows labels.  blocks / mappings: n_relations block handles and, for each, n_rows int32 block-row indices.  plain: NULL,
 * or a training dataset of n_rows rows batched by batch_rows.  batch_rows <= 0 (or > n_rows): one batch. */
int fmhip_relational_create(int device, int64_t n_rows, const double *y, int32_t n_relations, const fmhip_dataset_t *blocks,
                            const int32_t *const *mappings, fmhip_dataset_t plain /* nullable */, int64_t batch_rows,
                            fmhip_relational_t *out);
int fmhip_relational_destroy(fmhip_relational_t r);
/* every out pointer is nullable */
int fmhip_relational_info(fmhip_relational_t r, int64_t *n_rows, int64_t *dimension, int64_t *batch_rows, int64_t *n_batches,
                          int32_t *n_relations);

/* FMModel.predict of every data row (yhat: n_rows doubles); RMSE and mean log-loss as fmhip_rmse / fmhip_logloss define them.  Every
 * block's q-mode pass runs ONCE per call; a lazily decayed model scores correctly. */
int fmhip_relational_predict(fmhip_model_t m, fmhip_relational_t r, double *yhat);
int fmhip_relational_rmse(fmhip_model_t m, fmhip_relational_t r, double *rmse, fmhip_stats *stats /* nullable */);
int fmhip_relational_logloss(fmhip_model_t m, fmhip_relational_t r, double *logloss, fmhip_stats *stats /* nullable */);

/* One mini-batch step on batch `batch` / one epoch over all batches (order: NULL = ascending, else n_batches batch indices), as
 * fmhip_sgd_step / fmhip_sgd_epoch. */
int fmhip_relational_sgd_step(fmhip_model_t m, fmhip_relational_t r, int64_t batch, double eta, double reg0, double regw, double regv,
                              fmhip_stats *stats /* nullable */);
int fmhip_relational_sgd_epoch(fmhip_model_t m, fmhip_relational_t r, double eta, double reg0, double regw, double regv,
                               const int64_t *order /* nullable */, fmhip_stats *stats /* nullable */);

#ifdef __cplusplus
}
#endif
#endif /* FMHIP_RELATIONAL_H */
