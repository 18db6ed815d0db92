/*
 * fmhip_metrics.h — ranking metrics of a binary classifier (libfmhip.so): the area under the ROC curve, and its per-group
 * form (GAUC: the AUC inside each group of rows — a user's impressions — averaged by the groups' row counts).
 *
 * AUC is a rank statistic and therefore an exact integer count: with t = [y > 0] the label of a row and yhat its prediction,
 *
 *     2 U = sum over (positive, negative) pairs of the same group of  2 [yhat_p > yhat_n] + [yhat_p == yhat_n],   AUC = 2 U / (2 P N)
 *
 * The device holds the predictions, the labels and a stable radix sort, so a held-out set is scored with one forward pass, one
 * sort of one 64-bit word per row and a few scans; nothing per row leaves the GPU, and the answer is exact to the last tied pair.
 *
 * Same library and conventions as fmhip.h (plain C, int status, fmhip_last_error, never throws), which this header includes.
 *
 * Semantics, of both calls:
 *  - order: predictions are compared as the fp32 values fmhip_predict returns.  -0 and +0 tie; +-Inf rank as themselves; NaN ranks
 *    below -Inf and ties with every other NaN (the rule of fmhip_topk.h).  Rows with a non-finite prediction are counted in
 *    stats.nonfinite and are never masked.
 *  - labels: t = [y > 0], as fmhip_logloss (so {-1, +1} and {0, 1} labels both work).
 *  - group == NULL: all rows form one group, and gauc == auc bit for bit.
 *  - group ids: any ints in [0, 2^31), unsorted and sparse.  A negative id: FMHIP_ERR_INVALID (the message names the row).
 *  - only pairs inside a group count.  A group with a single class is counted in `groups`, not in `groups_scored`, and contributes
 *    nothing to u2, pairs or gauc.
 *  - n == 0: FMHIP_OK, zero counts, NaN for both ratios.
 *  - refusals made before any handle or device is touched: out == NULL or out->struct_size != sizeof(fmhip_auc_result):
 *    FMHIP_ERR_INVALID; n >= 2^31: FMHIP_ERR_UNSUPPORTED.
 *  - determinism: every integer field is exact; gauc is an fp64 sum over the groups in ascending id order whose shape is fixed (it
 *    does not depend on the device or on how the work is launched); with exactly one scored group gauc is that group's AUC itself.
 *    Repeated calls return identical bits.
 *  - memory: a few arrays of 4-8 B per row (28 B per row in all, plus the sort's temporary storage), allocated for the call and freed when it returns; nothing
 *    is cached in the model.
 *  - data-parallel training: AUC is not additive over shards of the rows, so there is no fmhip_dp_* variant.  Gather the ranks'
 *    predictions (and labels, and group ids) on one rank and call fmhip_auc_scores.
 */
#ifndef FMHIP_METRICS_H
#define FMHIP_METRICS_H
#include "fmhip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fmhip_auc_result {
    int32_t  struct_size;      /* in: sizeof(fmhip_auc_result) */
    int32_t  reserved;
    uint64_t u2;               /* sum over scored groups of 2*U_g (exact) */
    int64_t  pairs;            /* sum over scored groups of positives_g * negatives_g */
    int64_t  positives, negatives;   /* over ALL rows: t = [y > 0] as fmhip_logloss */
    int64_t  groups, groups_scored;  /* distinct group ids; those with both classes */
    double   auc;              /* (double)u2 / (2.0 * (double)pairs); NaN when pairs == 0 */
    double   gauc;             /* sum_g rows_g * AUC_g / sum_g rows_g over scored groups; NaN when none */
} fmhip_auc_result;

/* Scores already on the host — the core, and what a data-parallel caller uses after gathering its ranks' predictions.  score, y
 * (and group, if given) hold n entries; they are uploaded to `device` and ranked there.  FMHIP_ERR_INVALID: n < 0, or score or
 * y NULL with n > 0. */
int fmhip_auc_scores(int device, int64_t n, const float *score, const float *y,
                     const int32_t *group /* nullable: one group */, fmhip_auc_result *out);

/* A model over a dataset: FMModel.predict (fmhip_predict) of every row on the device, then the same core.  A SCORING call in the
 * sense of fmhip.h (re-entrant, the model's lock taken shared, a stream and a workspace of its own); a lazily decayed model scores
 * correctly; the model's loss and pairing do not matter.  `d` may be of either kind (fmhip_rows_create*, or a training dataset);
 * group: nullable, n_rows host ints in the dataset's row order.  stats: nullable, filled as fmhip_rmse fills it. */
int fmhip_auc(fmhip_model_t m, fmhip_dataset_t d, const int32_t *group /* nullable, n_rows host ints */,
              fmhip_auc_result *out, fmhip_stats *stats /* nullable; filled as fmhip_rmse fills it */);

#ifdef __cplusplus
}
#endif
#endif /* FMHIP_METRICS_H */
