/*
 * fmhip_ffm.h — field-aware factorization machines (libfmhip.so): the third model of xLearn / libffm (Juan et al., "Field-aware
 * factorization machines for CTR prediction", RecSys 2016) beside the library's degree-2 FM.  Every feature keeps one factor vector
 * PER FIELD, and a pair of entries interacts through the vectors each keeps for the other's field.  A model and kernels of their
 * own: nothing here touches fmhip_model_t, and nothing of fmhip.h's training calls takes these handles.
 *
 * THE MODEL.  A data row has entries (i_a, f_a, x_a), a = 0 .. L-1: feature id, field id, value.
 *   yhat = w0 + sum_a w[i_a] x_a + sum_{a<b} x_a x_b <V[i_a][f_b], V[i_b][f_a]>         V: (n + 1) x F x k
 * Entries that share a field interact like any other pair.  libffm's model is this one with w0 = w = 0 and never stepped
 * (fmhip_ffm_model_set_linear(m, 0)).
 * The residual: squared loss e = yhat - y; logistic loss e = sigma(yhat) - t, t = [y > 0] (fmhip.h's conventions).
 * The gradient of a batch B, for every (i, f) the batch TOUCHES — some row of B holds i at a position a and another entry b != a with
 * f_b = f; that depends on which entries exist, never on their values —
 *   g_V[i][f] = (1/|B|) sum_{rows r, a: i_a = i} sum_{b != a, f_b = f} e_r x_a x_b V[i_b][f_a]
 *   g_w[i]    = (1/|B|) sum e_r x_a  (touched: i is in a row of B)          g_w0 = (1/|B|) sum e_r
 * The update is libffm's lazy regularisation stated for a mini-batch: a touched (i, f) steps on g + regv V[i][f], a touched w[i] on
 * g + regw w[i], w0 on g + reg0 w0; a parameter the batch does not touch keeps every bit.  The step is plain SGD,
 * theta <- theta - eta g_hat, or AdaGrad with the rule, eps and initial accumulator of fmhip_model_set_optimizer (fmhip.h):
 * n <- n + g_hat^2, theta <- theta - eta g_hat / (sqrt(n) + eps); libffm's own rule is init = 1 with a tiny eps.
 * Three launches per step, no atomics, every sum in an order fixed by the data: the same bits on every run.
 *
 * LIMITS, each refused before any launch (the message names the offending value):
 *   1 <= num_fields <= FMHIP_FFM_MAX_FIELDS, 1 <= num_factor <= FMHIP_FFM_MAX_FACTORS (padded to 4, 8 or 16 floats), num_attribute >= 0:
 *       FMHIP_ERR_INVALID below the range, FMHIP_ERR_UNSUPPORTED above it
 *   a data row of more than FMHIP_FFM_MAX_ROW entries: FMHIP_ERR_UNSUPPORTED
 *   a feature id < 0 (at create) or > the model's num_attribute (at the first call that pairs the two), a field id outside
 *   [0, FMHIP_FFM_MAX_FIELDS) (at create) or >= the model's num_fields (at pairing), a feature id twice in one row, a value that
 *   is not finite as fp32, a row_ptr that does not start at 0 or decreases: FMHIP_ERR_INVALID
 * Same library and conventions as fmhip.h (plain C, int status, fmhip_last_error, never throws), which this header includes.  A
 * model handle serialises its calls (one lock); a dataset is read-only once made and may be shared by models on its device.
 *
 * Not here: the data-parallel exchanges (fmhip_dp_*), example weights, pairs / the BPR trainer, relational data, FTRL-Proximal,
 * ALS / MCMC, include/sparkfm.hpp and the JNI shim.
 */
#ifndef FMHIP_FFM_H
#define FMHIP_FFM_H
#include "fmhip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FMHIP_FFM_MAX_FIELDS 64
#define FMHIP_FFM_MAX_FACTORS 16
#define FMHIP_FFM_MAX_ROW 64

typedef struct fmhip_ffm_model *fmhip_ffm_model_t;
typedef struct fmhip_ffm_dataset *fmhip_ffm_dataset_t;

/* ---- model ---- */
/* Parameters start at zero, the rule at squared loss + SGD, the linear terms on.  `stream`: a hipStream_t (NULL: the library
 * creates its own non-blocking stream).  The limits above are checked before the device is looked at. */
int fmhip_ffm_model_create(int device, int64_t num_attribute, int32_t num_fields, int32_t num_factor, void *stream, fmhip_ffm_model_t *out);
int fmhip_ffm_model_destroy(fmhip_ffm_model_t m);
/* padded_factors: floats per (feature, field) vector on the device: 4, 8 or 16.  All out pointers nullable */
int fmhip_ffm_model_info(fmhip_ffm_model_t m, int64_t *num_attribute, int32_t *num_fields, int32_t *num_factor, int32_t *padded_factors);
/* w: n + 1 doubles; v: (n + 1) * F * k doubles at v[((i * F) + f) * k + d]; stored as fp32.  get: every pointer nullable */
int fmhip_ffm_model_set_params(fmhip_ffm_model_t m, double w0, const double *w, const double *v);
int fmhip_ffm_model_get_params(fmhip_ffm_model_t m, double *w0, double *w, double *v);
/* loss: enum fmhip_loss; optimizer: FMHIP_OPT_SGD or FMHIP_OPT_ADAGRAD with eps (finite, > 0) and the accumulators' initial value
 * (finite, >= 0), both ignored under SGD.  AdaGrad on a model that is not already under it with the same settings (bit-equal)
 * allocates the accumulators — one more copy of the model — and fills them with `init`; the same settings again keep them; SGD
 * frees them.  Anything else: FMHIP_ERR_INVALID */
int fmhip_ffm_model_set_rule(fmhip_ffm_model_t m, int loss, int optimizer, double eps, double init);
/* linear = 0: w0 and w are never stepped (they are still read: libffm's model while they hold 0); 1: stepped */
int fmhip_ffm_model_set_linear(fmhip_ffm_model_t m, int linear);
/* AdaGrad's accumulators, laid out like the parameters (checkpoints).  FMHIP_ERR_INVALID unless the model is under AdaGrad;
 * set: every value finite and >= 0 */
int fmhip_ffm_model_get_accumulators(fmhip_ffm_model_t m, double *n0, double *nw, double *nv);
int fmhip_ffm_model_set_accumulators(fmhip_ffm_model_t m, double n0, const double *nw, const double *nv);

/* ---- dataset ---- */
/* CSR rows with a field id per entry.  y may be NULL (predict only: the training calls refuse the dataset).  batch_rows <= 0: one
 * batch.  Every row's entries are sorted by (field, feature) and every batch's transpose built on the host, once; the caller keeps
 * the arrays.  The data's limits (above) are checked before the device is looked at */
int fmhip_ffm_dataset_create(int device, int64_t n_rows, const int64_t *row_ptr, const int32_t *col, const int32_t *field, const double *val,
                             const double *y, int64_t batch_rows, fmhip_ffm_dataset_t *out);
int fmhip_ffm_dataset_destroy(fmhip_ffm_dataset_t d);
/* dimension: the largest feature id; fields: the largest field id + 1; max_row: the longest row.  All out pointers nullable */
int fmhip_ffm_dataset_info(fmhip_ffm_dataset_t d, int64_t *n_rows, int64_t *nnz, int64_t *dimension, int32_t *fields, int32_t *max_row,
                           int64_t *batch_rows, int64_t *n_batches);

/* ---- compute ---- */
/* yhat: n_rows doubles, the margins (under either loss) */
int fmhip_ffm_predict(fmhip_ffm_model_t m, fmhip_ffm_dataset_t d, double *yhat);
/* One step on batch `batch`, asynchronous on the model's stream; a non-NULL stats synchronises: sse and sum_e over the batch's e at
 * the parameters before the step, rows, nnz, nonfinite (rows whose margin was not finite), steps = 1 */
int fmhip_ffm_step(fmhip_ffm_model_t m, fmhip_ffm_dataset_t d, int64_t batch, double eta, double reg0, double regw, double regv, fmhip_stats *stats);
/* One pass over the batches in `order` (NULL: ascending; else n_batches ids, each in range); nothing inside it synchronises with the
 * host.  stats (nullable; synchronises): the sums over the epoch's batches */
int fmhip_ffm_epoch(fmhip_ffm_model_t m, fmhip_ffm_dataset_t d, double eta, double reg0, double regw, double regv, const int64_t *order,
                    fmhip_stats *stats);

#ifdef __cplusplus
}
#endif
#endif /* FMHIP_FFM_H */
