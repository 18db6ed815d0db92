/*
 * fmhip_deepfm.h — DeepFM (libfmhip.so): Guo et al., "DeepFM: A Factorization-Machine based Neural Network for CTR Prediction", IJCAI
 * 2017.  The plain FM term plus a small multi-layer perceptron, both reading the same feature embeddings.  A model and kernels of
 * their own; the data handle is fmhip_ffm.h's fmhip_ffm_dataset_t, unchanged.
 *
 * THE MODEL.  A data row has entries (i_a, f_a, x_a): feature id (at most once per row), field id, value.  z_a = x_a v[i_a] (k
 * floats), T = sum_a z_a, S_f = the sum of z_a over the row's entries of field f (sum-pooled; 0 for a field the row lacks), and s =
 * S_0 .. S_{F-1} side by side.
 *   y_fm   = w0 + sum_a w[i_a] x_a + 1/2 sum_d (T_d^2 - sum_a z_ad^2)        (the plain FM over the row's entries, fields ignored)
 *   h_0    = s;   h_l = relu(h_{l-1} W_l + b_l),  l = 1 .. L                   W_l: n_{l-1} x n_l,  n_0 = F k
 *   y_deep = <h_L, u>                                                          u: n_L (no bias of its own: w0 is the model's)
 *   yhat   = y_fm + y_deep
 * With m_l = [h_l > 0]: delta_L = u o m_L, delta_{l-1} = (delta_l W_l^T) o m_{l-1}, J = delta_1 W_1^T (F k floats, no mask);
 *   d yhat / d v[i_a] = x_a ((T - z_a) + J[f_a]);   dL/dW_l = 1/|B| sum_r e_r h_{l-1,r}^T delta_{l,r};
 *   dL/db_l = 1/|B| sum_r e_r delta_{l,r};   dL/du = 1/|B| sum_r e_r h_{L,r}
 * Residuals, both losses, the 1/|B| mean, SGD / AdaGrad, eps, the accumulators' initial value, the statistics and `linear` are
 * fmhip_fwfm.h's.  The update: v[i] and w[i] step on g + reg theta for every feature present in the batch, every other feature keeps
 * every bit; w0 as in fmhip_fwfm.h; W_l and u are stepped densely every batch on g + regd theta, b_l on g alone, with AdaGrad
 * accumulators of their own.
 * A new model has v = w = w0 = 0 and W_l = b_l = u = 0.  AN ALL-ZERO v HAS AN ALL-ZERO GRADIENT under this model (T, z_a and s are 0,
 * so is every d yhat / d v, and W_1's gradient): draw v before training, as the Python class does from its seed.  With u = 0 and the
 * dense part not trained (fmhip_deepfm_model_set_deep) the model is the plain FM.
 * Five launches per step, no atomics, every sum in an order fixed by the data and by compile-time constants: the same bits on every run.
 *
 * LIMITS, each refused before any launch (the message names the offending value):
 *   1 <= num_fields <= FMHIP_DEEPFM_MAX_FIELDS, 1 <= num_factor <= FMHIP_DEEPFM_MAX_FACTORS (padded to Kp = 4, 8 or 16 floats),
 *   num_fields * Kp <= FMHIP_DEEPFM_MAX_WIDTH, 1 <= n_layers <= FMHIP_DEEPFM_MAX_LAYERS, every width a multiple of 16 with
 *   16 <= n_l <= FMHIP_DEEPFM_MAX_UNITS, num_attribute >= 0: FMHIP_ERR_INVALID below a range or for a width that is no multiple of 16,
 *   FMHIP_ERR_UNSUPPORTED above a range
 *   rows of at most FMHIP_FFM_MAX_ROW entries and the other limits of the data: the dataset's own (fmhip_ffm_dataset_create)
 *   a feature id above the model's num_attribute, a field id >= the model's num_fields: FMHIP_ERR_INVALID at the first call that
 *   pairs the two
 *
 * Not here: dropout and batch-norm, Adam, the data-parallel exchanges (fmhip_dp_*), example weights, pairs / the BPR trainer,
 * relational data, FTRL-Proximal, include/sparkfm.hpp and the JNI shim.
 */
#ifndef FMHIP_DEEPFM_H
#define FMHIP_DEEPFM_H
#include "fmhip_ffm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FMHIP_DEEPFM_MAX_FIELDS 64
#define FMHIP_DEEPFM_MAX_FACTORS 16
#define FMHIP_DEEPFM_MAX_WIDTH 768
#define FMHIP_DEEPFM_MAX_LAYERS 3
#define FMHIP_DEEPFM_MAX_UNITS 256

typedef struct fmhip_deepfm_model *fmhip_deepfm_model_t;

/* ---- model ---- */
/* Every parameter starts at zero, the rule at squared loss + SGD, the linear terms on, the dense part trained.  widths: n_layers
 * ints, n_1 .. n_L.  `stream`: a hipStream_t (NULL: the library creates its own non-blocking stream).  The limits above are checked
 * before the device is looked at. */
int fmhip_deepfm_model_create(int device, int64_t num_attribute, int32_t num_fields, int32_t num_factor, int32_t n_layers, const int32_t *widths,
                              void *stream, fmhip_deepfm_model_t *out);
int fmhip_deepfm_model_destroy(fmhip_deepfm_model_t m);
/* padded_factors: floats per feature vector on the device: 4, 8 or 16; widths: room for FMHIP_DEEPFM_MAX_LAYERS ints.  All out
 * pointers nullable */
int fmhip_deepfm_model_info(fmhip_deepfm_model_t m, int64_t *num_attribute, int32_t *num_fields, int32_t *num_factor, int32_t *padded_factors,
                            int32_t *n_layers, int32_t *widths);
/* w: n + 1 doubles; v: (n + 1) * k doubles at v[i * k + d]; W: n_layers pointers, W[l - 1] the n_{l-1} * n_l doubles of W_l, row-major,
 * n_0 = F * k with row f * k + d for slot d of field f; b: n_layers pointers, b[l - 1] the n_l doubles of b_l; u: n_L doubles; stored
 * as fp32.  get: every pointer (and every pointer inside W and b) nullable */
int fmhip_deepfm_model_set_params(fmhip_deepfm_model_t m, double w0, const double *w, const double *v, const double *const *W, const double *const *b,
                                  const double *u);
int fmhip_deepfm_model_get_params(fmhip_deepfm_model_t m, double *w0, double *w, double *v, double *const *W, double *const *b, double *u);
/* as fmhip_fwfm_model_set_rule; AdaGrad also allocates and fills the dense part's accumulators */
int fmhip_deepfm_model_set_rule(fmhip_deepfm_model_t m, int loss, int optimizer, double eps, double init);
/* linear = 0: w0 and w are read and never stepped; 1: stepped */
int fmhip_deepfm_model_set_linear(fmhip_deepfm_model_t m, int linear);
/* train = 0: W_l, b_l and u are read and never stepped (with u = 0: the plain FM); 1: stepped */
int fmhip_deepfm_model_set_deep(fmhip_deepfm_model_t m, int train);
/* AdaGrad's accumulators, laid out like the parameters.  FMHIP_ERR_INVALID unless the model is under AdaGrad; set: every value finite
 * and >= 0 */
int fmhip_deepfm_model_get_accumulators(fmhip_deepfm_model_t m, double *n0, double *nw, double *nv, double *const *nW, double *const *nb, double *nu);
int fmhip_deepfm_model_set_accumulators(fmhip_deepfm_model_t m, double n0, const double *nw, const double *nv, const double *const *nW,
                                        const double *const *nb, const double *nu);

/* ---- compute ---- */
/* yhat: n_rows doubles, the margins (under either loss) */
int fmhip_deepfm_predict(fmhip_deepfm_model_t m, fmhip_ffm_dataset_t d, double *yhat);
/* One step on batch `batch`, asynchronous on the model's stream; a non-NULL stats synchronises (as fmhip_ffm_step's) */
int fmhip_deepfm_step(fmhip_deepfm_model_t m, fmhip_ffm_dataset_t d, int64_t batch, double eta, double reg0, double regw, double regv, double regd,
                      fmhip_stats *stats);
/* One pass over the batches in `order` (NULL: ascending; else n_batches ids, each in range); nothing inside it synchronises with the
 * host.  stats (nullable; synchronises): the sums over the epoch's batches */
int fmhip_deepfm_epoch(fmhip_deepfm_model_t m, fmhip_ffm_dataset_t d, double eta, double reg0, double regw, double regv, double regd,
                       const int64_t *order, fmhip_stats *stats);

#ifdef __cplusplus
}
#endif
#endif /* FMHIP_DEEPFM_H */
