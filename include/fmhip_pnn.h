/*
 * fmhip_pnn.h — the product-based neural network (libfmhip.so): Qu et al., "Product-based Neural Networks for User Response
 * Prediction", ICDM 2016, the inner-product form.  A multi-layer perceptron whose input is the field embeddings AND their pairwise
 * inner products; the product layer is also the dot interaction of DLRM.  A model and kernels of their own; the data handle is
 * fmhip_ffm.h's fmhip_ffm_dataset_t, unchanged.
 *
 * THE MODEL.  A data row has entries (i_a, f_a, x_a): feature id (at most once per row), field id, value.  z_a = x_a v[i_a] (k
 * floats), S_f = the sum of z_a over the row's entries of field f (sum-pooled; 0 for a field the row lacks), s = S_0 .. S_{F-1} side
 * by side, and g_p = <S_i, S_j> for the G = F (F - 1) / 2 pairs i < j, p(i, j) ascending in i, then in j.
 *   h_0  = [s | g]                                      n_0 = F k + G
 *   h_l  = relu(h_{l-1} W_l + b_l),  l = 1 .. L         W_l: n_{l-1} x n_l
 *   yhat = w0 + sum_a w[i_a] x_a + <h_L, u>             u: n_L (no bias of its own: w0 is the model's)
 * There is no FM pair term beside the network: a first layer that is constant over the pair rows IS that term.
 * With m_l = [h_l > 0], per row: delta_L = u o m_L, delta_{l-1} = (delta_l W_l^T) o m_{l-1}, [Js | dg] = delta_1 W_1^T (no mask),
 *   J[i] = Js[i] + sum_{j != i} dg_{p(min(i, j), max(i, j))} S_j;   d yhat / d v[i_a] = x_a J[f_a];
 *   dL/dW_l = 1/|B| sum_r e_r h_{l-1,r}^T delta_{l,r};   dL/db_l = 1/|B| sum_r e_r delta_{l,r};   dL/du = 1/|B| sum_r e_r h_{L,r}
 * Residuals, both losses, the 1/|B| mean, SGD / AdaGrad, eps, the accumulators' initial value, the statistics and `linear` are
 * fmhip_fwfm.h's.  The update: v[i] and w[i] step on g + reg theta for every feature present in the batch, every other feature keeps
 * every bit; w0 as in fmhip_fwfm.h; W_l and u are stepped densely every batch on g + regd theta, b_l on g alone, with AdaGrad
 * accumulators of their own.
 * With F = 1 there is no pair: G = 0 and the model is an MLP over s.  A new model is all zero: v = w = w0 = 0 and W_l = b_l = u = 0.
 * AN ALL-ZERO v HAS AN ALL-ZERO GRADIENT under this model (s and g are 0, so is every d yhat / d v, and W_1's gradient): draw v and
 * the dense part before training, as the Python class does from its seed (He-uniform with fan-in n_0).
 * Five launches per step (three with the dense part frozen), no atomics, every sum in an order fixed by the data and by compile-time
 * constants: the same bits on every run.
 *
 * LIMITS, each refused before any launch (the message names the offending value):
 *   1 <= num_fields <= FMHIP_PNN_MAX_FIELDS, 1 <= num_factor <= FMHIP_PNN_MAX_FACTORS (padded to Kp = 4, 8 or 16 floats),
 *   round16(num_fields * Kp) + round16(G) <= FMHIP_PNN_MAX_WIDTH (1376 at 39 fields with k = 16, 1392 at 49 fields with Kp = 4: this,
 *   not the field count, is what bounds F), 1 <= n_layers <= FMHIP_PNN_MAX_LAYERS, every width a multiple of 16 with
 *   16 <= n_l <= FMHIP_PNN_MAX_UNITS, num_attribute >= 0: FMHIP_ERR_INVALID below a range or for a width that is no multiple of 16,
 *   FMHIP_ERR_UNSUPPORTED above a range
 *   a device whose LDS per workgroup does not hold the forward's 16-row tile: FMHIP_ERR_UNSUPPORTED at the first call that pairs
 *   model and data (the widest accepted model takes 114 KB to train; gfx950 gives 160 KB)
 *   rows of at most FMHIP_FFM_MAX_ROW entries and the other limits of the data: the dataset's own (fmhip_ffm_dataset_create)
 *   a feature id above the model's num_attribute, a field id >= the model's num_fields: FMHIP_ERR_INVALID at the first call that
 *   pairs the two
 *
 * Not here: the outer-product form, an FM pair term beside the network, dropout and batch-norm, Adam, the data-parallel exchanges
 * (fmhip_dp_*), example weights, pairs / the BPR trainer, relational data, FTRL-Proximal, include/sparkfm.hpp and the JNI shim.
 */
#ifndef FMHIP_PNN_H
#define FMHIP_PNN_H
#include "fmhip_ffm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FMHIP_PNN_MAX_FIELDS 64
#define FMHIP_PNN_MAX_FACTORS 16
#define FMHIP_PNN_MAX_LAYERS 3
#define FMHIP_PNN_MAX_UNITS 256
#define FMHIP_PNN_MAX_WIDTH 1408

typedef struct fmhip_pnn_model *fmhip_pnn_model_t;

/* ---- model ---- */
/* Every parameter starts at zero, the rule at squared loss + SGD, the linear terms on, the dense part trained.  widths: n_layers
 * ints, n_1 .. n_L.  `stream`: a hipStream_t (NULL: the library creates its own non-blocking stream).  The limits above are checked
 * before the device is looked at. */
int fmhip_pnn_model_create(int device, int64_t num_attribute, int32_t num_fields, int32_t num_factor, int32_t n_layers, const int32_t *widths,
                           void *stream, fmhip_pnn_model_t *out);
int fmhip_pnn_model_destroy(fmhip_pnn_model_t m);
/* padded_factors: floats per feature vector on the device: 4, 8 or 16; widths: room for FMHIP_PNN_MAX_LAYERS ints.  All out pointers
 * nullable */
int fmhip_pnn_model_info(fmhip_pnn_model_t m, int64_t *num_attribute, int32_t *num_fields, int32_t *num_factor, int32_t *padded_factors,
                         int32_t *n_layers, int32_t *widths);
/* w: n + 1 doubles; v: (n + 1) * k doubles at v[i * k + d]; W: n_layers pointers, W[l - 1] the n_{l-1} * n_l doubles of W_l, row-major;
 * W[0] is n_0 * n_1 doubles with n_0 = F * k + G: row f * k + d belongs to slot d of field f, row F * k + p(i, j) to the pair (i, j);
 * b: n_layers pointers, b[l - 1] the n_l doubles of b_l; u: n_L doubles; stored as fp32.  get: every pointer (and every pointer inside
 * W and b) nullable */
int fmhip_pnn_model_set_params(fmhip_pnn_model_t m, double w0, const double *w, const double *v, const double *const *W, const double *const *b,
                               const double *u);
int fmhip_pnn_model_get_params(fmhip_pnn_model_t m, double *w0, double *w, double *v, double *const *W, double *const *b, double *u);
/* as fmhip_fwfm_model_set_rule; AdaGrad also allocates and fills the dense part's accumulators */
int fmhip_pnn_model_set_rule(fmhip_pnn_model_t m, int loss, int optimizer, double eps, double init);
/* linear = 0: w0 and w are read and never stepped; 1: stepped */
int fmhip_pnn_model_set_linear(fmhip_pnn_model_t m, int linear);
/* train = 0: W_l, b_l and u are read and never stepped; 1: stepped */
int fmhip_pnn_model_set_deep(fmhip_pnn_model_t m, int train);
/* AdaGrad's accumulators, laid out like the parameters.  FMHIP_ERR_INVALID unless the model is under AdaGrad; set: every value finite
 * and >= 0 */
int fmhip_pnn_model_get_accumulators(fmhip_pnn_model_t m, double *n0, double *nw, double *nv, double *const *nW, double *const *nb, double *nu);
int fmhip_pnn_model_set_accumulators(fmhip_pnn_model_t m, double n0, const double *nw, const double *nv, const double *const *nW,
                                     const double *const *nb, const double *nu);

/* ---- compute ---- */
/* yhat: n_rows doubles, the margins (under either loss) */
int fmhip_pnn_predict(fmhip_pnn_model_t m, fmhip_ffm_dataset_t d, double *yhat);
/* One step on batch `batch`, asynchronous on the model's stream; a non-NULL stats synchronises (as fmhip_ffm_step's) */
int fmhip_pnn_step(fmhip_pnn_model_t m, fmhip_ffm_dataset_t d, int64_t batch, double eta, double reg0, double regw, double regv, double regd,
                   fmhip_stats *stats);
/* One pass over the batches in `order` (NULL: ascending; else n_batches ids, each in range); nothing inside it synchronises with the
 * host.  stats (nullable; synchronises): the sums over the epoch's batches */
int fmhip_pnn_epoch(fmhip_pnn_model_t m, fmhip_ffm_dataset_t d, double eta, double reg0, double regw, double regv, double regd,
                    const int64_t *order, fmhip_stats *stats);

#ifdef __cplusplus
}
#endif
#endif /* FMHIP_PNN_H */
