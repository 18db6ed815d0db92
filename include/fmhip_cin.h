/*
 * fmhip_cin.h — xDeepFM's Compressed Interaction Network (libfmhip.so): Lian et al., "xDeepFM: Combining Explicit and Implicit Feature
 * Interactions for Recommender Systems", KDD 2018.  Explicit feature crosses of bounded degree L + 1 over the rows' field sums, formed
 * VECTOR-WISE: a feature map is a weighted sum of element-by-element products of whole k-vectors, one weight per pair of vectors.
 * A model and kernels of their own; the data handle is fmhip_ffm.h's fmhip_ffm_dataset_t, unchanged.
 *
 * THE MODEL.  A data row has entries (i_a, f_a, x_a): feature id (at most once per row), field id, value.  z_a = x_a v[i_a] (k
 * floats), S_f = the sum of z_a over the row's entries of field f (sum-pooled; 0 for a field the row lacks, which takes part).
 *   X^0     = S_0 .. S_{F-1}                                              H_0 = F rows of k
 *   X^l[h, d] = sum_{i < H_{l-1}} sum_{j < F} W_l[h, i, j] X^{l-1}[i, d] X^0[j, d]          l = 1 .. L,   W_l: H_l x H_{l-1} x F
 *   p^l[h]  = sum_d X^l[h, d]
 *   yhat    = w0 + sum_a w[i_a] x_a + < [p^1 .. p^L], u >                 u: H_1 + .. + H_L
 * The activation is the identity (the paper's best form); there are no biases and no FM pair term.  With L = 1 the CIN term is
 * sum_{i,j} (sum_h u_h W_1[h, i, j]) <S_i, S_j>: the field-weighted FM's form on pooled field sums.
 * Per row, d yhat / d . (the backward launch multiplies by the residual e_r itself):
 *   G^L[h, d] = u^L[h];   for l = L .. 1:   dZ[i, j, d] = sum_h G^l[h, d] W_l[h, i, j],
 *   G^{l-1}[i, d] = sum_j dZ[i, j, d] X^0[j, d] (+ u^{l-1}[i] for l - 1 >= 1),   J[j, d] += sum_i dZ[i, j, d] X^{l-1}[i, d]
 *   J += G^0;   d yhat / d v[i_a] = x_a J[f_a]
 *   dL/dW_l[h, i, j] = 1/|B| sum_r e_r sum_d G^l[h, d] X^{l-1}[i, d] X^0[j, d];   dL/du^l = 1/|B| sum_r e_r p^l
 * Residuals, both losses, the 1/|B| mean, SGD / AdaGrad, eps, the accumulators' initial value, the statistics and `linear` are
 * fmhip_fwfm.h's.  The update: v[i] and w[i] step on g + reg theta for every feature present in the batch, every other feature keeps
 * every bit; w0 as in fmhip_fwfm.h; W_l and u are stepped densely every batch on g + regd theta, with AdaGrad accumulators of their
 * own.
 * A new model has v = w = w0 = 0 and W_l = u = 0.  AN ALL-ZERO v HAS AN ALL-ZERO GRADIENT under this model (X^0 is 0, so is every
 * X^l and J): draw v before training, as the Python class does from its seed.  With u = 0 and the CIN part not trained
 * (fmhip_cin_model_set_cin) the model is the linear model w0 + <w, x>.
 * Five launches per step, no atomics, every sum in an order fixed by the data and by compile-time constants: the same bits on every run.
 *
 * LIMITS, each refused before any launch (the message names the offending value):
 *   1 <= num_fields <= FMHIP_CIN_MAX_FIELDS, 1 <= num_factor <= FMHIP_CIN_MAX_FACTORS, 1 <= n_layers <= FMHIP_CIN_MAX_LAYERS,
 *   every feature_maps[l] a multiple of 16 with 16 <= feature_maps[l] <= FMHIP_CIN_MAX_MAPS, num_attribute >= 0: FMHIP_ERR_INVALID
 *   below a range or for a map count that is no multiple of 16, FMHIP_ERR_UNSUPPORTED above a range
 *   the forward keeps X^0 .. X^L of a tile of rows in LDS (csrc/fm_cin.h: cin_forward_lds): the widest model (64 fields, 16 factors,
 *   three layers of 128 maps) takes 74,512 bytes for a training tile of one row, which gfx950's 160 KB hold; a device that gives a
 *   workgroup less than a model's one-row tile refuses the pairing with FMHIP_ERR_UNSUPPORTED
 *   rows of at most FMHIP_FFM_MAX_ROW entries and the other limits of the data: the dataset's own (fmhip_ffm_dataset_create)
 *   a feature id above the model's num_attribute, a field id >= the model's num_fields: FMHIP_ERR_INVALID at the first call that
 *   pairs the two
 * WORKSPACE of training, allocated at the first step for the dataset's largest batch of R rows (an allocation failure is
 * FMHIP_ERR_NOMEM), with Fp = F rounded up to 16 and T the floats of the W_l and u on the device:
 * 4 (R (k (Fp + 2 sum_l H_l - H_L) + sum_l H_l) + ceil(R / 512) T) bytes beside the FwFM's, when the CIN part is trained.
 *
 * Not here: the DNN beside the CIN (fmhip_deepfm.h is that part), the split-half connection, an activation on the feature maps;
 * dropout and batch-norm, Adam, the data-parallel exchanges (fmhip_dp_*), example weights, pairs / the BPR trainer, relational data,
 * FTRL-Proximal, include/sparkfm.hpp and the JNI shim.
 */
#ifndef FMHIP_CIN_H
#define FMHIP_CIN_H
#include "fmhip_ffm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FMHIP_CIN_MAX_FIELDS 64
#define FMHIP_CIN_MAX_FACTORS 16
#define FMHIP_CIN_MAX_LAYERS 3
#define FMHIP_CIN_MAX_MAPS 128

typedef struct fmhip_cin_model *fmhip_cin_model_t;

/* ---- model ---- */
/* Every parameter starts at zero, the rule at squared loss + SGD, the linear terms on, the CIN part trained.  feature_maps: n_layers
 * values, H_1 .. H_L.  `stream`: a hipStream_t (NULL: the library creates its own non-blocking stream).  The limits above are checked
 * before the device is looked at. */
int fmhip_cin_model_create(int device, int64_t num_attribute, int32_t num_fields, int32_t num_factor, int32_t n_layers, const int32_t *feature_maps,
                           void *stream, fmhip_cin_model_t *out);
int fmhip_cin_model_destroy(fmhip_cin_model_t m);
/* padded_factors: floats per feature vector on the device: 4, 8 or 16; feature_maps: n_layers values.  All out pointers nullable */
int fmhip_cin_model_info(fmhip_cin_model_t m, int64_t *num_attribute, int32_t *num_fields, int32_t *num_factor, int32_t *padded_factors, int32_t *n_layers,
                         int32_t *feature_maps);
/* w: n + 1 doubles; v: (n + 1) * k doubles at v[i * k + d]; W: n_layers pointers, W[l - 1] the H_l * H_{l-1} * F doubles of W_l at
 * (h * H_{l-1} + i) * F + j, H_0 = F; u: H_1 + .. + H_L doubles, u^1 first; stored as fp32.  get: every pointer (and every pointer
 * inside W) nullable */
int fmhip_cin_model_set_params(fmhip_cin_model_t m, double w0, const double *w, const double *v, const double *const *W, const double *u);
int fmhip_cin_model_get_params(fmhip_cin_model_t m, double *w0, double *w, double *v, double *const *W, double *u);
/* as fmhip_fwfm_model_set_rule; AdaGrad also allocates and fills the CIN part's accumulators */
int fmhip_cin_model_set_rule(fmhip_cin_model_t m, int loss, int optimizer, double eps, double init);
/* linear = 0: w0 and w are read and never stepped; 1: stepped */
int fmhip_cin_model_set_linear(fmhip_cin_model_t m, int linear);
/* train = 0: W_l and u are read and never stepped; 1: stepped */
int fmhip_cin_model_set_cin(fmhip_cin_model_t m, int train);
/* AdaGrad's accumulators, laid out like the parameters.  FMHIP_ERR_INVALID unless the model is under AdaGrad; set: every value finite
 * and >= 0 */
int fmhip_cin_model_get_accumulators(fmhip_cin_model_t m, double *n0, double *nw, double *nv, double *const *nW, double *nu);
int fmhip_cin_model_set_accumulators(fmhip_cin_model_t m, double n0, const double *nw, const double *nv, const double *const *nW, const double *nu);

/* ---- compute ---- */
/* yhat: n_rows doubles, the margins (under either loss) */
int fmhip_cin_predict(fmhip_cin_model_t m, fmhip_ffm_dataset_t d, double *yhat);
/* One step on batch `batch`, asynchronous on the model's stream; a non-NULL stats synchronises (as fmhip_ffm_step's) */
int fmhip_cin_step(fmhip_cin_model_t m, fmhip_ffm_dataset_t d, int64_t batch, double eta, double reg0, double regw, double regv, double regd,
                   fmhip_stats *stats);
/* One pass over the batches in `order` (NULL: ascending; else n_batches ids, each in range); nothing inside it synchronises with the
 * host.  stats (nullable; synchronises): the sums over the epoch's batches */
int fmhip_cin_epoch(fmhip_cin_model_t m, fmhip_ffm_dataset_t d, double eta, double reg0, double regw, double regv, double regd, const int64_t *order,
                    fmhip_stats *stats);

#ifdef __cplusplus
}
#endif
#endif /* FMHIP_CIN_H */
