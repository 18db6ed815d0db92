/*
 * fmhip_autoint.h — AutoInt (libfmhip.so): Song et al., "AutoInt: Automatic Feature Interaction Learning via Self-Attentive Neural
 * Networks", CIKM 2019.  Multi-head self-attention over the rows' field sums: each field attends to the other fields of its own row,
 * so the weights that mix the fields are computed per row.  A model and kernels of their own; the data handle is fmhip_ffm.h's
 * fmhip_ffm_dataset_t, unchanged.
 *
 * THE MODEL.  A data row has entries (i_a, f_a, x_a): feature id (at most once per row), field id, value.  Its tokens are the field
 * sums X_0[f] = S_f = the sum of x_a v[i_a] over the row's entries of field f: an F x k matrix.  A field the row lacks is the zero
 * token, and it still takes part in the softmax.  Layer l = 0 .. L-1 has H heads of width d, A = H d:
 *   [Q | K | V | R] = X_l W_l                  W_l: D_l x 4A, D_0 = k, D_l = A for l >= 1; head h owns the columns h d .. h d + d - 1
 *                                              of each of the four blocks
 *   P^h     = softmax over g of (Q^h_f . K^h_g)          F x F per head, unscaled (the paper's form)
 *   O^h     = P^h V^h
 *   X_{l+1} = relu([O^0 .. O^{H-1}] + R)                 F x A
 *   yhat    = w0 + sum_a w[i_a] x_a + <vec(X_L), u>      u: F A, element f A + j
 * There is no FM pair term and there are no biases.
 * Per row, d yhat / d . (the backward launch multiplies v's side by the residual e_r itself; the dense gradients are weighted by e_r in
 * the forward launch), with G = d yhat / d X_{l+1} and Z the pre-activation:
 *   Gz = G o [Z > 0];   dV^h = P^h^T Gz^h;   dP^h = Gz^h V^h^T;   dSc^h = P^h o (dP^h - rowsum(dP^h o P^h))
 *   dQ^h = dSc^h K^h;   dK^h = dSc^h^T Q^h;   dW_l = X_l^T [dQ | dK | dV | Gz];   d yhat / d X_l = [dQ | dK | dV | Gz] W_l^T
 *   du = vec(X_L);   J = d yhat / d X_0;   d yhat / d v[i_a] = x_a J[f_a]
 * Residuals, both losses, the 1/|B| mean, SGD / AdaGrad, eps, the accumulators' initial value, the statistics and `linear` are
 * fmhip_fwfm.h's.  The update: v[i] and w[i] step on g + reg theta for every feature present in the batch, every other feature keeps
 * every bit; w0 as in fmhip_fwfm.h; W_l and u are stepped densely every batch on g + regd theta, with AdaGrad accumulators of their own.
 * On the device a feature vector is padded to Kp = 4, 8 or 16 floats and W_0 to 16 rows; the rows of W_0 at pad slots are 0 and stay 0:
 * X_0 is 0 there, and with it their gradient.
 * A new model has v = w = w0 = 0 and W_l = u = 0.  AN ALL-ZERO v HAS AN ALL-ZERO GRADIENT under this model: draw v before training, as
 * the Python class does from its seed.  With u = 0 and the attention part not trained (fmhip_autoint_model_set_attention) the model is
 * the linear model w0 + <w, x>.
 * Four launches per step, no atomics, every sum in an order fixed by the data and by compile-time constants: the same bits on every
 * run.  The softmax subtracts the row maximum; its exp is within 1 ulp.
 *
 * LIMITS, each refused before any launch (the message names the offending value):
 *   1 <= num_fields <= FMHIP_AUTOINT_MAX_FIELDS, 1 <= num_factor <= FMHIP_AUTOINT_MAX_FACTORS (padded to Kp = 4, 8 or 16 floats),
 *   1 <= n_layers <= FMHIP_AUTOINT_MAX_LAYERS, heads 1, 2 or 4, head_dim 16 or 32, heads * head_dim <= FMHIP_AUTOINT_MAX_WIDTH,
 *   num_attribute >= 0: FMHIP_ERR_INVALID below a range or for a value off the grid, FMHIP_ERR_UNSUPPORTED above a range
 *   the forward keeps one row's X_0 .. X_L, [Q | K | V | R] and two F x F tiles in LDS, with Fp = num_fields rounded up to 16:
 *   4 (Fp (20 + L (A + 4) + 4A + 4 + 2 (Fp + 4)) + 16) bytes: 158,784 at the largest model (64 fields, A = 64, 3 layers), which gfx950's
 *   160 KB hold; a device that gives a workgroup less refuses the model's creation with FMHIP_ERR_UNSUPPORTED
 *   rows of at most FMHIP_FFM_MAX_ROW entries and the other limits of the data: the dataset's own (fmhip_ffm_dataset_create)
 *   a feature id above the model's num_attribute, a field id >= the model's num_fields: FMHIP_ERR_INVALID at the first call that
 *   pairs the two
 * WORKSPACE of training, allocated at the first step (an allocation failure is FMHIP_ERR_NOMEM): beside the FwFM's yhat, e and dz
 * nothing grows with the batch's rows but two arrays with a slot per forward workgroup, G = ceil(R / 128) for the largest batch of R
 * rows: 4 G ((L - 1) Fp 3A + L-layer parameter count) bytes.
 *
 * Not here: the 1/sqrt(d) scale, an MLP beside the attention (the paper's "AutoInt+"), dropout and layer-norm, returning the attention
 * maps, Adam, batch-norm, the data-parallel exchanges (fmhip_dp_*), example weights, pairs / the BPR trainer, relational data,
 * FTRL-Proximal, include/sparkfm.hpp and the JNI shim.
 */
#ifndef FMHIP_AUTOINT_H
#define FMHIP_AUTOINT_H
#include "fmhip_ffm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FMHIP_AUTOINT_MAX_FIELDS 64
#define FMHIP_AUTOINT_MAX_FACTORS 16
#define FMHIP_AUTOINT_MAX_LAYERS 3
#define FMHIP_AUTOINT_MAX_HEADS 4
#define FMHIP_AUTOINT_MAX_HEAD_DIM 32
#define FMHIP_AUTOINT_MAX_WIDTH 64

typedef struct fmhip_autoint_model *fmhip_autoint_model_t;

/* ---- model ---- */
/* Every parameter starts at zero, the rule at squared loss + SGD, the linear terms on, the attention part trained.  `stream`: a
 * hipStream_t (NULL: the library creates its own non-blocking stream).  The limits above are checked before the device is looked at. */
int fmhip_autoint_model_create(int device, int64_t num_attribute, int32_t num_fields, int32_t num_factor, int32_t n_layers, int32_t heads, int32_t head_dim,
                               void *stream, fmhip_autoint_model_t *out);
int fmhip_autoint_model_destroy(fmhip_autoint_model_t m);
/* padded_factors: floats per feature vector on the device: 4, 8 or 16.  All out pointers nullable */
int fmhip_autoint_model_info(fmhip_autoint_model_t m, int64_t *num_attribute, int32_t *num_fields, int32_t *num_factor, int32_t *padded_factors,
                             int32_t *n_layers, int32_t *heads, int32_t *head_dim);
/* w: n + 1 doubles; v: (n + 1) * k doubles at v[i * k + d]; W: n_layers pointers, W[l] the D_l * 4A doubles of W_l, row-major
 * (D_0 = k, D_l = A); u: F * A doubles; stored as fp32.  get: every pointer (and every pointer inside W) nullable */
int fmhip_autoint_model_set_params(fmhip_autoint_model_t m, double w0, const double *w, const double *v, const double *const *W, const double *u);
int fmhip_autoint_model_get_params(fmhip_autoint_model_t m, double *w0, double *w, double *v, double *const *W, double *u);
/* as fmhip_fwfm_model_set_rule; AdaGrad also allocates and fills the dense part's accumulators */
int fmhip_autoint_model_set_rule(fmhip_autoint_model_t m, int loss, int optimizer, double eps, double init);
/* linear = 0: w0 and w are read and never stepped; 1: stepped */
int fmhip_autoint_model_set_linear(fmhip_autoint_model_t m, int linear);
/* train = 0: W_l and u are read and never stepped; 1: stepped */
int fmhip_autoint_model_set_attention(fmhip_autoint_model_t m, int train);
/* AdaGrad's accumulators, laid out like the parameters.  FMHIP_ERR_INVALID unless the model is under AdaGrad; set: every value finite
 * and >= 0 */
int fmhip_autoint_model_get_accumulators(fmhip_autoint_model_t m, double *n0, double *nw, double *nv, double *const *nW, double *nu);
int fmhip_autoint_model_set_accumulators(fmhip_autoint_model_t m, double n0, const double *nw, const double *nv, const double *const *nW, const double *nu);

/* ---- compute ---- */
/* yhat: n_rows doubles, the margins (under either loss) */
int fmhip_autoint_predict(fmhip_autoint_model_t m, fmhip_ffm_dataset_t d, double *yhat);
/* One step on batch `batch`, asynchronous on the model's stream; a non-NULL stats synchronises (as fmhip_ffm_step's) */
int fmhip_autoint_step(fmhip_autoint_model_t m, fmhip_ffm_dataset_t d, int64_t batch, double eta, double reg0, double regw, double regv, double regd,
                       fmhip_stats *stats);
/* One pass over the batches in `order` (NULL: ascending; else n_batches ids, each in range); nothing inside it synchronises with the
 * host.  stats (nullable; synchronises): the sums over the epoch's batches */
int fmhip_autoint_epoch(fmhip_autoint_model_t m, fmhip_ffm_dataset_t d, double eta, double reg0, double regw, double regv, double regd, const int64_t *order,
                        fmhip_stats *stats);

#ifdef __cplusplus
}
#endif
#endif /* FMHIP_AUTOINT_H */
