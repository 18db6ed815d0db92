/*
 * fmhip_afm.h — the Attentional Factorization Machine (libfmhip.so): Xiao et al., "Attentional Factorization Machines: Learning the
 * Weight of Feature Interactions via Attention Networks", IJCAI 2017.  Every pair of fields interacts through the element-by-element
 * product of their sums; a one-hidden-layer net scores each product PER ROW, a softmax over the pairs turns the scores into weights,
 * and the weighted sum of the products is projected to the margin.  A model and kernels of their own; the data handle is fmhip_ffm.h's
 * fmhip_ffm_dataset_t, unchanged.
 *
 * THE MODEL.  A data row has entries (i_a, f_a, x_a): feature id (at most once per row), field id, value.  z_a = x_a v[i_a] (k
 * floats), S_f = the sum of z_a over the row's entries of field f (sum-pooled; 0 for a field the row lacks, which takes part).  The
 * pairs are (i, j) with i < j < F, P = F (F - 1) / 2 of them:
 *   E_ij  = S_i o S_j                                (k floats)
 *   H_ij  = relu(W E_ij + b)                         W: t x k, b: t   (t = the attention factor)
 *   s_ij  = <h, H_ij>                                h: t
 *   a     = softmax of s over the P pairs            (the maximum subtracted)
 *   o     = sum_ij a_ij E_ij                         (k floats)
 *   yhat  = w0 + sum_a w[i_a] x_a + <p, o>           p: k
 * With F = 1 there are no pairs: the AFM term is 0 and the gradients of W, b, h, p are 0.
 * Per row, d yhat / d . with c_ij = <p, E_ij> and T = sum a_ij c_ij (the dense gradients are multiplied by the residual e_r and
 * averaged over the batch; the backward launch multiplies d yhat / d v by e_r itself):
 *   ds_ij = a_ij (c_ij - T);   dh += ds_ij H_ij;   dH_ij = ds_ij h o 1[W E_ij + b > 0];   db += dH_ij;   dW += dH_ij E_ij^T;   dp += o
 *   dE_ij = a_ij p + W^T dH_ij;   J[i] += dE_ij o S_j;   J[j] += dE_ij o S_i;   d yhat / d v[i_a] = x_a J[f_a]
 * Residuals, both losses, the 1/|B| mean, SGD / AdaGrad, eps, the accumulators' initial value, the statistics and `linear` are
 * fmhip_fwfm.h's.  The update: v[i] and w[i] step on g + reg theta for every feature present in the batch, every other feature keeps
 * every bit; w0 as in fmhip_fwfm.h; every element of W, b, h and p is stepped every batch on g + regd theta, with AdaGrad
 * accumulators of its own.
 * A new model has v = w = w0 = 0 and W = b = h = p = 0.  AN ALL-ZERO v HAS AN ALL-ZERO GRADIENT under this model (every E is 0, and
 * so is J): draw v before training, as the Python class does from its seed.  With p = 0 and the attention part not trained
 * (fmhip_afm_model_set_attention) the model is the linear model w0 + <w, x>.
 * Four launches per step, no atomics, every sum in an order fixed by the data and by compile-time constants: the same bits on every
 * run.
 *
 * LIMITS, each refused before any launch (the message names the offending value):
 *   1 <= num_fields <= FMHIP_AFM_MAX_FIELDS, 1 <= num_factor <= FMHIP_AFM_MAX_FACTORS, attention_factor a multiple of 16 with
 *   16 <= attention_factor <= FMHIP_AFM_MAX_ATTENTION, num_attribute >= 0: FMHIP_ERR_INVALID below a range or for an attention factor
 *   that is no multiple of 16, FMHIP_ERR_UNSUPPORTED above a range
 *   a forward workgroup keeps the field sums, their gradient and one score per pair of four rows in LDS (csrc/fm_afm.h:
 *   afm_forward_lds): 64 fields at 16 factors take 80,896 bytes when training, which gfx950's 160 KB hold; a device that gives a
 *   workgroup less refuses the pairing with FMHIP_ERR_UNSUPPORTED
 *   rows of at most FMHIP_FFM_MAX_ROW entries and the other limits of the data: the dataset's own (fmhip_ffm_dataset_create)
 *   a feature id above the model's num_attribute, a field id >= the model's num_fields: FMHIP_ERR_INVALID at the first call that
 *   pairs the two
 * WORKSPACE of training, allocated at the first step for the dataset's largest batch of R rows (an allocation failure is
 * FMHIP_ERR_NOMEM): 4 ceil(R / 128) (t Kp + 2 t + Kp) bytes beside the FwFM's, Kp the padded factors.
 *
 * Not here: dropout on the attention output, restricting the pairs to the fields a row holds, the plain FM pair term beside the
 * attention, Adam; and, as fmhip_deepfm.h, batch-norm, the data-parallel exchanges (fmhip_dp_*), example weights, pairs / the BPR
 * trainer, relational data, FTRL-Proximal, include/sparkfm.hpp and the JNI shim.
 */
#ifndef FMHIP_AFM_H
#define FMHIP_AFM_H
#include "fmhip_ffm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FMHIP_AFM_MAX_FIELDS 64
#define FMHIP_AFM_MAX_FACTORS 16
#define FMHIP_AFM_MAX_ATTENTION 64

typedef struct fmhip_afm_model *fmhip_afm_model_t;

/* ---- model ---- */
/* Every parameter starts at zero, the rule at squared loss + SGD, the linear terms on, the attention part trained.  `stream`: a
 * hipStream_t (NULL: the library creates its own non-blocking stream).  The limits above are checked before the device is looked at. */
int fmhip_afm_model_create(int device, int64_t num_attribute, int32_t num_fields, int32_t num_factor, int32_t attention_factor, void *stream,
                           fmhip_afm_model_t *out);
int fmhip_afm_model_destroy(fmhip_afm_model_t m);
/* padded_factors: floats per feature vector on the device: 4, 8 or 16.  All out pointers nullable */
int fmhip_afm_model_info(fmhip_afm_model_t m, int64_t *num_attribute, int32_t *num_fields, int32_t *num_factor, int32_t *padded_factors,
                         int32_t *attention_factor);
/* w: n + 1 doubles; v: (n + 1) * k doubles at v[i * k + d]; W: t * k doubles at n * k + d; b, h: t doubles; p: k doubles; stored as
 * fp32.  get: every pointer nullable */
int fmhip_afm_model_set_params(fmhip_afm_model_t m, double w0, const double *w, const double *v, const double *W, const double *b, const double *h,
                               const double *p);
int fmhip_afm_model_get_params(fmhip_afm_model_t m, double *w0, double *w, double *v, double *W, double *b, double *h, double *p);
/* as fmhip_fwfm_model_set_rule; AdaGrad also allocates and fills the attention part's accumulators */
int fmhip_afm_model_set_rule(fmhip_afm_model_t m, int loss, int optimizer, double eps, double init);
/* linear = 0: w0 and w are read and never stepped; 1: stepped */
int fmhip_afm_model_set_linear(fmhip_afm_model_t m, int linear);
/* train = 0: W, b, h and p are read and never stepped; 1: stepped */
int fmhip_afm_model_set_attention(fmhip_afm_model_t m, int train);
/* AdaGrad's accumulators, laid out like the parameters.  FMHIP_ERR_INVALID unless the model is under AdaGrad; set: every value finite
 * and >= 0 */
int fmhip_afm_model_get_accumulators(fmhip_afm_model_t m, double *n0, double *nw, double *nv, double *nW, double *nb, double *nh, double *np);
int fmhip_afm_model_set_accumulators(fmhip_afm_model_t m, double n0, const double *nw, const double *nv, const double *nW, const double *nb,
                                     const double *nh, const double *np);

/* ---- compute ---- */
/* yhat: n_rows doubles, the margins (under either loss) */
int fmhip_afm_predict(fmhip_afm_model_t m, fmhip_ffm_dataset_t d, double *yhat);
/* One step on batch `batch`, asynchronous on the model's stream; a non-NULL stats synchronises (as fmhip_ffm_step's) */
int fmhip_afm_step(fmhip_afm_model_t m, fmhip_ffm_dataset_t d, int64_t batch, double eta, double reg0, double regw, double regv, double regd,
                   fmhip_stats *stats);
/* One pass over the batches in `order` (NULL: ascending; else n_batches ids, each in range); nothing inside it synchronises with the
 * host.  stats (nullable; synchronises): the sums over the epoch's batches */
int fmhip_afm_epoch(fmhip_afm_model_t m, fmhip_ffm_dataset_t d, double eta, double reg0, double regw, double regv, double regd, const int64_t *order,
                    fmhip_stats *stats);

#ifdef __cplusplus
}
#endif
#endif /* FMHIP_AFM_H */
