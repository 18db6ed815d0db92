/*
 * fmhip_dcn.h — DCN-V2's low-rank cross network (libfmhip.so): Wang et al., "DCN V2: Improved Deep & Cross Network and Practical
 * Lessons for Web-scale Learning to Rank Systems", WWW 2021.  Explicit feature crosses of bounded degree L + 1 over the rows'
 * concatenated field sums, each cross layer's P x P matrix in the paper's low-rank form C_l = V_l U_l.  A model and kernels of their
 * own; the data handle is fmhip_ffm.h's fmhip_ffm_dataset_t, unchanged.
 *
 * THE MODEL.  A data row has entries (i_a, f_a, x_a): feature id (at most once per row), field id, value.  z_a = x_a v[i_a] (k
 * floats), S_f = the sum of z_a over the row's entries of field f (sum-pooled; 0 for a field the row lacks), and s = S_0 .. S_{F-1}
 * side by side, P = F k floats.
 *   x_0     = s
 *   t_l     = x_l V_l                          V_l: P x r
 *   p_l     = t_l U_l + c_l                    U_l: r x P,  c_l: P
 *   x_{l+1} = x_0 o p_l + x_l                  l = 0 .. L-1   (o: element by element)
 *   yhat    = w0 + sum_a w[i_a] x_a + <x_L, u>                u: P
 * There is no FM pair term: with L = 1, c_0 = -1 and u = 1 the cross term is s^T (V_0 U_0) s, the field-matrixed FM's form.
 * Per row, d yhat / d . (the backward launch multiplies by the residual e_r itself):
 *   g_L = u;   for l = L-1 .. 0:   q_l = g_{l+1} o x_0,   m_l = q_l U_l^T (r floats),   g_l = m_l V_l^T + g_{l+1}
 *   J = g_0 + sum_l g_{l+1} o p_l;   d yhat / d v[i_a] = x_a J[f_a]
 *   dL/dU_l = 1/|B| sum_r e_r t_{l,r}^T q_{l,r};   dL/dV_l = 1/|B| sum_r e_r x_{l,r}^T m_{l,r};
 *   dL/dc_l = 1/|B| sum_r e_r q_{l,r};   dL/du = 1/|B| sum_r e_r x_{L,r}
 * Residuals, both losses, the 1/|B| mean, SGD / AdaGrad, eps, the accumulators' initial value, the statistics and `linear` are
 * fmhip_fwfm.h's.  The update: v[i] and w[i] step on g + reg theta for every feature present in the batch, every other feature keeps
 * every bit; w0 as in fmhip_fwfm.h; V_l, U_l and u are stepped densely every batch on g + regd theta, c_l on g alone, with AdaGrad
 * accumulators of their own.
 * On the device a feature vector is padded to Kp = 4, 8 or 16 floats and s to Pp = F Kp rounded up to 16.  The rows of V_l, the
 * columns of U_l and the elements of c_l and u that belong to pad slots are 0 and stay 0: x_0 is 0 there, so every x_l and q_l is,
 * and with them every one of those gradients.
 * A new model has v = w = w0 = 0 and V_l = U_l = c_l = u = 0.  AN ALL-ZERO v HAS AN ALL-ZERO GRADIENT under this model (s is 0, so is
 * every x_l and q_l): draw v before training, as the Python class does from its seed.  With u = 0 and the cross part not trained
 * (fmhip_dcn_model_set_cross) the model is the linear model w0 + <w, x>.
 * Five launches per step, no atomics, every sum in an order fixed by the data and by compile-time constants: the same bits on every run.
 *
 * LIMITS, each refused before any launch (the message names the offending value):
 *   1 <= num_fields <= FMHIP_DCN_MAX_FIELDS, 1 <= num_factor <= FMHIP_DCN_MAX_FACTORS (padded to Kp = 4, 8 or 16 floats),
 *   num_fields * Kp <= FMHIP_DCN_MAX_WIDTH, 1 <= n_layers <= FMHIP_DCN_MAX_LAYERS, rank a multiple of 16 with
 *   16 <= rank <= FMHIP_DCN_MAX_RANK, num_attribute >= 0: FMHIP_ERR_INVALID below a range or for a rank that is no multiple of 16,
 *   FMHIP_ERR_UNSUPPORTED above a range
 *   the forward keeps x_0, x_l and t_l of at least 16 rows in LDS: 4 (16 (2 (Pp + 4) + rank + 6) + 17) bytes rounded up to 16, plus
 *   384: 116,048 at the widest model (768, rank 256), which gfx950's 160 KB hold, so the width limit is not lowered; a device that
 *   gives a workgroup less refuses the pairing with FMHIP_ERR_UNSUPPORTED
 *   rows of at most FMHIP_FFM_MAX_ROW entries and the other limits of the data: the dataset's own (fmhip_ffm_dataset_create)
 *   a feature id above the model's num_attribute, a field id >= the model's num_fields: FMHIP_ERR_INVALID at the first call that
 *   pairs the two
 * WORKSPACE of training, allocated at the first step for the dataset's largest batch of R rows (an allocation failure is
 * FMHIP_ERR_NOMEM): at most 4 (R (L (3 Pp + 2 rank) + 2 Pp) + ceil(R / 512) (L (2 Pp rank + Pp) + Pp)) bytes beside the FwFM's.
 *
 * Not here: the full-rank C_l, the mixture of low-rank experts, an MLP beside or behind the cross network (the paper's parallel and
 * stacked forms), the gate non-linearities inside the bottleneck; dropout and batch-norm, Adam, the data-parallel exchanges
 * (fmhip_dp_*), example weights, pairs / the BPR trainer, relational data, FTRL-Proximal, include/sparkfm.hpp and the JNI shim.
 */
#ifndef FMHIP_DCN_H
#define FMHIP_DCN_H
#include "fmhip_ffm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FMHIP_DCN_MAX_FIELDS 64
#define FMHIP_DCN_MAX_FACTORS 16
#define FMHIP_DCN_MAX_WIDTH 768
#define FMHIP_DCN_MAX_LAYERS 3
#define FMHIP_DCN_MAX_RANK 256

typedef struct fmhip_dcn_model *fmhip_dcn_model_t;

/* ---- model ---- */
/* Every parameter starts at zero, the rule at squared loss + SGD, the linear terms on, the cross part trained.  `stream`: a
 * hipStream_t (NULL: the library creates its own non-blocking stream).  The limits above are checked before the device is looked at. */
int fmhip_dcn_model_create(int device, int64_t num_attribute, int32_t num_fields, int32_t num_factor, int32_t n_layers, int32_t rank, void *stream,
                           fmhip_dcn_model_t *out);
int fmhip_dcn_model_destroy(fmhip_dcn_model_t m);
/* padded_factors: floats per feature vector on the device: 4, 8 or 16.  All out pointers nullable */
int fmhip_dcn_model_info(fmhip_dcn_model_t m, int64_t *num_attribute, int32_t *num_fields, int32_t *num_factor, int32_t *padded_factors, int32_t *n_layers,
                         int32_t *rank);
/* w: n + 1 doubles; v: (n + 1) * k doubles at v[i * k + d]; V, U, c: n_layers pointers each, V[l] the F k * rank doubles of V_l,
 * row-major with row f * k + d for slot d of field f, U[l] the rank * F k doubles of U_l, row-major, c[l] the F k doubles of c_l;
 * u: F k doubles; stored as fp32.  get: every pointer (and every pointer inside V, U and c) nullable */
int fmhip_dcn_model_set_params(fmhip_dcn_model_t m, double w0, const double *w, const double *v, const double *const *V, const double *const *U,
                               const double *const *c, const double *u);
int fmhip_dcn_model_get_params(fmhip_dcn_model_t m, double *w0, double *w, double *v, double *const *V, double *const *U, double *const *c, double *u);
/* as fmhip_fwfm_model_set_rule; AdaGrad also allocates and fills the dense part's accumulators */
int fmhip_dcn_model_set_rule(fmhip_dcn_model_t m, int loss, int optimizer, double eps, double init);
/* linear = 0: w0 and w are read and never stepped; 1: stepped */
int fmhip_dcn_model_set_linear(fmhip_dcn_model_t m, int linear);
/* train = 0: V_l, U_l, c_l and u are read and never stepped; 1: stepped */
int fmhip_dcn_model_set_cross(fmhip_dcn_model_t m, int train);
/* AdaGrad's accumulators, laid out like the parameters.  FMHIP_ERR_INVALID unless the model is under AdaGrad; set: every value finite
 * and >= 0 */
int fmhip_dcn_model_get_accumulators(fmhip_dcn_model_t m, double *n0, double *nw, double *nv, double *const *nV, double *const *nU, double *const *nc,
                                     double *nu);
int fmhip_dcn_model_set_accumulators(fmhip_dcn_model_t m, double n0, const double *nw, const double *nv, const double *const *nV, const double *const *nU,
                                     const double *const *nc, const double *nu);

/* ---- compute ---- */
/* yhat: n_rows doubles, the margins (under either loss) */
int fmhip_dcn_predict(fmhip_dcn_model_t m, fmhip_ffm_dataset_t d, double *yhat);
/* One step on batch `batch`, asynchronous on the model's stream; a non-NULL stats synchronises (as fmhip_ffm_step's) */
int fmhip_dcn_step(fmhip_dcn_model_t m, fmhip_ffm_dataset_t d, int64_t batch, double eta, double reg0, double regw, double regv, double regd,
                   fmhip_stats *stats);
/* One pass over the batches in `order` (NULL: ascending; else n_batches ids, each in range); nothing inside it synchronises with the
 * host.  stats (nullable; synchronises): the sums over the epoch's batches */
int fmhip_dcn_epoch(fmhip_dcn_model_t m, fmhip_ffm_dataset_t d, double eta, double reg0, double regw, double regv, double regd, const int64_t *order,
                    fmhip_stats *stats);

#ifdef __cplusplus
}
#endif
#endif /* FMHIP_DCN_H */
