/*
 * fmhip_fwfm.h — field-weighted factorization machines (libfmhip.so): Pan et al., "Field-weighted Factorization Machines for
 * Click-Through Rate Prediction in Display Advertising", WWW 2018.  One factor vector per feature, as the plain FM keeps, and one
 * learned scalar r[f][g] per PAIR OF FIELDS: the field-pair strengths of the field-aware FM (fmhip_ffm.h) at the plain FM's size.
 * A model and kernels of their own; the data handle is fmhip_ffm.h's fmhip_ffm_dataset_t, unchanged.
 *
 * THE MODEL.  A data row has entries (i_a, f_a, x_a), a = 0 .. L-1: feature id (at most once per row), field id, value.
 *   yhat = w0 + sum_a w[i_a] x_a + sum_{a<b} x_a x_b r[f_a][f_b] <v[i_a], v[i_b]>       v: (n + 1) x k,  r: F x F symmetric
 * Entries that share a field interact through r[f][f], like any other pair.  With r == 1 it is the plain FM.
 * With u_a = x_a v[i_a], S_f = sum_{a in f} u_a, R0 = r without its diagonal, Z0 = R0 S and D_a = Z0[f_a] + r[f_a][f_a] (S_{f_a} - u_a):
 *   the pair term is 1/2 sum_a <u_a, D_a>;   d yhat / d v[i_a] = x_a D_a;
 *   d yhat / d r[f][g] = <S_f, S_g> for f < g (one parameter for the symmetric pair);  d yhat / d r[f][f] = 1/2 sum_{a in f} <u_a, S_f - u_a>
 * A field that holds one entry in a row contributes exactly 0 to r[f][f]'s gradient.
 * Residuals, losses, the 1/|B| mean, SGD / AdaGrad, eps and the accumulators' initial value are fmhip_ffm.h's.  The update: v[i] and w[i]
 * step on g + reg theta for every feature present in the batch, every other feature keeps every bit; w0 as in fmhip_ffm.h; r (at most
 * 2080 numbers) is stepped densely every batch on g + regr r, with AdaGrad accumulators of its own.
 * A new model has v = w = w0 = 0 and r == 1.
 * Three launches per step, no atomics, every sum in an order fixed by the data and by compile-time constants: the same bits on every run.
 *
 * LIMITS, each refused before any launch (the message names the offending value):
 *   1 <= num_fields <= FMHIP_FWFM_MAX_FIELDS, 1 <= num_factor <= FMHIP_FWFM_MAX_FACTORS (padded to 4, 8, 16 or 32 floats),
 *   num_attribute >= 0: FMHIP_ERR_INVALID below the range, FMHIP_ERR_UNSUPPORTED above it
 *   rows of at most FMHIP_FFM_MAX_ROW entries and the other limits of the data: the dataset's own (fmhip_ffm_dataset_create)
 *   a feature id above the model's num_attribute, a field id >= the model's num_fields: FMHIP_ERR_INVALID at the first call that
 *   pairs the two
 *
 * Not here: the data-parallel exchanges (fmhip_dp_*), example weights, pairs / the BPR trainer, relational data, FTRL-Proximal,
 * ALS / MCMC, include/sparkfm.hpp and the JNI shim.
 */
#ifndef FMHIP_FWFM_H
#define FMHIP_FWFM_H
#include "fmhip_ffm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FMHIP_FWFM_MAX_FIELDS 64
#define FMHIP_FWFM_MAX_FACTORS 32

typedef struct fmhip_fwfm_model *fmhip_fwfm_model_t;

/* ---- model ---- */
/* v, w, w0 start at zero and r at 1, the rule at squared loss + SGD, the linear terms on, r trained.  `stream`: a hipStream_t (NULL:
 * the library creates its own non-blocking stream).  The limits above are checked before the device is looked at. */
int fmhip_fwfm_model_create(int device, int64_t num_attribute, int32_t num_fields, int32_t num_factor, void *stream, fmhip_fwfm_model_t *out);
int fmhip_fwfm_model_destroy(fmhip_fwfm_model_t m);
/* padded_factors: floats per feature vector on the device: 4, 8, 16 or 32.  All out pointers nullable */
int fmhip_fwfm_model_info(fmhip_fwfm_model_t m, int64_t *num_attribute, int32_t *num_fields, int32_t *num_factor, int32_t *padded_factors);
/* w: n + 1 doubles; v: (n + 1) * k doubles at v[i * k + d]; r: F * F doubles at r[f * F + g], symmetric (set: FMHIP_ERR_INVALID
 * otherwise, naming the pair; get: symmetric); stored as fp32.  get: every pointer nullable */
int fmhip_fwfm_model_set_params(fmhip_fwfm_model_t m, double w0, const double *w, const double *v, const double *r);
int fmhip_fwfm_model_get_params(fmhip_fwfm_model_t m, double *w0, double *w, double *v, double *r);
/* as fmhip_ffm_model_set_rule; AdaGrad also allocates and fills r's accumulators */
int fmhip_fwfm_model_set_rule(fmhip_fwfm_model_t m, int loss, int optimizer, double eps, double init);
/* linear = 0: w0 and w are read and never stepped; 1: stepped */
int fmhip_fwfm_model_set_linear(fmhip_fwfm_model_t m, int linear);
/* train = 0: r is read and never stepped (with r == 1: the plain FM); 1: stepped */
int fmhip_fwfm_model_set_field_weights(fmhip_fwfm_model_t m, int train);
/* AdaGrad's accumulators, laid out like the parameters (nr: F * F, symmetric).  FMHIP_ERR_INVALID unless the model is under AdaGrad;
 * set: every value finite and >= 0, nr symmetric */
int fmhip_fwfm_model_get_accumulators(fmhip_fwfm_model_t m, double *n0, double *nw, double *nv, double *nr);
int fmhip_fwfm_model_set_accumulators(fmhip_fwfm_model_t m, double n0, const double *nw, const double *nv, const double *nr);

/* ---- compute ---- */
/* yhat: n_rows doubles, the margins (under either loss) */
int fmhip_fwfm_predict(fmhip_fwfm_model_t m, fmhip_ffm_dataset_t d, double *yhat);
/* One step on batch `batch`, asynchronous on the model's stream; a non-NULL stats synchronises (as fmhip_ffm_step's) */
int fmhip_fwfm_step(fmhip_fwfm_model_t m, fmhip_ffm_dataset_t d, int64_t batch, double eta, double reg0, double regw, double regv, double regr,
                    fmhip_stats *stats);
/* One pass over the batches in `order` (NULL: ascending; else n_batches ids, each in range); nothing inside it synchronises with the
 * host.  stats (nullable; synchronises): the sums over the epoch's batches */
int fmhip_fwfm_epoch(fmhip_fwfm_model_t m, fmhip_ffm_dataset_t d, double eta, double reg0, double regw, double regv, double regr,
                     const int64_t *order, fmhip_stats *stats);

#ifdef __cplusplus
}
#endif
#endif /* FMHIP_FWFM_H */
