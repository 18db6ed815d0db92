/*
 * fmhip_fmfm.h — field-matrixed factorization machines, FmFM / FM^2 (libfmhip.so): Sun et al., "FM^2: Field-matrixed Factorization
 * Machines for Recommender Systems", WWW 2021.  One factor vector per feature, as the plain FM keeps, and one learned k x k MATRIX
 * M[f][g] per PAIR OF FIELDS: between the field-weighted FM (fmhip_fwfm.h, a scalar per pair) and the field-aware FM (fmhip_ffm.h, F
 * vectors per feature).  A model and kernels of their own; the data handle is fmhip_ffm.h's fmhip_ffm_dataset_t, unchanged.
 *
 * THE MODEL.  A data row has entries (i_a, f_a, x_a), a = 0 .. L-1: feature id (at most once per row), field id, value.
 *   S_f  = sum_{a in field f} x_a v[i_a]                           (k floats; 0 for a field the row lacks)
 *   yhat = w0 + sum_a w[i_a] x_a + sum_{f<g} S_f^T M[f][g] S_g     v: (n + 1) x k,  M[f][g]: k x k,  M[g][f] := M[f][g]^T
 * Entries of one field are sum-pooled: there is no interaction inside a field (the CTR convention for multi-valued fields).  M[f][f]
 * is not a parameter: it reads as 0, and a set_params call that gives it a non-zero element is refused.
 * On rows with at most one entry per field, M[f][g] = I for every f != g is the plain FM and M[f][g] = r[f][g] I is fmhip_fwfm.h's
 * model; on any row it is that model with r[f][f] = 0.
 * With Z_f = sum_{g != f} M[f][g] S_g:
 *   the pair term is 1/2 sum_f <S_f, Z_f>;   d yhat / d v[i_a] = x_a Z_{f_a};
 *   d yhat / d M[f][g] = S_f S_g^T for f < g (one parameter block for the unordered pair)
 * Residuals, both losses, the 1/|B| mean, SGD / AdaGrad, eps, the accumulators' initial value, the statistics and `linear` are
 * fmhip_fwfm.h's.  The update: v[i] and w[i] step on g + reg theta for every feature present in the batch, every other feature keeps
 * every bit; w0 as in fmhip_fwfm.h; M is stepped densely every batch on g + regm M, with AdaGrad accumulators of its own.
 * A new model has v = w = w0 = 0 and M[f][g] = I for f != g.
 * Five launches per step, no atomics, every sum in an order fixed by the data and by compile-time constants: the same bits on every run.
 *
 * LIMITS, each refused before any launch (the message names the offending value):
 *   1 <= num_fields <= FMHIP_FMFM_MAX_FIELDS, 1 <= num_factor <= FMHIP_FMFM_MAX_FACTORS (padded to Kp = 4, 8 or 16 floats),
 *   num_fields * Kp <= FMHIP_FMFM_MAX_WIDTH, num_attribute >= 0: FMHIP_ERR_INVALID below a range, FMHIP_ERR_UNSUPPORTED above it
 *   (39 fields at k = 16 give 624 and 64 fields at k = 8 give 512; 64 fields at k = 16 are refused)
 *   rows of at most FMHIP_FFM_MAX_ROW entries and the other limits of the data: the dataset's own (fmhip_ffm_dataset_create)
 *   a feature id above the model's num_attribute, a field id >= the model's num_fields: FMHIP_ERR_INVALID at the first call that
 *   pairs the two
 *
 * Not here: the data-parallel exchanges (fmhip_dp_*), example weights, pairs / the BPR trainer, relational data, FTRL-Proximal,
 * per-field embedding sizes, pruning field pairs, include/sparkfm.hpp and the JNI shim.
 */
#ifndef FMHIP_FMFM_H
#define FMHIP_FMFM_H
#include "fmhip_ffm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FMHIP_FMFM_MAX_FIELDS 64
#define FMHIP_FMFM_MAX_FACTORS 16
#define FMHIP_FMFM_MAX_WIDTH 768

typedef struct fmhip_fmfm_model *fmhip_fmfm_model_t;

/* ---- model ---- */
/* v, w, w0 start at zero and M[f][g] at I (f != g), the rule at squared loss + SGD, the linear terms on, M trained.  `stream`: a
 * hipStream_t (NULL: the library creates its own non-blocking stream).  The limits above are checked before the device is looked at. */
int fmhip_fmfm_model_create(int device, int64_t num_attribute, int32_t num_fields, int32_t num_factor, void *stream, fmhip_fmfm_model_t *out);
int fmhip_fmfm_model_destroy(fmhip_fmfm_model_t m);
/* padded_factors: floats per feature vector on the device: 4, 8 or 16.  All out pointers nullable */
int fmhip_fmfm_model_info(fmhip_fmfm_model_t m, int64_t *num_attribute, int32_t *num_fields, int32_t *num_factor, int32_t *padded_factors);
/* w: n + 1 doubles; v: (n + 1) * k doubles at v[i * k + d]; m: F * F * k * k doubles at m[((f * F + g) * k + d) * k + d'] with
 * M[g][f][d'][d] == M[f][g][d][d'] after rounding to fp32 and every M[f][f] zero (set: FMHIP_ERR_INVALID otherwise, naming the element;
 * get: so); stored as fp32.  get: every pointer nullable */
int fmhip_fmfm_model_set_params(fmhip_fmfm_model_t m, double w0, const double *w, const double *v, const double *mm);
int fmhip_fmfm_model_get_params(fmhip_fmfm_model_t m, double *w0, double *w, double *v, double *mm);
/* as fmhip_fwfm_model_set_rule; AdaGrad also allocates and fills M's accumulators */
int fmhip_fmfm_model_set_rule(fmhip_fmfm_model_t m, int loss, int optimizer, double eps, double init);
/* linear = 0: w0 and w are read and never stepped; 1: stepped */
int fmhip_fmfm_model_set_linear(fmhip_fmfm_model_t m, int linear);
/* train = 0: M is read and never stepped (with M = I: the plain FM on rows of one entry per field); 1: stepped */
int fmhip_fmfm_model_set_field_matrices(fmhip_fmfm_model_t m, int train);
/* AdaGrad's accumulators, laid out like the parameters (nm: F * F * k * k, mirrored like m; its diagonal blocks are stored and never
 * used).  FMHIP_ERR_INVALID unless the model is under AdaGrad; set: every value finite and >= 0, nm mirrored */
int fmhip_fmfm_model_get_accumulators(fmhip_fmfm_model_t m, double *n0, double *nw, double *nv, double *nm);
int fmhip_fmfm_model_set_accumulators(fmhip_fmfm_model_t m, double n0, const double *nw, const double *nv, const double *nm);

/* ---- compute ---- */
/* yhat: n_rows doubles, the margins (under either loss) */
int fmhip_fmfm_predict(fmhip_fmfm_model_t m, fmhip_ffm_dataset_t d, double *yhat);
/* One step on batch `batch`, asynchronous on the model's stream; a non-NULL stats synchronises (as fmhip_ffm_step's) */
int fmhip_fmfm_step(fmhip_fmfm_model_t m, fmhip_ffm_dataset_t d, int64_t batch, double eta, double reg0, double regw, double regv, double regm,
                    fmhip_stats *stats);
/* One pass over the batches in `order` (NULL: ascending; else n_batches ids, each in range); nothing inside it synchronises with the
 * host.  stats (nullable; synchronises): the sums over the epoch's batches */
int fmhip_fmfm_epoch(fmhip_fmfm_model_t m, fmhip_ffm_dataset_t d, double eta, double reg0, double regw, double regv, double regm,
                     const int64_t *order, fmhip_stats *stats);

#ifdef __cplusplus
}
#endif
#endif /* FMHIP_FMFM_H */
