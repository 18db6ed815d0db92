// fmhip_autoint.hip — the C ABI of AutoInt (include/fmhip_autoint.h): the model handle, the refusals, and the launch sequence of a
// step — fm_autoint.hip's forward (the attention layers forwards and backwards, a row at a time), fm_fwfm.hip's backward and update for
// v, w, w0 and the statistics, then the dense part's own update.  The data handle is the FFM's (fmhip_ffm_dataset.h), read and never
// changed; what the handle shares with the other field models is fmhip_field_model.h's.
#include "../../include/fmhip_autoint.h"
#include "fm_autoint.h"
#include "fmhip_field_model.h"

using namespace fmhip;
using namespace fmhip::host;

static_assert(FMHIP_AUTOINT_MAX_FIELDS == kFfmMaxFields, "fmhip_autoint.h and fmhip_host.h disagree on the fields");
static_assert(FMHIP_AUTOINT_MAX_FACTORS == kAutoIntMaxFactors && FMHIP_AUTOINT_MAX_WIDTH == kAutoIntMaxWidth, "fmhip_autoint.h and fm_autoint.h disagree on the widths");
static_assert(FMHIP_AUTOINT_MAX_LAYERS == kAutoIntMaxLayers && FMHIP_AUTOINT_MAX_HEADS == kAutoIntMaxHeads && FMHIP_AUTOINT_MAX_HEAD_DIM == kAutoIntMaxHeadDim,
              "fmhip_autoint.h and fm_autoint.h disagree on the layers");
static_assert(kAutoIntMaxLayers == kFieldMaxLayers, "fm_autoint.h and fmhip_field_layout.h disagree on the layers");
static_assert(kFwfmChunkLen == kFfmChunk, "fm_fwfm.h and fmhip_host.h disagree on the chunk length");
// the largest accepted model runs inside gfx950's 160 KB of LDS a workgroup may ask for
static_assert(autoint_forward_lds(64, kAutoIntMaxWidth, kAutoIntMaxLayers, true) <= 160 * 1024, "the largest model's row");

struct fmhip_autoint_model : FieldCore {
    int32_t H = 0, d = 0;
    AutoIntSlots s;          // the layers and A = H d, and where W_l and u sit in D
    DevBuf<float> D, ND;
    DevBuf<float> scratch, gpart;          // workspace (fm_autoint.h)
};

namespace {

constexpr FieldNames kNames{"AutoInt", "AUTOINT", "autoint", "regd"};

// the caller's arrays by (slot map array, layer): W_l, u
template <typename T>
auto arrays(T *const *W, T *u) {
    return [=](int a, int l) -> T * { return a == 0 ? (W ? W[l] : nullptr) : u; };
}

int check_dense_pointers(const fmhip_autoint_model *m, const double *const *W, const double *u) {
    if (!W || !u) return fail(FMHIP_ERR_INVALID, "NULL argument");
    const int l = first_null_layer(m->s, arrays(W, u));
    return l < 0 ? FMHIP_OK : fail(FMHIP_ERR_INVALID, "layer %d: NULL argument", l);
}

// every refusal of (m, d) that needs no launch, then the device and the workspace
int pair_up(fmhip_autoint_model_t m, fmhip_ffm_dataset_t d, bool train) {
    TRY(pair_refusals(*m, d, train));
    const size_t blocks = (size_t)autoint_forward_blocks(std::max<int64_t>(d->max_rows, 1));
    TRY(pair_workspace(*m, d, train, blocks));
    if (train) {
        if (m->s.L > 1) TRY(m->scratch.ensure(blocks * autoint_scratch(m->Fp(), m->s.A, m->s.L)));
        TRY(m->gpart.ensure(blocks * m->s.total()));          // (also what the FwFM's update launch is handed as rpart)
    }
    return FMHIP_OK;
}

AutoIntArgs batch_args(fmhip_autoint_model_t m, fmhip_ffm_dataset_t d, const FfmBatch &b) {
    const AutoIntSlots &s = m->s;
    AutoIntArgs q{};
    q.b = fwfm_args(*m, d, b, autoint_forward_blocks(b.rows));
    q.b.Nr = m->ND.p;               // (the FwFM's update launch wants the pointers; with train_r = 0 it reads neither)
    q.b.rpart = m->gpart.p;
    q.D = m->D.p;
    q.ND = m->ND.p;
    q.k = m->k;
    q.L = s.L;
    q.H = m->H;
    q.d = m->d;
    q.A = s.A;
    for (int l = 0; l < s.L; ++l) q.woff[l] = s.woff[l];
    q.hoff = s.hoff;
    q.total = s.n_total;
    q.scratch = m->scratch.p;
    q.gpart = m->gpart.p;
    q.n_splits = autoint_forward_blocks(b.rows);
    q.train_d = m->train;
    return q;
}

hipError_t forward(fmhip_autoint_model_t m, fmhip_ffm_dataset_t d, const FfmBatch &b, float *yhat) {
    AutoIntArgs a = batch_args(m, d, b);
    a.b.yhat = yhat;
    return launch_autoint_forward(a, false, m->stream);
}

int one_step(fmhip_autoint_model_t m, fmhip_ffm_dataset_t d, int64_t b, const Rates &q, double *acc, bool acc_reset) {
    AutoIntArgs a = batch_args(m, d, d->batches[(size_t)b]);
    set_rates(a.b, q, acc, acc_reset);
    a.regd = (float)q.regx;
    const bool ada = m->opt == FMHIP_OPT_ADAGRAD;
    HIP_TRY(launch_autoint_forward(a, true, m->stream));
    HIP_TRY(launch_fwfm_backward(a.b, ada, m->stream));
    HIP_TRY(launch_fwfm_update(a.b, ada, m->stream));
    if (m->train) HIP_TRY(launch_autoint_dupdate(a, ada, m->stream));
    return FMHIP_OK;
}

}  // namespace

extern "C" {

int fmhip_autoint_model_create(int device, int64_t num_attribute, int32_t num_fields, int32_t num_factor, int32_t n_layers, int32_t heads, int32_t head_dim,
                               void *stream, fmhip_autoint_model_t *out) {
    TRY(check_field_shape(kNames, out, num_attribute, num_fields, num_factor, FMHIP_AUTOINT_MAX_FACTORS));
    if (n_layers < 1) return fail(FMHIP_ERR_INVALID, "n_layers = %d: the attention has at least one layer", n_layers);
    if (n_layers > FMHIP_AUTOINT_MAX_LAYERS)
        return fail(FMHIP_ERR_UNSUPPORTED, "n_layers = %d is above FMHIP_AUTOINT_MAX_LAYERS = %d", n_layers, FMHIP_AUTOINT_MAX_LAYERS);
    if (heads > FMHIP_AUTOINT_MAX_HEADS) return fail(FMHIP_ERR_UNSUPPORTED, "heads = %d is above FMHIP_AUTOINT_MAX_HEADS = %d", heads, FMHIP_AUTOINT_MAX_HEADS);
    if (heads != 1 && heads != 2 && heads != 4) return fail(FMHIP_ERR_INVALID, "heads = %d: 1, 2 or 4", heads);
    if (head_dim > FMHIP_AUTOINT_MAX_HEAD_DIM)
        return fail(FMHIP_ERR_UNSUPPORTED, "head_dim = %d is above FMHIP_AUTOINT_MAX_HEAD_DIM = %d", head_dim, FMHIP_AUTOINT_MAX_HEAD_DIM);
    if (head_dim != 16 && head_dim != 32) return fail(FMHIP_ERR_INVALID, "head_dim = %d: 16 or 32", head_dim);
    if (heads * head_dim > FMHIP_AUTOINT_MAX_WIDTH)
        return fail(FMHIP_ERR_UNSUPPORTED, "heads = %d at head_dim = %d: heads·head_dim = %d is above FMHIP_AUTOINT_MAX_WIDTH = %d", heads, head_dim,
                    heads * head_dim, FMHIP_AUTOINT_MAX_WIDTH);
    TRY(check_feature_ids(num_attribute));
    TRY(set_device(device));
    const int32_t Fp = round16(num_fields), A = heads * head_dim;
    int lds_limit = 0;
    hipError_t e = hipDeviceGetAttribute(&lds_limit, hipDeviceAttributeMaxSharedMemoryPerBlock, device);
    if (e != hipSuccess) return fail(FMHIP_ERR_HIP, "hipDeviceGetAttribute failed: %s", hipGetErrorString(e));
    if (autoint_forward_lds(Fp, A, n_layers, true) > (size_t)lds_limit)
        return fail(FMHIP_ERR_UNSUPPORTED, "num_fields = %d at heads·head_dim = %d and n_layers = %d: a row takes %zu bytes of LDS, the device gives a workgroup %d",
                    num_fields, A, n_layers, autoint_forward_lds(Fp, A, n_layers, true), lds_limit);
    fmhip_autoint_model *m = new (std::nothrow) fmhip_autoint_model();
    if (!m) return fail(FMHIP_ERR_NOMEM, "out of host memory");
    set_shape(*m, device, num_attribute, num_fields, num_factor);
    m->H = heads;
    m->d = head_dim;
    m->s = AutoIntSlots(num_fields, num_factor, n_layers, A, kAutoIntD0);
    if (int rc = open_model(*m, kNames, stream, m->D, m->s.total(), nullptr)) {
        destroy_model(m);
        return rc;
    }
    *out = m;
    return FMHIP_OK;
}

int fmhip_autoint_model_destroy(fmhip_autoint_model_t m) { return destroy_model(m); }

int fmhip_autoint_model_info(fmhip_autoint_model_t m, int64_t *num_attribute, int32_t *num_fields, int32_t *num_factor, int32_t *padded_factors,
                             int32_t *n_layers, int32_t *heads, int32_t *head_dim) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the AutoInt model handle is NULL");
    model_info(*m, num_attribute, num_fields, num_factor, padded_factors);
    if (n_layers) *n_layers = m->s.L;
    if (heads) *heads = m->H;
    if (head_dim) *head_dim = m->d;
    return FMHIP_OK;
}

int fmhip_autoint_model_set_params(fmhip_autoint_model_t m, double w0, const double *w, const double *v, const double *const *W, const double *u) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the AutoInt model handle is NULL");
    if (!w || !v) return fail(FMHIP_ERR_INVALID, "NULL argument");
    TRY(check_dense_pointers(m, W, u));
    return set_params(*m, w0, w, v, m->D.p, m->s, arrays(W, u));
}

int fmhip_autoint_model_get_params(fmhip_autoint_model_t m, double *w0, double *w, double *v, double *const *W, double *u) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the AutoInt model handle is NULL");
    return get_params(*m, w0, w, v, m->D.p, m->s, W || u, arrays(W, u));
}

int fmhip_autoint_model_set_rule(fmhip_autoint_model_t m, int loss, int optimizer, double eps, double init) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the AutoInt model handle is NULL");
    return set_rule(*m, loss, optimizer, eps, init, m->ND, m->s.total());
}

int fmhip_autoint_model_set_linear(fmhip_autoint_model_t m, int linear) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the AutoInt model handle is NULL");
    return set_flag(*m, &FieldCore::linear, "linear", linear);
}

int fmhip_autoint_model_set_attention(fmhip_autoint_model_t m, int train) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the AutoInt model handle is NULL");
    return set_flag(*m, &FieldCore::train, "train", train);
}

int fmhip_autoint_model_get_accumulators(fmhip_autoint_model_t m, double *n0, double *nw, double *nv, double *const *nW, double *nu) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the AutoInt model handle is NULL");
    return get_accumulators(*m, kNames, n0, nw, nv, m->ND.p, m->s, nW || nu, arrays(nW, nu));
}

int fmhip_autoint_model_set_accumulators(fmhip_autoint_model_t m, double n0, const double *nw, const double *nv, const double *const *nW, const double *nu) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the AutoInt model handle is NULL");
    if (!nw || !nv) return fail(FMHIP_ERR_INVALID, "NULL argument");
    TRY(check_dense_pointers(m, nW, nu));
    return set_accumulators(*m, kNames, n0, nw, nv, m->ND.p, m->s, arrays(nW, nu));
}

int fmhip_autoint_predict(fmhip_autoint_model_t m, fmhip_ffm_dataset_t d, double *yhat) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the AutoInt model handle is NULL");
    return predict(m, d, yhat, pair_up, forward);
}

int fmhip_autoint_step(fmhip_autoint_model_t m, fmhip_ffm_dataset_t d, int64_t batch, double eta, double reg0, double regw, double regv, double regd,
                       fmhip_stats *stats) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the AutoInt model handle is NULL");
    return step(m, kNames, d, batch, Rates{eta, reg0, regw, regv, regd}, stats, pair_up, one_step);
}

int fmhip_autoint_epoch(fmhip_autoint_model_t m, fmhip_ffm_dataset_t d, double eta, double reg0, double regw, double regv, double regd, const int64_t *order,
                        fmhip_stats *stats) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the AutoInt model handle is NULL");
    return epoch(m, kNames, d, Rates{eta, reg0, regw, regv, regd}, order, stats, pair_up, one_step);
}

}  // extern "C"
