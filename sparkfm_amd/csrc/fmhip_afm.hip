// fmhip_afm.hip — the C ABI of the Attentional Factorization Machine (include/fmhip_afm.h): the model handle, the refusals, and the
// launch sequence of a step — fm_afm.hip's forward (a wave per row, forwards and backwards), fm_fwfm.hip's backward and update for v,
// w, w0 and the statistics, then the attention part's own update.  The data handle is the FFM's (fmhip_ffm_dataset.h), read and never
// changed; what the handle shares with the other field models is fmhip_field_model.h's.
#include "../../include/fmhip_afm.h"
#include "fm_afm.h"
#include "fmhip_field_model.h"

using namespace fmhip;
using namespace fmhip::host;

static_assert(FMHIP_AFM_MAX_FIELDS == kFfmMaxFields, "fmhip_afm.h and fmhip_host.h disagree on the fields");
static_assert(FMHIP_AFM_MAX_FACTORS == kAfmMaxFactors && FMHIP_AFM_MAX_ATTENTION == kAfmMaxAttention, "fmhip_afm.h and fm_afm.h disagree on the widths");
static_assert(kFwfmChunkLen == kFfmChunk, "fm_fwfm.h and fmhip_host.h disagree on the chunk length");

struct fmhip_afm_model : FieldCore {
    int lds_limit = 0;
    AfmSlots s;          // the attention factor, and where W, b, h and p sit in D
    DevBuf<float> D, ND;
    DevBuf<float> gpart;          // workspace (fm_afm.h)
};

namespace {

constexpr FieldNames kNames{"AFM", "AFM", "afm", "regd"};

// the caller's arrays by (slot map array, layer): W, b, h, p
template <typename T>
auto arrays(T *W, T *b, T *h, T *p) {
    return [=](int a, int) -> T * { return a == 0 ? W : (a == 1 ? b : (a == 2 ? h : p)); };
}

// every refusal of (m, d) that needs no launch, then the device and the workspace
int pair_up(fmhip_afm_model_t m, fmhip_ffm_dataset_t d, bool train) {
    TRY(pair_refusals(*m, d, train));
    const size_t lds = afm_forward_lds(m->Fp(), m->Kp, train) + afm_forward_static();
    if (lds > (size_t)m->lds_limit)
        return fail(FMHIP_ERR_UNSUPPORTED, "a workgroup takes %zu bytes of LDS, the device gives a workgroup %d", lds, m->lds_limit);
    const size_t blocks = (size_t)afm_forward_blocks(std::max<int64_t>(d->max_rows, 1));
    TRY(pair_workspace(*m, d, train, blocks));
    if (train) TRY(m->gpart.ensure(blocks * m->s.total()));          // (also what the FwFM's update launch is handed as rpart)
    return FMHIP_OK;
}

AfmArgs batch_args(fmhip_afm_model_t m, fmhip_ffm_dataset_t d, const FfmBatch &b) {
    AfmArgs q{};
    q.b = fwfm_args(*m, d, b, afm_forward_blocks(b.rows));
    q.b.Nr = m->ND.p;               // (the FwFM's update launch wants the pointers; with train_r = 0 it reads neither)
    q.b.rpart = m->gpart.p;
    q.D = m->D.p;
    q.ND = m->ND.p;
    q.k = m->k;
    q.t = m->s.t;
    q.total = (int32_t)m->s.total();
    q.gpart = m->gpart.p;
    q.n_splits = afm_forward_blocks(b.rows);
    q.train_d = m->train;
    q.lds_limit = m->lds_limit;
    return q;
}

hipError_t forward(fmhip_afm_model_t m, fmhip_ffm_dataset_t d, const FfmBatch &b, float *yhat) {
    AfmArgs a = batch_args(m, d, b);
    a.b.yhat = yhat;
    return launch_afm_forward(a, false, m->stream);
}

int one_step(fmhip_afm_model_t m, fmhip_ffm_dataset_t d, int64_t b, const Rates &q, double *acc, bool acc_reset) {
    AfmArgs a = batch_args(m, d, d->batches[(size_t)b]);
    set_rates(a.b, q, acc, acc_reset);
    a.regd = (float)q.regx;
    const bool ada = m->opt == FMHIP_OPT_ADAGRAD;
    HIP_TRY(launch_afm_forward(a, true, m->stream));
    HIP_TRY(launch_fwfm_backward(a.b, ada, m->stream));
    HIP_TRY(launch_fwfm_update(a.b, ada, m->stream));
    if (m->train) HIP_TRY(launch_afm_dupdate(a, ada, m->stream));
    return FMHIP_OK;
}

}  // namespace

extern "C" {

int fmhip_afm_model_create(int device, int64_t num_attribute, int32_t num_fields, int32_t num_factor, int32_t attention_factor, void *stream,
                           fmhip_afm_model_t *out) {
    TRY(check_field_shape(kNames, out, num_attribute, num_fields, num_factor, FMHIP_AFM_MAX_FACTORS));
    if (attention_factor > FMHIP_AFM_MAX_ATTENTION)
        return fail(FMHIP_ERR_UNSUPPORTED, "attention_factor = %d is above FMHIP_AFM_MAX_ATTENTION = %d", attention_factor, FMHIP_AFM_MAX_ATTENTION);
    if (attention_factor < 16 || attention_factor % 16)
        return fail(FMHIP_ERR_INVALID, "attention_factor = %d: the attention factor is a multiple of 16, at least 16", attention_factor);
    TRY(check_feature_ids(num_attribute));
    TRY(set_device(device));
    fmhip_afm_model *m = new (std::nothrow) fmhip_afm_model();
    if (!m) return fail(FMHIP_ERR_NOMEM, "out of host memory");
    set_shape(*m, device, num_attribute, num_fields, num_factor);
    m->s = AfmSlots(num_fields, num_factor, attention_factor);
    hipError_t e = hipDeviceGetAttribute(&m->lds_limit, hipDeviceAttributeMaxSharedMemoryPerBlock, device);
    if (e != hipSuccess) {
        delete m;
        return fail(FMHIP_ERR_HIP, "hipDeviceGetAttribute failed: %s", hipGetErrorString(e));
    }
    if (int rc = open_model(*m, kNames, stream, m->D, m->s.total(), nullptr)) {
        destroy_model(m);
        return rc;
    }
    *out = m;
    return FMHIP_OK;
}

int fmhip_afm_model_destroy(fmhip_afm_model_t m) { return destroy_model(m); }

int fmhip_afm_model_info(fmhip_afm_model_t m, int64_t *num_attribute, int32_t *num_fields, int32_t *num_factor, int32_t *padded_factors,
                         int32_t *attention_factor) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the AFM model handle is NULL");
    model_info(*m, num_attribute, num_fields, num_factor, padded_factors);
    if (attention_factor) *attention_factor = m->s.t;
    return FMHIP_OK;
}

int fmhip_afm_model_set_params(fmhip_afm_model_t m, double w0, const double *w, const double *v, const double *W, const double *b, const double *h,
                               const double *p) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the AFM model handle is NULL");
    if (!w || !v || !W || !b || !h || !p) return fail(FMHIP_ERR_INVALID, "NULL argument");
    return set_params(*m, w0, w, v, m->D.p, m->s, arrays(W, b, h, p));
}

int fmhip_afm_model_get_params(fmhip_afm_model_t m, double *w0, double *w, double *v, double *W, double *b, double *h, double *p) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the AFM model handle is NULL");
    return get_params(*m, w0, w, v, m->D.p, m->s, W || b || h || p, arrays(W, b, h, p));
}

int fmhip_afm_model_set_rule(fmhip_afm_model_t m, int loss, int optimizer, double eps, double init) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the AFM model handle is NULL");
    return set_rule(*m, loss, optimizer, eps, init, m->ND, m->s.total());
}

int fmhip_afm_model_set_linear(fmhip_afm_model_t m, int linear) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the AFM model handle is NULL");
    return set_flag(*m, &FieldCore::linear, "linear", linear);
}

int fmhip_afm_model_set_attention(fmhip_afm_model_t m, int train) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the AFM model handle is NULL");
    return set_flag(*m, &FieldCore::train, "train", train);
}

int fmhip_afm_model_get_accumulators(fmhip_afm_model_t m, double *n0, double *nw, double *nv, double *nW, double *nb, double *nh, double *np) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the AFM model handle is NULL");
    return get_accumulators(*m, kNames, n0, nw, nv, m->ND.p, m->s, nW || nb || nh || np, arrays(nW, nb, nh, np));
}

int fmhip_afm_model_set_accumulators(fmhip_afm_model_t m, double n0, const double *nw, const double *nv, const double *nW, const double *nb,
                                     const double *nh, const double *np) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the AFM model handle is NULL");
    if (!nw || !nv || !nW || !nb || !nh || !np) return fail(FMHIP_ERR_INVALID, "NULL argument");
    return set_accumulators(*m, kNames, n0, nw, nv, m->ND.p, m->s, arrays(nW, nb, nh, np));
}

int fmhip_afm_predict(fmhip_afm_model_t m, fmhip_ffm_dataset_t d, double *yhat) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the AFM model handle is NULL");
    return predict(m, d, yhat, pair_up, forward);
}

int fmhip_afm_step(fmhip_afm_model_t m, fmhip_ffm_dataset_t d, int64_t batch, double eta, double reg0, double regw, double regv, double regd,
                   fmhip_stats *stats) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the AFM model handle is NULL");
    return step(m, kNames, d, batch, Rates{eta, reg0, regw, regv, regd}, stats, pair_up, one_step);
}

int fmhip_afm_epoch(fmhip_afm_model_t m, fmhip_ffm_dataset_t d, double eta, double reg0, double regw, double regv, double regd, const int64_t *order,
                    fmhip_stats *stats) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the AFM model handle is NULL");
    return epoch(m, kNames, d, Rates{eta, reg0, regw, regv, regd}, order, stats, pair_up, one_step);
}

}  // extern "C"
