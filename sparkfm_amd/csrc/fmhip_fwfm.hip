// fmhip_fwfm.hip — the C ABI of the field-weighted FM (include/fmhip_fwfm.h): the model handle, the refusals, and the launch sequence
// of a step — fm_fwfm.hip's three kernels.  The data handle is the FFM's (fmhip_ffm_dataset.h), read and never changed; what the handle
// shares with the other field models is fmhip_field_model.h's.
#include "../../include/fmhip_fwfm.h"
#include "fmhip_field_model.h"

using namespace fmhip;
using namespace fmhip::host;

static_assert(FMHIP_FWFM_MAX_FIELDS == kFfmMaxFields, "fmhip_fwfm.h and fmhip_host.h disagree on the fields");
static_assert(kFwfmChunkLen == kFfmChunk, "fm_fwfm.h and fmhip_host.h disagree on the chunk length");

struct fmhip_fwfm_model : FieldCore {
    DevBuf<float> r, Nr;
    DevBuf<float> rpart;          // workspace
    FwfmSlots slots() const { return FwfmSlots(F); }
};

namespace {

constexpr FieldNames kNames{"FwFM", "FWFM", "fwfm", "regr"};

int check_symmetric(const fmhip_fwfm_model *m, const double *r, const char *name) {
    for (int f = 0; f < m->F; ++f)
        for (int g = f + 1; g < m->F; ++g)
            if ((float)r[f * m->F + g] != (float)r[g * m->F + f] && !(std::isnan(r[f * m->F + g]) && std::isnan(r[g * m->F + f])))
                return fail(FMHIP_ERR_INVALID, "%s[%d][%d] = %g but %s[%d][%d] = %g: the field weights are symmetric", name, f, g, r[f * m->F + g], name, g, f,
                            r[g * m->F + f]);
    return FMHIP_OK;
}

// every refusal of (m, d) that needs no launch, then the device and the workspace
int pair_up(fmhip_fwfm_model_t m, fmhip_ffm_dataset_t d, bool train) {
    TRY(pair_refusals(*m, d, train));
    const size_t blocks = (size_t)std::max(fwfm_forward_blocks(d->max_rows), 1);
    TRY(pair_workspace(*m, d, train, blocks));
    if (train) TRY(m->rpart.ensure(blocks * fwfm_rpart(m->Fp())));
    return FMHIP_OK;
}

FwfmArgs batch_args(fmhip_fwfm_model_t m, fmhip_ffm_dataset_t d, const FfmBatch &b) {
    FwfmArgs a = fwfm_args(*m, d, b, fwfm_forward_blocks(b.rows));
    a.r = m->r.p;
    a.Nr = m->Nr.p;
    a.rpart = m->rpart.p;
    a.train_r = m->train;
    return a;
}

hipError_t forward(fmhip_fwfm_model_t m, fmhip_ffm_dataset_t d, const FfmBatch &b, float *yhat) {
    FwfmArgs a = batch_args(m, d, b);
    a.yhat = yhat;
    return launch_fwfm_forward(a, false, m->stream);
}

int one_step(fmhip_fwfm_model_t m, fmhip_ffm_dataset_t d, int64_t b, const Rates &q, double *acc, bool acc_reset) {
    FwfmArgs a = batch_args(m, d, d->batches[(size_t)b]);
    set_rates(a, q, acc, acc_reset);
    a.regr = (float)q.regx;
    const bool ada = m->opt == FMHIP_OPT_ADAGRAD;
    HIP_TRY(launch_fwfm_forward(a, true, m->stream));
    HIP_TRY(launch_fwfm_backward(a, ada, m->stream));
    HIP_TRY(launch_fwfm_update(a, ada, m->stream));
    return FMHIP_OK;
}

}  // namespace

extern "C" {

int fmhip_fwfm_model_create(int device, int64_t num_attribute, int32_t num_fields, int32_t num_factor, void *stream, fmhip_fwfm_model_t *out) {
    TRY(check_field_shape(kNames, out, num_attribute, num_fields, num_factor, FMHIP_FWFM_MAX_FACTORS));
    TRY(check_feature_ids(num_attribute));
    TRY(set_device(device));
    fmhip_fwfm_model *m = new (std::nothrow) fmhip_fwfm_model();
    if (!m) return fail(FMHIP_ERR_NOMEM, "out of host memory");
    set_shape(*m, device, num_attribute, num_fields, num_factor);
    const std::vector<float> ones(m->slots().total(), 1.f);
    if (int rc = open_model(*m, kNames, stream, m->r, ones.size(), ones.data())) {
        destroy_model(m);
        return rc;
    }
    *out = m;
    return FMHIP_OK;
}

int fmhip_fwfm_model_destroy(fmhip_fwfm_model_t m) { return destroy_model(m); }

int fmhip_fwfm_model_info(fmhip_fwfm_model_t m, int64_t *num_attribute, int32_t *num_fields, int32_t *num_factor, int32_t *padded_factors) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the FwFM model handle is NULL");
    model_info(*m, num_attribute, num_fields, num_factor, padded_factors);
    return FMHIP_OK;
}

int fmhip_fwfm_model_set_params(fmhip_fwfm_model_t m, double w0, const double *w, const double *v, const double *r) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the FwFM model handle is NULL");
    if (!w || !v || !r) return fail(FMHIP_ERR_INVALID, "NULL argument");
    TRY(check_symmetric(m, r, "r"));
    return set_params(*m, w0, w, v, m->r.p, m->slots(), [=](int, int) { return r; });
}

int fmhip_fwfm_model_get_params(fmhip_fwfm_model_t m, double *w0, double *w, double *v, double *r) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the FwFM model handle is NULL");
    return get_params(*m, w0, w, v, m->r.p, m->slots(), r != nullptr, [=](int, int) { return r; });
}

int fmhip_fwfm_model_set_rule(fmhip_fwfm_model_t m, int loss, int optimizer, double eps, double init) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the FwFM model handle is NULL");
    return set_rule(*m, loss, optimizer, eps, init, m->Nr, m->slots().total());
}

int fmhip_fwfm_model_set_linear(fmhip_fwfm_model_t m, int linear) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the FwFM model handle is NULL");
    return set_flag(*m, &FieldCore::linear, "linear", linear);
}

int fmhip_fwfm_model_set_field_weights(fmhip_fwfm_model_t m, int train) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the FwFM model handle is NULL");
    return set_flag(*m, &FieldCore::train, "train", train);
}

int fmhip_fwfm_model_get_accumulators(fmhip_fwfm_model_t m, double *n0, double *nw, double *nv, double *nr) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the FwFM model handle is NULL");
    return get_accumulators(*m, kNames, n0, nw, nv, m->Nr.p, m->slots(), nr != nullptr, [=](int, int) { return nr; });
}

int fmhip_fwfm_model_set_accumulators(fmhip_fwfm_model_t m, double n0, const double *nw, const double *nv, const double *nr) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the FwFM model handle is NULL");
    if (!nw || !nv || !nr) return fail(FMHIP_ERR_INVALID, "NULL argument");
    return set_accumulators(*m, kNames, n0, nw, nv, m->Nr.p, m->slots(), [=](int, int) { return nr; }, [=] { return check_symmetric(m, nr, "nr"); });
}

int fmhip_fwfm_predict(fmhip_fwfm_model_t m, fmhip_ffm_dataset_t d, double *yhat) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the FwFM model handle is NULL");
    return predict(m, d, yhat, pair_up, forward);
}

int fmhip_fwfm_step(fmhip_fwfm_model_t m, fmhip_ffm_dataset_t d, int64_t batch, double eta, double reg0, double regw, double regv, double regr,
                    fmhip_stats *stats) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the FwFM model handle is NULL");
    return step(m, kNames, d, batch, Rates{eta, reg0, regw, regv, regr}, stats, pair_up, one_step);
}

int fmhip_fwfm_epoch(fmhip_fwfm_model_t m, fmhip_ffm_dataset_t d, double eta, double reg0, double regw, double regv, double regr,
                     const int64_t *order, fmhip_stats *stats) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the FwFM model handle is NULL");
    return epoch(m, kNames, d, Rates{eta, reg0, regw, regv, regr}, order, stats, pair_up, one_step);
}

}  // extern "C"
