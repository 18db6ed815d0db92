// fmhip_fmfm.hip — the C ABI of the field-matrixed FM (include/fmhip_fmfm.h): the model handle, the refusals, and the launch sequence
// of a step — fm_fmfm.hip's forward, its gradient product, fm_fwfm.hip's backward and update for v, w, w0 and the statistics, then
// M's own update.  The data handle is the FFM's (fmhip_ffm_dataset.h), read and never changed; what the handle shares with the other
// field models is fmhip_field_model.h's.
#include "../../include/fmhip_fmfm.h"
#include "fm_fmfm.h"
#include "fmhip_field_model.h"

using namespace fmhip;
using namespace fmhip::host;

static_assert(FMHIP_FMFM_MAX_FIELDS == kFfmMaxFields, "fmhip_fmfm.h and fmhip_host.h disagree on the fields");
static_assert(FMHIP_FMFM_MAX_WIDTH == kFmfmMaxWidth, "fmhip_fmfm.h and fm_fmfm.h disagree on the width");
static_assert(kFwfmChunkLen == kFfmChunk, "fm_fwfm.h and fmhip_host.h disagree on the chunk length");

struct fmhip_fmfm_model : FieldCore {
    FmfmSlots s;          // where the caller's m sits in MM [Pp][Pp]
    DevBuf<float> MM, NM;
    DevBuf<float> sw, mpart;          // workspace
};

namespace {

constexpr FieldNames kNames{"FmFM", "FMFM", "fmfm", "regm"};

// M[g][f] == M[f][g]^T as fp32; with `diagonal` also M[f][f] == 0
int check_mirrored(const fmhip_fmfm_model *m, const double *mm, const char *name, bool diagonal) {
    for (int f = 0; f < m->F; ++f)
        for (int g = f; g < m->F; ++g)
            for (int d = 0; d < m->k; ++d)
                for (int d2 = 0; d2 < m->k; ++d2) {
                    const double x = mm[m->s.at(f, g, d, d2)], y = mm[m->s.at(g, f, d2, d)];
                    if (f == g) {
                        if (diagonal && x != 0.0)
                            return fail(FMHIP_ERR_INVALID, "%s[%d][%d][%d][%d] = %g: a field's own block is not a parameter, it is 0", name, f, f, d, d2, x);
                    } else if ((float)x != (float)y && !(std::isnan(x) && std::isnan(y))) {
                        return fail(FMHIP_ERR_INVALID, "%s[%d][%d][%d][%d] = %g but %s[%d][%d][%d][%d] = %g: M[g][f] is the transpose of M[f][g]", name, f, g, d, d2,
                                    x, name, g, f, d2, d, y);
                    }
                }
    return FMHIP_OK;
}

// every refusal of (m, d) that needs no launch, then the device and the workspace
int pair_up(fmhip_fmfm_model_t m, fmhip_ffm_dataset_t d, bool train) {
    TRY(pair_refusals(*m, d, train));
    const size_t rows = (size_t)std::max<int64_t>(d->max_rows, 1);
    TRY(pair_workspace(*m, d, train, (size_t)fmfm_forward_blocks(rows)));
    if (train) {
        TRY(m->sw.ensure(rows * m->s.Pp));
        TRY(m->mpart.ensure((size_t)fmfm_grad_splits(rows) * m->s.total()));
    }
    return FMHIP_OK;
}

FmfmArgs batch_args(fmhip_fmfm_model_t m, fmhip_ffm_dataset_t d, const FfmBatch &b) {
    FmfmArgs q{};
    q.b = fwfm_args(*m, d, b, fmfm_forward_blocks(b.rows));
    q.b.Nr = m->NM.p;               // (the FwFM's update launch wants the pointers; with train_r = 0 it reads neither)
    q.b.rpart = m->mpart.p;
    q.MM = m->MM.p;
    q.NM = m->NM.p;
    q.k = m->k;
    q.Pp = m->s.Pp;
    q.sw = m->sw.p;
    q.mpart = m->mpart.p;
    q.n_splits = fmfm_grad_splits(b.rows);
    q.train_m = m->train;
    return q;
}

hipError_t forward(fmhip_fmfm_model_t m, fmhip_ffm_dataset_t d, const FfmBatch &b, float *yhat) {
    FmfmArgs a = batch_args(m, d, b);
    a.b.yhat = yhat;
    return launch_fmfm_forward(a, false, m->stream);
}

int one_step(fmhip_fmfm_model_t m, fmhip_ffm_dataset_t d, int64_t b, const Rates &q, double *acc, bool acc_reset) {
    FmfmArgs a = batch_args(m, d, d->batches[(size_t)b]);
    set_rates(a.b, q, acc, acc_reset);
    a.regm = (float)q.regx;
    const bool ada = m->opt == FMHIP_OPT_ADAGRAD;
    HIP_TRY(launch_fmfm_forward(a, true, m->stream));
    if (m->train) HIP_TRY(launch_fmfm_mgrad(a, m->stream));
    HIP_TRY(launch_fwfm_backward(a.b, ada, m->stream));
    HIP_TRY(launch_fwfm_update(a.b, ada, m->stream));
    if (m->train) HIP_TRY(launch_fmfm_mupdate(a, ada, m->stream));
    return FMHIP_OK;
}

}  // namespace

extern "C" {

int fmhip_fmfm_model_create(int device, int64_t num_attribute, int32_t num_fields, int32_t num_factor, void *stream, fmhip_fmfm_model_t *out) {
    TRY(check_field_shape(kNames, out, num_attribute, num_fields, num_factor, FMHIP_FMFM_MAX_FACTORS));
    const int32_t Kp = field_kp(num_factor);
    if (num_fields * Kp > FMHIP_FMFM_MAX_WIDTH)
        return fail(FMHIP_ERR_UNSUPPORTED, "num_fields = %d at num_factor = %d (padded to %d): F·Kp = %d is above %d", num_fields, num_factor, Kp, num_fields * Kp,
                    FMHIP_FMFM_MAX_WIDTH);
    TRY(check_feature_ids(num_attribute));
    TRY(set_device(device));
    fmhip_fmfm_model *m = new (std::nothrow) fmhip_fmfm_model();
    if (!m) return fail(FMHIP_ERR_NOMEM, "out of host memory");
    set_shape(*m, device, num_attribute, num_fields, num_factor);
    m->s = FmfmSlots(num_fields, num_factor);
    std::vector<float> eye(m->s.total(), 0.f);
    for (int f = 0; f < m->F; ++f)
        for (int g = 0; g < m->F; ++g)
            for (int d = 0; d < m->k && f != g; ++d) eye[m->s.dev_at(f, g, d, d)] = 1.f;
    if (int rc = open_model(*m, kNames, stream, m->MM, eye.size(), eye.data())) {
        destroy_model(m);
        return rc;
    }
    *out = m;
    return FMHIP_OK;
}

int fmhip_fmfm_model_destroy(fmhip_fmfm_model_t m) { return destroy_model(m); }

int fmhip_fmfm_model_info(fmhip_fmfm_model_t m, int64_t *num_attribute, int32_t *num_fields, int32_t *num_factor, int32_t *padded_factors) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the FmFM model handle is NULL");
    model_info(*m, num_attribute, num_fields, num_factor, padded_factors);
    return FMHIP_OK;
}

int fmhip_fmfm_model_set_params(fmhip_fmfm_model_t m, double w0, const double *w, const double *v, const double *mm) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the FmFM model handle is NULL");
    if (!w || !v || !mm) return fail(FMHIP_ERR_INVALID, "NULL argument");
    TRY(check_mirrored(m, mm, "m", true));
    return set_params(*m, w0, w, v, m->MM.p, m->s, [=](int, int) { return mm; });
}

int fmhip_fmfm_model_get_params(fmhip_fmfm_model_t m, double *w0, double *w, double *v, double *mm) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the FmFM model handle is NULL");
    return get_params(*m, w0, w, v, m->MM.p, m->s, mm != nullptr, [=](int, int) { return mm; });
}

int fmhip_fmfm_model_set_rule(fmhip_fmfm_model_t m, int loss, int optimizer, double eps, double init) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the FmFM model handle is NULL");
    return set_rule(*m, loss, optimizer, eps, init, m->NM, m->s.total());
}

int fmhip_fmfm_model_set_linear(fmhip_fmfm_model_t m, int linear) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the FmFM model handle is NULL");
    return set_flag(*m, &FieldCore::linear, "linear", linear);
}

int fmhip_fmfm_model_set_field_matrices(fmhip_fmfm_model_t m, int train) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the FmFM model handle is NULL");
    return set_flag(*m, &FieldCore::train, "train", train);
}

int fmhip_fmfm_model_get_accumulators(fmhip_fmfm_model_t m, double *n0, double *nw, double *nv, double *nm) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the FmFM model handle is NULL");
    return get_accumulators(*m, kNames, n0, nw, nv, m->NM.p, m->s, nm != nullptr, [=](int, int) { return nm; });
}

int fmhip_fmfm_model_set_accumulators(fmhip_fmfm_model_t m, double n0, const double *nw, const double *nv, const double *nm) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the FmFM model handle is NULL");
    if (!nw || !nv || !nm) return fail(FMHIP_ERR_INVALID, "NULL argument");
    return set_accumulators(*m, kNames, n0, nw, nv, m->NM.p, m->s, [=](int, int) { return nm; }, [=] { return check_mirrored(m, nm, "nm", false); });
}

int fmhip_fmfm_predict(fmhip_fmfm_model_t m, fmhip_ffm_dataset_t d, double *yhat) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the FmFM model handle is NULL");
    return predict(m, d, yhat, pair_up, forward);
}

int fmhip_fmfm_step(fmhip_fmfm_model_t m, fmhip_ffm_dataset_t d, int64_t batch, double eta, double reg0, double regw, double regv, double regm,
                    fmhip_stats *stats) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the FmFM model handle is NULL");
    return step(m, kNames, d, batch, Rates{eta, reg0, regw, regv, regm}, stats, pair_up, one_step);
}

int fmhip_fmfm_epoch(fmhip_fmfm_model_t m, fmhip_ffm_dataset_t d, double eta, double reg0, double regw, double regv, double regm,
                     const int64_t *order, fmhip_stats *stats) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the FmFM model handle is NULL");
    return epoch(m, kNames, d, Rates{eta, reg0, regw, regv, regm}, order, stats, pair_up, one_step);
}

}  // extern "C"
