// fmhip_cin.hip — the C ABI of xDeepFM's Compressed Interaction Network (include/fmhip_cin.h): the model handle, the refusals, and the
// launch sequence of a step — fm_cin.hip's forward (the layers forwards and backwards for a tile of rows), its weight gradients,
// fm_fwfm.hip's backward and update for v, w, w0 and the statistics, then the CIN part's own update.  The data handle is the FFM's
// (fmhip_ffm_dataset.h), read and never changed; what the handle shares with the other field models is fmhip_field_model.h's.
#include "../../include/fmhip_cin.h"
#include "fm_cin.h"
#include "fmhip_field_model.h"

using namespace fmhip;
using namespace fmhip::host;

static_assert(FMHIP_CIN_MAX_FIELDS == kFfmMaxFields, "fmhip_cin.h and fmhip_host.h disagree on the fields");
static_assert(FMHIP_CIN_MAX_FACTORS == kCinMaxFactors && FMHIP_CIN_MAX_MAPS == kCinMaxMaps, "fmhip_cin.h and fm_cin.h disagree on the widths");
static_assert(FMHIP_CIN_MAX_LAYERS == kCinMaxLayers && kCinMaxLayers == kFieldMaxLayers, "fmhip_cin.h, fm_cin.h and fmhip_field_layout.h disagree on the layers");
static_assert(kFwfmChunkLen == kFfmChunk, "fm_fwfm.h and fmhip_host.h disagree on the chunk length");

struct fmhip_cin_model : FieldCore {
    int lds_limit = 0;
    CinSlots s;          // the layers and their maps, and where W_l and u sit in D
    DevBuf<float> D, ND;
    // workspace (fm_cin.h)
    DevBuf<float> xw[kCinMaxLayers], gw[kCinMaxLayers], pw, gpart;
};

namespace {

constexpr FieldNames kNames{"CIN", "CIN", "cin", "regd"};

// the caller's arrays by (slot map array, layer): W_l, u
template <typename T>
auto arrays(T *const *W, T *u) {
    return [=](int a, int l) -> T * { return a == 0 ? (W ? W[l] : nullptr) : u; };
}

int check_dense_pointers(const fmhip_cin_model *m, const double *const *W, const double *u) {
    if (!W || !u) return fail(FMHIP_ERR_INVALID, "NULL argument");
    const int l = first_null_layer(m->s, arrays(W, u));
    return l < 0 ? FMHIP_OK : fail(FMHIP_ERR_INVALID, "layer %d: NULL argument", l);
}

// every refusal of (m, d) that needs no launch, then the device and the workspace
int pair_up(fmhip_cin_model_t m, fmhip_ffm_dataset_t d, bool train) {
    const CinSlots &s = m->s;
    TRY(pair_refusals(*m, d, train));
    if (cin_row_tile(s.k, s.Fp, s.L, s.H, train, m->lds_limit) == 0)
        return fail(FMHIP_ERR_UNSUPPORTED, "a one-row tile takes %zu bytes of LDS, the device gives a workgroup %d",
                    cin_forward_lds(1, s.k, s.Fp, s.L, s.H, train) + cin_forward_static(), m->lds_limit);
    const size_t rows = (size_t)std::max<int64_t>(d->max_rows, 1);
    TRY(pair_workspace(*m, d, train, (size_t)cin_forward_blocks(rows)));
    if (train) {
        if (m->train) {
            const size_t mrows = rows * s.k;
            TRY(m->xw[0].ensure(mrows * s.Fp));
            for (int l = 1; l <= s.L; ++l) {
                if (l < s.L) TRY(m->xw[l].ensure(mrows * s.H[l]));
                TRY(m->gw[l - 1].ensure(mrows * s.H[l]));
            }
            TRY(m->pw.ensure(rows * (s.total() - s.uoff)));
        }
        TRY(m->gpart.ensure((size_t)cin_grad_splits(rows) * s.total()));          // (also what the FwFM's update launch is handed as rpart)
    }
    return FMHIP_OK;
}

CinArgs batch_args(fmhip_cin_model_t m, fmhip_ffm_dataset_t d, const FfmBatch &b) {
    const CinSlots &s = m->s;
    CinArgs q{};
    q.b = fwfm_args(*m, d, b, cin_forward_blocks(b.rows));
    q.b.Nr = m->ND.p;               // (the FwFM's update launch wants the pointers; with train_r = 0 it reads neither)
    q.b.rpart = m->gpart.p;
    q.D = m->D.p;
    q.ND = m->ND.p;
    q.k = m->k;
    q.Fp = s.Fp;
    q.L = s.L;
    q.H[0] = s.F;
    for (int l = 1; l <= s.L; ++l) {
        q.H[l] = s.H[l];
        q.woff[l - 1] = s.woff[l - 1];
        q.xw[l - 1] = m->xw[l - 1].p;
        q.gw[l - 1] = m->gw[l - 1].p;
    }
    q.uoff = s.uoff;
    q.total = s.n_total;
    q.pw = m->pw.p;
    q.gpart = m->gpart.p;
    q.n_splits = cin_grad_splits(b.rows);
    q.train_d = m->train;
    q.lds_limit = m->lds_limit;
    return q;
}

hipError_t forward(fmhip_cin_model_t m, fmhip_ffm_dataset_t d, const FfmBatch &b, float *yhat) {
    CinArgs a = batch_args(m, d, b);
    a.b.yhat = yhat;
    return launch_cin_forward(a, false, m->stream);
}

int one_step(fmhip_cin_model_t m, fmhip_ffm_dataset_t d, int64_t b, const Rates &q, double *acc, bool acc_reset) {
    CinArgs a = batch_args(m, d, d->batches[(size_t)b]);
    set_rates(a.b, q, acc, acc_reset);
    a.regd = (float)q.regx;
    const bool ada = m->opt == FMHIP_OPT_ADAGRAD;
    HIP_TRY(launch_cin_forward(a, true, m->stream));
    if (m->train) HIP_TRY(launch_cin_wgrad(a, m->stream));
    HIP_TRY(launch_fwfm_backward(a.b, ada, m->stream));
    HIP_TRY(launch_fwfm_update(a.b, ada, m->stream));
    if (m->train) HIP_TRY(launch_cin_dupdate(a, ada, m->stream));
    return FMHIP_OK;
}

}  // namespace

extern "C" {

int fmhip_cin_model_create(int device, int64_t num_attribute, int32_t num_fields, int32_t num_factor, int32_t n_layers, const int32_t *feature_maps,
                           void *stream, fmhip_cin_model_t *out) {
    TRY(check_field_shape(kNames, out, num_attribute, num_fields, num_factor, FMHIP_CIN_MAX_FACTORS));
    if (n_layers < 1) return fail(FMHIP_ERR_INVALID, "n_layers = %d: the CIN has at least one layer", n_layers);
    if (n_layers > FMHIP_CIN_MAX_LAYERS) return fail(FMHIP_ERR_UNSUPPORTED, "n_layers = %d is above FMHIP_CIN_MAX_LAYERS = %d", n_layers, FMHIP_CIN_MAX_LAYERS);
    if (!feature_maps) return fail(FMHIP_ERR_INVALID, "feature_maps is NULL");
    for (int l = 0; l < n_layers; ++l) {
        const int32_t h = feature_maps[l];
        if (h > FMHIP_CIN_MAX_MAPS) return fail(FMHIP_ERR_UNSUPPORTED, "feature_maps[%d] = %d is above FMHIP_CIN_MAX_MAPS = %d", l, h, FMHIP_CIN_MAX_MAPS);
        if (h < 16 || h % 16) return fail(FMHIP_ERR_INVALID, "feature_maps[%d] = %d: a layer's map count is a multiple of 16, at least 16", l, h);
    }
    TRY(check_feature_ids(num_attribute));
    TRY(set_device(device));
    fmhip_cin_model *m = new (std::nothrow) fmhip_cin_model();
    if (!m) return fail(FMHIP_ERR_NOMEM, "out of host memory");
    set_shape(*m, device, num_attribute, num_fields, num_factor);
    m->s = CinSlots(num_fields, num_factor, n_layers, feature_maps);
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

int fmhip_cin_model_destroy(fmhip_cin_model_t m) { return destroy_model(m); }

int fmhip_cin_model_info(fmhip_cin_model_t m, int64_t *num_attribute, int32_t *num_fields, int32_t *num_factor, int32_t *padded_factors, int32_t *n_layers,
                         int32_t *feature_maps) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the CIN model handle is NULL");
    model_info(*m, num_attribute, num_fields, num_factor, padded_factors);
    if (n_layers) *n_layers = m->s.L;
    if (feature_maps)
        for (int l = 1; l <= m->s.L; ++l) feature_maps[l - 1] = m->s.H[l];
    return FMHIP_OK;
}

int fmhip_cin_model_set_params(fmhip_cin_model_t m, double w0, const double *w, const double *v, const double *const *W, const double *u) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the CIN model handle is NULL");
    if (!w || !v) return fail(FMHIP_ERR_INVALID, "NULL argument");
    TRY(check_dense_pointers(m, W, u));
    return set_params(*m, w0, w, v, m->D.p, m->s, arrays(W, u));
}

int fmhip_cin_model_get_params(fmhip_cin_model_t m, double *w0, double *w, double *v, double *const *W, double *u) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the CIN model handle is NULL");
    return get_params(*m, w0, w, v, m->D.p, m->s, W || u, arrays(W, u));
}

int fmhip_cin_model_set_rule(fmhip_cin_model_t m, int loss, int optimizer, double eps, double init) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the CIN model handle is NULL");
    return set_rule(*m, loss, optimizer, eps, init, m->ND, m->s.total());
}

int fmhip_cin_model_set_linear(fmhip_cin_model_t m, int linear) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the CIN model handle is NULL");
    return set_flag(*m, &FieldCore::linear, "linear", linear);
}

int fmhip_cin_model_set_cin(fmhip_cin_model_t m, int train) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the CIN model handle is NULL");
    return set_flag(*m, &FieldCore::train, "train", train);
}

int fmhip_cin_model_get_accumulators(fmhip_cin_model_t m, double *n0, double *nw, double *nv, double *const *nW, double *nu) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the CIN model handle is NULL");
    return get_accumulators(*m, kNames, n0, nw, nv, m->ND.p, m->s, nW || nu, arrays(nW, nu));
}

int fmhip_cin_model_set_accumulators(fmhip_cin_model_t m, double n0, const double *nw, const double *nv, const double *const *nW, const double *nu) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the CIN model handle is NULL");
    if (!nw || !nv) return fail(FMHIP_ERR_INVALID, "NULL argument");
    TRY(check_dense_pointers(m, nW, nu));
    return set_accumulators(*m, kNames, n0, nw, nv, m->ND.p, m->s, arrays(nW, nu));
}

int fmhip_cin_predict(fmhip_cin_model_t m, fmhip_ffm_dataset_t d, double *yhat) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the CIN model handle is NULL");
    return predict(m, d, yhat, pair_up, forward);
}

int fmhip_cin_step(fmhip_cin_model_t m, fmhip_ffm_dataset_t d, int64_t batch, double eta, double reg0, double regw, double regv, double regd,
                   fmhip_stats *stats) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the CIN model handle is NULL");
    return step(m, kNames, d, batch, Rates{eta, reg0, regw, regv, regd}, stats, pair_up, one_step);
}

int fmhip_cin_epoch(fmhip_cin_model_t m, fmhip_ffm_dataset_t d, double eta, double reg0, double regw, double regv, double regd, const int64_t *order,
                    fmhip_stats *stats) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the CIN model handle is NULL");
    return epoch(m, kNames, d, Rates{eta, reg0, regw, regv, regd}, order, stats, pair_up, one_step);
}

}  // extern "C"
