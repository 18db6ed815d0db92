// fmhip_pnn.hip — the C ABI of the product-based neural network (include/fmhip_pnn.h): the model handle, the refusals, and the launch
// sequence of a step — fm_pnn.hip's forward (the Gram tiles, the MLP forwards and backwards for a tile of rows), its weight gradients,
// fm_fwfm.hip's backward and update for v, w, w0 and the statistics, then fm_deepfm.hip's dense update.  The data handle is the FFM's
// (fmhip_ffm_dataset.h), read and never changed; what the handle shares with the other field models is fmhip_field_model.h's.
#include "../../include/fmhip_pnn.h"
#include "fm_pnn.h"
#include "fmhip_field_model.h"

using namespace fmhip;
using namespace fmhip::host;

static_assert(FMHIP_PNN_MAX_FIELDS == kFfmMaxFields, "fmhip_pnn.h and fmhip_host.h disagree on the fields");
static_assert(FMHIP_PNN_MAX_WIDTH == kPnnMaxWidth, "fmhip_pnn.h and fm_pnn.h disagree on the width");
static_assert(FMHIP_PNN_MAX_LAYERS == kDeepMaxLayers && FMHIP_PNN_MAX_UNITS == kDeepMaxUnits, "fmhip_pnn.h and fm_deepfm.h disagree on the layers");
static_assert(kDeepMaxLayers == kFieldMaxLayers, "fm_deepfm.h and fmhip_field_layout.h disagree on the layers");
static_assert(kFwfmChunkLen == kFfmChunk, "fm_fwfm.h and fmhip_host.h disagree on the chunk length");

struct fmhip_pnn_model : FieldCore {
    int lds_limit = 0;
    PnnSlots s;          // the widths, and where W_l, b_l and u sit in D
    PnnTiles tiles;      // the kernels' table of the Gram tiles (the slot map's, tile for tile)
    DevBuf<float> D, ND;
    DevBuf<float> sw, hw[kDeepMaxLayers], dw[kDeepMaxLayers], gpart;          // workspace
};

namespace {

constexpr FieldNames kNames{"PNN", "PNN", "pnn", "regd"};

// the caller's arrays by (slot map array, layer): W_l, b_l, u
template <typename T>
auto arrays(T *const *W, T *const *b, T *u) {
    return [=](int a, int l) -> T * { return a == 0 ? (W ? W[l] : nullptr) : (a == 1 ? (b ? b[l] : nullptr) : u); };
}

int check_dense_pointers(const fmhip_pnn_model *m, const double *const *W, const double *const *b, const double *u) {
    if (!W || !b || !u) return fail(FMHIP_ERR_INVALID, "NULL argument");
    const int l = first_null_layer(m->s, arrays(W, b, u));
    return l < 0 ? FMHIP_OK : fail(FMHIP_ERR_INVALID, "layer %d: NULL argument", l + 1);
}

int wy(const PnnSlots &s) { return std::max(s.width[1], s.L >= 3 ? s.width[3] : 0); }
int wz(const PnnSlots &s) { return std::max(kPnnStage, s.L >= 2 ? s.width[2] : 0); }

// every refusal of (m, d) that needs no launch, then the device and the workspace
int pair_up(fmhip_pnn_model_t m, fmhip_ffm_dataset_t d, bool train) {
    TRY(pair_refusals(*m, d, train));
    if (pnn_row_tile(m->s.Pp, wy(m->s), wz(m->s), train, m->lds_limit) == 0)
        return fail(FMHIP_ERR_UNSUPPORTED, "a workgroup takes %zu bytes of LDS, the device gives a workgroup %d",
                    pnn_forward_lds(16, m->s.Pp, wy(m->s), wz(m->s), train) + kPnnStaticLds, m->lds_limit);
    const size_t rows = (size_t)std::max<int64_t>(d->max_rows, 1);
    TRY(pair_workspace(*m, d, train, (size_t)pnn_forward_blocks(rows)));
    if (train) {
        for (int l = 0; l < m->s.L; ++l) TRY(m->hw[l].ensure(rows * m->s.width[l + 1]));
        TRY(m->gpart.ensure((size_t)deepfm_grad_splits(rows) * m->s.total()));          // (also what the FwFM's update launch is handed as rpart)
        if (m->train) {
            TRY(m->sw.ensure(rows * m->s.width[0]));
            for (int l = 0; l < m->s.L; ++l) TRY(m->dw[l].ensure(rows * m->s.width[l + 1]));
        }
    }
    return FMHIP_OK;
}

PnnArgs batch_args(fmhip_pnn_model_t m, fmhip_ffm_dataset_t d, const FfmBatch &b) {
    const PnnSlots &s = m->s;
    PnnArgs p{};
    DeepfmArgs &q = p.d;
    q.b = fwfm_args(*m, d, b, pnn_forward_blocks(b.rows));
    q.b.Nr = m->ND.p;               // (the FwFM's update launch wants the pointers; with train_r = 0 it reads neither)
    q.b.rpart = m->gpart.p;
    q.D = m->D.p;
    q.ND = m->ND.p;
    q.k = m->k;
    q.Pp = s.Pp;
    q.L = s.L;
    for (int l = 0; l <= s.L; ++l) q.n[l] = s.width[l];
    for (int l = 0; l < s.L; ++l) {
        q.woff[l] = s.woff[l];
        q.boff[l] = s.boff[l];
        q.hw[l] = m->hw[l].p;
        q.dw[l] = m->dw[l].p;
    }
    q.uoff = s.uoff;
    q.total = s.n_total;
    q.sw = m->sw.p;
    q.gpart = m->gpart.p;
    q.n_splits = deepfm_grad_splits(b.rows);
    q.train_d = m->train;
    p.t = m->tiles;
    p.lds_limit = m->lds_limit;
    return p;
}

hipError_t forward(fmhip_pnn_model_t m, fmhip_ffm_dataset_t d, const FfmBatch &b, float *yhat) {
    PnnArgs a = batch_args(m, d, b);
    a.d.b.yhat = yhat;
    return launch_pnn_forward(a, false, m->stream);
}

int one_step(fmhip_pnn_model_t m, fmhip_ffm_dataset_t d, int64_t b, const Rates &q, double *acc, bool acc_reset) {
    PnnArgs a = batch_args(m, d, d->batches[(size_t)b]);
    set_rates(a.d.b, q, acc, acc_reset);
    a.d.regd = (float)q.regx;
    const bool ada = m->opt == FMHIP_OPT_ADAGRAD;
    HIP_TRY(launch_pnn_forward(a, true, m->stream));
    if (m->train) HIP_TRY(launch_pnn_wgrad(a, m->stream));
    HIP_TRY(launch_fwfm_backward(a.d.b, ada, m->stream));
    HIP_TRY(launch_fwfm_update(a.d.b, ada, m->stream));
    if (m->train) HIP_TRY(launch_deepfm_dupdate(a.d, ada, m->stream));
    return FMHIP_OK;
}

}  // namespace

extern "C" {

int fmhip_pnn_model_create(int device, int64_t num_attribute, int32_t num_fields, int32_t num_factor, int32_t n_layers, const int32_t *widths,
                           void *stream, fmhip_pnn_model_t *out) {
    TRY(check_field_shape(kNames, out, num_attribute, num_fields, num_factor, FMHIP_PNN_MAX_FACTORS));
    const int32_t Kp = field_kp(num_factor), G = num_fields * (num_fields - 1) / 2, width = round16(num_fields * Kp) + round16(G);
    if (width > FMHIP_PNN_MAX_WIDTH)
        return fail(FMHIP_ERR_UNSUPPORTED, "num_fields = %d at num_factor = %d (padded to %d): the width round16(F·Kp) + round16(G) = %d + %d = %d is above FMHIP_PNN_MAX_WIDTH = %d",
                    num_fields, num_factor, Kp, round16(num_fields * Kp), round16(G), width, FMHIP_PNN_MAX_WIDTH);
    if (n_layers < 1) return fail(FMHIP_ERR_INVALID, "n_layers = %d: the dense part has at least one layer", n_layers);
    if (n_layers > FMHIP_PNN_MAX_LAYERS) return fail(FMHIP_ERR_UNSUPPORTED, "n_layers = %d is above FMHIP_PNN_MAX_LAYERS = %d", n_layers, FMHIP_PNN_MAX_LAYERS);
    if (!widths) return fail(FMHIP_ERR_INVALID, "widths is NULL");
    for (int l = 0; l < n_layers; ++l) {
        if (widths[l] < 16 || widths[l] % 16) return fail(FMHIP_ERR_INVALID, "widths[%d] = %d: a layer's width is a multiple of 16, at least 16", l, widths[l]);
        if (widths[l] > FMHIP_PNN_MAX_UNITS) return fail(FMHIP_ERR_UNSUPPORTED, "widths[%d] = %d is above FMHIP_PNN_MAX_UNITS = %d", l, widths[l], FMHIP_PNN_MAX_UNITS);
    }
    TRY(check_feature_ids(num_attribute));
    TRY(set_device(device));
    fmhip_pnn_model *m = new (std::nothrow) fmhip_pnn_model();
    if (!m) return fail(FMHIP_ERR_NOMEM, "out of host memory");
    set_shape(*m, device, num_attribute, num_fields, num_factor);
    m->s = PnnSlots(num_fields, num_factor, n_layers, widths);
    pnn_tiles(num_fields, m->tiles);          // (the launchers refuse a table that disagrees with the slot map's height of W_1)
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

int fmhip_pnn_model_destroy(fmhip_pnn_model_t m) { return destroy_model(m); }

int fmhip_pnn_model_info(fmhip_pnn_model_t m, int64_t *num_attribute, int32_t *num_fields, int32_t *num_factor, int32_t *padded_factors,
                         int32_t *n_layers, int32_t *widths) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the PNN model handle is NULL");
    model_info(*m, num_attribute, num_fields, num_factor, padded_factors);
    if (n_layers) *n_layers = m->s.L;
    if (widths)
        for (int l = 0; l < m->s.L; ++l) widths[l] = m->s.width[l + 1];
    return FMHIP_OK;
}

int fmhip_pnn_model_set_params(fmhip_pnn_model_t m, double w0, const double *w, const double *v, const double *const *W, const double *const *b,
                               const double *u) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the PNN model handle is NULL");
    if (!w || !v) return fail(FMHIP_ERR_INVALID, "NULL argument");
    TRY(check_dense_pointers(m, W, b, u));
    return set_params(*m, w0, w, v, m->D.p, m->s, arrays(W, b, u));
}

int fmhip_pnn_model_get_params(fmhip_pnn_model_t m, double *w0, double *w, double *v, double *const *W, double *const *b, double *u) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the PNN model handle is NULL");
    return get_params(*m, w0, w, v, m->D.p, m->s, W || b || u, arrays(W, b, u));
}

int fmhip_pnn_model_set_rule(fmhip_pnn_model_t m, int loss, int optimizer, double eps, double init) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the PNN model handle is NULL");
    return set_rule(*m, loss, optimizer, eps, init, m->ND, m->s.total());
}

int fmhip_pnn_model_set_linear(fmhip_pnn_model_t m, int linear) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the PNN model handle is NULL");
    return set_flag(*m, &FieldCore::linear, "linear", linear);
}

int fmhip_pnn_model_set_deep(fmhip_pnn_model_t m, int train) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the PNN model handle is NULL");
    return set_flag(*m, &FieldCore::train, "train", train);
}

int fmhip_pnn_model_get_accumulators(fmhip_pnn_model_t m, double *n0, double *nw, double *nv, double *const *nW, double *const *nb, double *nu) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the PNN model handle is NULL");
    return get_accumulators(*m, kNames, n0, nw, nv, m->ND.p, m->s, nW || nb || nu, arrays(nW, nb, nu));
}

int fmhip_pnn_model_set_accumulators(fmhip_pnn_model_t m, double n0, const double *nw, const double *nv, const double *const *nW,
                                     const double *const *nb, const double *nu) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the PNN model handle is NULL");
    if (!nw || !nv) return fail(FMHIP_ERR_INVALID, "NULL argument");
    TRY(check_dense_pointers(m, nW, nb, nu));
    return set_accumulators(*m, kNames, n0, nw, nv, m->ND.p, m->s, arrays(nW, nb, nu));
}

int fmhip_pnn_predict(fmhip_pnn_model_t m, fmhip_ffm_dataset_t d, double *yhat) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the PNN model handle is NULL");
    return predict(m, d, yhat, pair_up, forward);
}

int fmhip_pnn_step(fmhip_pnn_model_t m, fmhip_ffm_dataset_t d, int64_t batch, double eta, double reg0, double regw, double regv, double regd,
                   fmhip_stats *stats) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the PNN model handle is NULL");
    return step(m, kNames, d, batch, Rates{eta, reg0, regw, regv, regd}, stats, pair_up, one_step);
}

int fmhip_pnn_epoch(fmhip_pnn_model_t m, fmhip_ffm_dataset_t d, double eta, double reg0, double regw, double regv, double regd,
                    const int64_t *order, fmhip_stats *stats) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the PNN model handle is NULL");
    return epoch(m, kNames, d, Rates{eta, reg0, regw, regv, regd}, order, stats, pair_up, one_step);
}

}  // extern "C"
