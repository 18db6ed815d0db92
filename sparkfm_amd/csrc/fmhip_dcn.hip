// fmhip_dcn.hip — the C ABI of the low-rank cross network, DCN-V2 (include/fmhip_dcn.h): the model handle, the refusals, and the
// launch sequence of a step — fm_dcn.hip's forward (the cross layers forwards and backwards for a tile of rows), its weight gradients,
// fm_fwfm.hip's backward and update for v, w, w0 and the statistics, then the dense part's own update.  The data handle is the FFM's
// (fmhip_ffm_dataset.h), read and never changed; what the handle shares with the other field models is fmhip_field_model.h's.
#include "../../include/fmhip_dcn.h"
#include "fm_dcn.h"
#include "fmhip_field_model.h"

using namespace fmhip;
using namespace fmhip::host;

static_assert(FMHIP_DCN_MAX_FIELDS == kFfmMaxFields, "fmhip_dcn.h and fmhip_host.h disagree on the fields");
static_assert(FMHIP_DCN_MAX_WIDTH == kDcnMaxWidth, "fmhip_dcn.h and fm_dcn.h disagree on the width");
static_assert(FMHIP_DCN_MAX_LAYERS == kDcnMaxLayers && FMHIP_DCN_MAX_RANK == kDcnMaxRank, "fmhip_dcn.h and fm_dcn.h disagree on the layers");
static_assert(kDcnMaxLayers == kFieldMaxLayers, "fm_dcn.h and fmhip_field_layout.h disagree on the layers");
static_assert(kFwfmChunkLen == kFfmChunk, "fm_fwfm.h and fmhip_host.h disagree on the chunk length");
// the widest accepted model runs at a 16-row tile inside gfx950's 160 KB of LDS a workgroup may ask for
static_assert(dcn_forward_lds(16, kDcnMaxWidth, kDcnMaxRank) + dcn_forward_static(16) <= 160 * 1024, "the widest model's 16-row tile");

struct fmhip_dcn_model : FieldCore {
    int lds_limit = 0;
    DcnSlots s;          // the layers and the rank, and where V_l, U_l, c_l and u sit in D
    DevBuf<float> D, ND;
    // workspace (fm_dcn.h)
    DevBuf<float> sw, xw[kDcnMaxLayers], qw[kDcnMaxLayers], tw[kDcnMaxLayers], mw[kDcnMaxLayers], pw[kDcnMaxLayers], jw, gpart;
};

namespace {

constexpr FieldNames kNames{"DCN", "DCN", "dcn", "regd"};

// the caller's arrays by (slot map array, layer): V_l, U_l, c_l, u
template <typename T>
auto arrays(T *const *V, T *const *U, T *const *c, T *u) {
    return [=](int a, int l) -> T * { return a == 0 ? (V ? V[l] : nullptr) : (a == 1 ? (U ? U[l] : nullptr) : (a == 2 ? (c ? c[l] : nullptr) : u)); };
}

int check_dense_pointers(const fmhip_dcn_model *m, const double *const *V, const double *const *U, const double *const *c, const double *u) {
    if (!V || !U || !c || !u) return fail(FMHIP_ERR_INVALID, "NULL argument");
    const int l = first_null_layer(m->s, arrays(V, U, c, u));
    return l < 0 ? FMHIP_OK : fail(FMHIP_ERR_INVALID, "layer %d: NULL argument", l);
}

// every refusal of (m, d) that needs no launch, then the device and the workspace
int pair_up(fmhip_dcn_model_t m, fmhip_ffm_dataset_t d, bool train) {
    const DcnSlots &s = m->s;
    TRY(pair_refusals(*m, d, train));
    if (dcn_row_tile(s.Pp, s.r, m->lds_limit) == 0)
        return fail(FMHIP_ERR_UNSUPPORTED, "F·Kp = %d at rank = %d: a 16-row tile takes %zu bytes of LDS, the device gives a workgroup %d", m->F * m->Kp, s.r,
                    dcn_forward_lds(16, s.Pp, s.r) + dcn_forward_static(16), m->lds_limit);
    const size_t rows = (size_t)std::max<int64_t>(d->max_rows, 1);
    TRY(pair_workspace(*m, d, train, (size_t)dcn_forward_blocks(rows)));
    if (train) {
        for (int l = 0; l < s.L; ++l) TRY(m->pw[l].ensure(rows * s.Pp));
        if (s.L >= 2) TRY(m->jw.ensure(rows * s.Pp));
        if (m->train) {
            TRY(m->sw.ensure(rows * s.Pp));
            for (int l = 0; l < s.L; ++l) {
                TRY(m->xw[l].ensure(rows * s.Pp));
                TRY(m->qw[l].ensure(rows * s.Pp));
                TRY(m->tw[l].ensure(rows * s.r));
                TRY(m->mw[l].ensure(rows * s.r));
            }
        }
        TRY(m->gpart.ensure((size_t)dcn_grad_splits(rows) * s.total()));          // (also what the FwFM's update launch is handed as rpart)
    }
    return FMHIP_OK;
}

DcnArgs batch_args(fmhip_dcn_model_t m, fmhip_ffm_dataset_t d, const FfmBatch &b) {
    const DcnSlots &s = m->s;
    DcnArgs q{};
    q.b = fwfm_args(*m, d, b, dcn_forward_blocks(b.rows));
    q.b.Nr = m->ND.p;               // (the FwFM's update launch wants the pointers; with train_r = 0 it reads neither)
    q.b.rpart = m->gpart.p;
    q.D = m->D.p;
    q.ND = m->ND.p;
    q.k = m->k;
    q.Pp = s.Pp;
    q.L = s.L;
    q.r = s.r;
    for (int l = 0; l < s.L; ++l) {
        q.voff[l] = s.voff[l];
        q.uoff[l] = s.uoff[l];
        q.coff[l] = s.coff[l];
        q.xw[l] = m->xw[l].p;
        q.qw[l] = m->qw[l].p;
        q.tw[l] = m->tw[l].p;
        q.mw[l] = m->mw[l].p;
        q.pw[l] = m->pw[l].p;
    }
    q.hoff = s.hoff;
    q.total = s.n_total;
    q.sw = m->sw.p;
    q.jw = m->jw.p;
    q.gpart = m->gpart.p;
    q.n_splits = dcn_grad_splits(b.rows);
    q.train_d = m->train;
    q.lds_limit = m->lds_limit;
    return q;
}

hipError_t forward(fmhip_dcn_model_t m, fmhip_ffm_dataset_t d, const FfmBatch &b, float *yhat) {
    DcnArgs a = batch_args(m, d, b);
    a.b.yhat = yhat;
    return launch_dcn_forward(a, false, m->stream);
}

int one_step(fmhip_dcn_model_t m, fmhip_ffm_dataset_t d, int64_t b, const Rates &q, double *acc, bool acc_reset) {
    DcnArgs a = batch_args(m, d, d->batches[(size_t)b]);
    set_rates(a.b, q, acc, acc_reset);
    a.regd = (float)q.regx;
    const bool ada = m->opt == FMHIP_OPT_ADAGRAD;
    HIP_TRY(launch_dcn_forward(a, true, m->stream));
    if (m->train) HIP_TRY(launch_dcn_wgrad(a, m->stream));
    HIP_TRY(launch_fwfm_backward(a.b, ada, m->stream));
    HIP_TRY(launch_fwfm_update(a.b, ada, m->stream));
    if (m->train) HIP_TRY(launch_dcn_dupdate(a, ada, m->stream));
    return FMHIP_OK;
}

}  // namespace

extern "C" {

int fmhip_dcn_model_create(int device, int64_t num_attribute, int32_t num_fields, int32_t num_factor, int32_t n_layers, int32_t rank, void *stream,
                           fmhip_dcn_model_t *out) {
    TRY(check_field_shape(kNames, out, num_attribute, num_fields, num_factor, FMHIP_DCN_MAX_FACTORS));
    const int32_t Kp = field_kp(num_factor);
    if (num_fields * Kp > FMHIP_DCN_MAX_WIDTH)
        return fail(FMHIP_ERR_UNSUPPORTED, "num_fields = %d at num_factor = %d (padded to %d): F·Kp = %d is above %d", num_fields, num_factor, Kp, num_fields * Kp,
                    FMHIP_DCN_MAX_WIDTH);
    if (n_layers < 1) return fail(FMHIP_ERR_INVALID, "n_layers = %d: the cross network has at least one layer", n_layers);
    if (n_layers > FMHIP_DCN_MAX_LAYERS) return fail(FMHIP_ERR_UNSUPPORTED, "n_layers = %d is above FMHIP_DCN_MAX_LAYERS = %d", n_layers, FMHIP_DCN_MAX_LAYERS);
    if (rank > FMHIP_DCN_MAX_RANK) return fail(FMHIP_ERR_UNSUPPORTED, "rank = %d is above FMHIP_DCN_MAX_RANK = %d", rank, FMHIP_DCN_MAX_RANK);
    if (rank < 16 || rank % 16) return fail(FMHIP_ERR_INVALID, "rank = %d: the rank is a multiple of 16, at least 16", rank);
    TRY(check_feature_ids(num_attribute));
    TRY(set_device(device));
    fmhip_dcn_model *m = new (std::nothrow) fmhip_dcn_model();
    if (!m) return fail(FMHIP_ERR_NOMEM, "out of host memory");
    set_shape(*m, device, num_attribute, num_fields, num_factor);
    m->s = DcnSlots(num_fields, num_factor, n_layers, rank);
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

int fmhip_dcn_model_destroy(fmhip_dcn_model_t m) { return destroy_model(m); }

int fmhip_dcn_model_info(fmhip_dcn_model_t m, int64_t *num_attribute, int32_t *num_fields, int32_t *num_factor, int32_t *padded_factors, int32_t *n_layers,
                         int32_t *rank) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the DCN model handle is NULL");
    model_info(*m, num_attribute, num_fields, num_factor, padded_factors);
    if (n_layers) *n_layers = m->s.L;
    if (rank) *rank = m->s.r;
    return FMHIP_OK;
}

int fmhip_dcn_model_set_params(fmhip_dcn_model_t m, double w0, const double *w, const double *v, const double *const *V, const double *const *U,
                               const double *const *c, const double *u) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the DCN model handle is NULL");
    if (!w || !v) return fail(FMHIP_ERR_INVALID, "NULL argument");
    TRY(check_dense_pointers(m, V, U, c, u));
    return set_params(*m, w0, w, v, m->D.p, m->s, arrays(V, U, c, u));
}

int fmhip_dcn_model_get_params(fmhip_dcn_model_t m, double *w0, double *w, double *v, double *const *V, double *const *U, double *const *c, double *u) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the DCN model handle is NULL");
    return get_params(*m, w0, w, v, m->D.p, m->s, V || U || c || u, arrays(V, U, c, u));
}

int fmhip_dcn_model_set_rule(fmhip_dcn_model_t m, int loss, int optimizer, double eps, double init) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the DCN model handle is NULL");
    return set_rule(*m, loss, optimizer, eps, init, m->ND, m->s.total());
}

int fmhip_dcn_model_set_linear(fmhip_dcn_model_t m, int linear) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the DCN model handle is NULL");
    return set_flag(*m, &FieldCore::linear, "linear", linear);
}

int fmhip_dcn_model_set_cross(fmhip_dcn_model_t m, int train) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the DCN model handle is NULL");
    return set_flag(*m, &FieldCore::train, "train", train);
}

int fmhip_dcn_model_get_accumulators(fmhip_dcn_model_t m, double *n0, double *nw, double *nv, double *const *nV, double *const *nU, double *const *nc,
                                     double *nu) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the DCN model handle is NULL");
    return get_accumulators(*m, kNames, n0, nw, nv, m->ND.p, m->s, nV || nU || nc || nu, arrays(nV, nU, nc, nu));
}

int fmhip_dcn_model_set_accumulators(fmhip_dcn_model_t m, double n0, const double *nw, const double *nv, const double *const *nV, const double *const *nU,
                                     const double *const *nc, const double *nu) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the DCN model handle is NULL");
    if (!nw || !nv) return fail(FMHIP_ERR_INVALID, "NULL argument");
    TRY(check_dense_pointers(m, nV, nU, nc, nu));
    return set_accumulators(*m, kNames, n0, nw, nv, m->ND.p, m->s, arrays(nV, nU, nc, nu));
}

int fmhip_dcn_predict(fmhip_dcn_model_t m, fmhip_ffm_dataset_t d, double *yhat) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the DCN model handle is NULL");
    return predict(m, d, yhat, pair_up, forward);
}

int fmhip_dcn_step(fmhip_dcn_model_t m, fmhip_ffm_dataset_t d, int64_t batch, double eta, double reg0, double regw, double regv, double regd,
                   fmhip_stats *stats) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the DCN model handle is NULL");
    return step(m, kNames, d, batch, Rates{eta, reg0, regw, regv, regd}, stats, pair_up, one_step);
}

int fmhip_dcn_epoch(fmhip_dcn_model_t m, fmhip_ffm_dataset_t d, double eta, double reg0, double regw, double regv, double regd, const int64_t *order,
                    fmhip_stats *stats) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the DCN model handle is NULL");
    return epoch(m, kNames, d, Rates{eta, reg0, regw, regv, regd}, order, stats, pair_up, one_step);
}

}  // extern "C"
