// fmhip_field_model.h — what the handles of the field models that step through the FwFM's backward and update launches share (FwFM,
// FmFM, DeepFM, DCN, AutoInt: fmhip_<model>.hip): the state of a handle, the codecs, the refusals, the rule, and the scaffold of
// predict, step and epoch.  A unit's handle inherits FieldCore and adds its own parameter array (a slot map of fmhip_field_layout.h
// says where its elements sit), its workspace and its launch sequence.  The helpers at the top take any handle with a stream: the
// FFM's (fmhip_ffm.hip) uses those.  Not installed, not part of the ABI.
#pragma once
#include "../../include/fmhip_ffm.h"
#include "fm_fwfm.h"
#include "fmhip_ffm_dataset.h"
#include "fmhip_field_layout.h"
#include "fmhip_internal.h"

#include <algorithm>
#include <cmath>
#include <mutex>
#include <new>
#include <vector>

namespace fmhip {
namespace host {

// ---- for any handle with a stream ------------------------------------------------------------------------------------------------
inline int write_floats(hipStream_t s, float *dev, const std::vector<float> &t) {
    HIP_TRY(hipMemcpyAsync(dev, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    return FMHIP_OK;
}

inline int write_vector(hipStream_t s, float *dev, const double *src, size_t n) { return write_floats(s, dev, std::vector<float>(src, src + n)); }

inline int read_floats(hipStream_t s, const float *dev, size_t n, std::vector<float> &t) {
    t.resize(n);
    HIP_TRY(hipMemcpyAsync(t.data(), dev, n * sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return FMHIP_OK;
}

// n floats of the device as doubles; stride > width: the first `width` of every `stride` (a factor table)
inline int read_vector(hipStream_t s, const float *dev, size_t n, double *out, int width = 1, int stride = 1) {
    std::vector<float> t;
    TRY(read_floats(s, dev, n, t));
    for (size_t j = 0; j < n / stride; ++j)
        for (int d = 0; d < width; ++d) out[j * width + d] = t[j * stride + d];
    return FMHIP_OK;
}

inline int read_stats(hipStream_t s, const double *dev, int64_t nnz, int64_t steps, fmhip_stats *st) {
    double h[4];
    HIP_TRY(hipMemcpyAsync(h, dev, sizeof h, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    memset(st, 0, sizeof *st);
    fill_stats(st, h);
    st->nnz = nnz;
    st->steps = steps;
    return FMHIP_OK;
}

inline bool rate_ok(double x) { return std::isfinite(x) && x >= 0.0; }

inline int check_order(const int64_t *order, int64_t nb) {
    if (order)
        for (int64_t j = 0; j < nb; ++j)
            if (order[j] < 0 || order[j] >= nb)
                return fail(FMHIP_ERR_INVALID, "order[%lld] = %lld: the dataset has %lld batches", (long long)j, (long long)order[j], (long long)nb);
    return FMHIP_OK;
}

// the caller's stream, or one of the handle's own
template <class M>
int open_stream(M *m, void *stream) {
    if (stream) {
        m->stream = reinterpret_cast<hipStream_t>(stream);
        return FMHIP_OK;
    }
    hipError_t e = hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking);
    if (e != hipSuccess) return fail(FMHIP_ERR_HIP, "hipStreamCreate failed: %s", hipGetErrorString(e));
    m->own_stream = true;
    return FMHIP_OK;
}

template <class M>
int destroy_model(M *m) {
    if (!m) return FMHIP_OK;
    (void)hipSetDevice(m->device);
    if (m->stream) (void)hipStreamSynchronize(m->stream);
    if (m->own_stream && m->stream) (void)hipStreamDestroy(m->stream);
    delete m;
    return FMHIP_OK;
}

// ---- the five handles' common state -----------------------------------------------------------------------------------------------
// how a model is called in messages: "DCN", its macros' FMHIP_<DCN>_, its functions' fmhip_<dcn>_, its own regulariser
struct FieldNames {
    const char *model, *macro, *lower, *reg;
};

struct Rates {
    double eta, reg0, regw, regv, regx;          // regx: the regulariser of the model's own array
};

struct FieldCore {
    std::mutex mu;
    int device = 0;
    int64_t n = 0, n1 = 0;
    int32_t F = 0, k = 0, Kp = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    DevBuf<float> V, w, w0, NV, Nw, N0;
    int loss = FMHIP_LOSS_SQUARED, opt = FMHIP_OPT_SGD, linear = 1, train = 1;          // train: the model's own array is stepped
    double eps = 0.0, init = 0.0;
    // workspace, grown to the largest dataset the model has been paired with
    DevBuf<float> yhat, e, dz, part;
    DevBuf<double> bsum, stats, acc;
    size_t vfloats() const { return (size_t)n1 * Kp; }
    int32_t Fp() const { return round16(F); }
};

// ---- create ----------------------------------------------------------------------------------------------------------------------
// the refusals every create opens with; the model's own follow, then check_feature_ids
inline int check_field_shape(const FieldNames &nm, void *out, int64_t num_attribute, int32_t num_fields, int32_t num_factor, int max_factors) {
    if (!out) return fail(FMHIP_ERR_INVALID, "out is NULL");
    *static_cast<void **>(out) = nullptr;
    if (num_attribute < 0) return fail(FMHIP_ERR_INVALID, "num_attribute = %lld: a model has at least feature 0", (long long)num_attribute);
    if (num_fields < 1) return fail(FMHIP_ERR_INVALID, "num_fields = %d: a model has at least one field", num_fields);
    if (num_fields > kFfmMaxFields) return fail(FMHIP_ERR_UNSUPPORTED, "num_fields = %d is above FMHIP_%s_MAX_FIELDS = %d", num_fields, nm.macro, kFfmMaxFields);
    if (num_factor < 1) return fail(FMHIP_ERR_INVALID, "num_factor = %d: a model has at least one factor", num_factor);
    if (num_factor > max_factors)
        return fail(FMHIP_ERR_UNSUPPORTED, "num_factor = %d is above FMHIP_%s_MAX_FACTORS = %d", num_factor, nm.macro, max_factors);
    return FMHIP_OK;
}

inline int check_feature_ids(int64_t num_attribute) {
    if (num_attribute >= INT32_MAX) return fail(FMHIP_ERR_UNSUPPORTED, "num_attribute = %lld: feature ids are 32-bit", (long long)num_attribute);
    return FMHIP_OK;
}

inline void set_shape(FieldCore &m, int device, int64_t num_attribute, int32_t num_fields, int32_t num_factor) {
    m.device = device;
    m.n = num_attribute;
    m.n1 = num_attribute + 1;
    m.F = num_fields;
    m.k = num_factor;
    m.Kp = field_kp(num_factor);
}

// the stream, the parameters and the statistics of a new handle: V = w = w0 = 0, X (the model's own array) = x0, or 0 without one
inline int open_model(FieldCore &m, const FieldNames &nm, void *stream, DevBuf<float> &X, size_t xfloats, const float *x0) {
    TRY(open_stream(&m, stream));
    TRY(m.V.alloc(m.vfloats()));
    TRY(m.w.alloc((size_t)m.n1));
    TRY(m.w0.alloc(1));
    TRY(X.alloc(xfloats));
    TRY(m.stats.alloc(4));
    TRY(m.acc.alloc(4));
    hipError_t e = hipMemset(m.V.p, 0, m.V.n * sizeof(float));
    if (e == hipSuccess) e = hipMemset(m.w.p, 0, m.w.n * sizeof(float));
    if (e == hipSuccess) e = hipMemset(m.w0.p, 0, sizeof(float));
    if (e == hipSuccess) e = x0 ? hipMemcpy(X.p, x0, xfloats * sizeof(float), hipMemcpyHostToDevice) : hipMemset(X.p, 0, xfloats * sizeof(float));
    if (e == hipSuccess) e = hipMemset(m.stats.p, 0, 4 * sizeof(double));
    if (e == hipSuccess) e = hipMemset(m.acc.p, 0, 4 * sizeof(double));
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return fail(FMHIP_ERR_HIP, "setting up the %s model failed: %s", nm.model, hipGetErrorString(e));
    return FMHIP_OK;
}

inline void model_info(const FieldCore &m, int64_t *num_attribute, int32_t *num_fields, int32_t *num_factor, int32_t *padded_factors) {
    if (num_attribute) *num_attribute = m.n;
    if (num_fields) *num_fields = m.F;
    if (num_factor) *num_factor = m.k;
    if (padded_factors) *padded_factors = m.Kp;
}

// ---- the rule --------------------------------------------------------------------------------------------------------------------
// NX: the accumulator of the model's own array, xfloats long
inline int set_rule(FieldCore &m, int loss, int optimizer, double eps, double init, DevBuf<float> &NX, size_t xfloats) {
    if (loss != FMHIP_LOSS_SQUARED && loss != FMHIP_LOSS_LOGISTIC) return fail(FMHIP_ERR_INVALID, "loss = %d: FMHIP_LOSS_SQUARED or FMHIP_LOSS_LOGISTIC", loss);
    if (optimizer != FMHIP_OPT_SGD && optimizer != FMHIP_OPT_ADAGRAD)
        return fail(FMHIP_ERR_INVALID, "optimizer = %d: FMHIP_OPT_SGD or FMHIP_OPT_ADAGRAD", optimizer);
    if (optimizer == FMHIP_OPT_ADAGRAD) {
        if (!(std::isfinite(eps) && eps > 0.0)) return fail(FMHIP_ERR_INVALID, "eps = %g: AdaGrad's eps is finite and > 0", eps);
        if (!rate_ok(init)) return fail(FMHIP_ERR_INVALID, "init = %g: AdaGrad's initial accumulator is finite and >= 0", init);
    }
    std::lock_guard<std::mutex> lock(m.mu);
    TRY(set_device(m.device));
    m.loss = loss;
    if (optimizer == FMHIP_OPT_SGD) {
        HIP_TRY(hipStreamSynchronize(m.stream));
        m.NV.release();
        m.Nw.release();
        m.N0.release();
        NX.release();
        m.opt = FMHIP_OPT_SGD;
        return FMHIP_OK;
    }
    // the same (eps, init) again keeps the accumulators as they are
    if (m.opt == FMHIP_OPT_ADAGRAD && memcmp(&m.eps, &eps, sizeof eps) == 0 && memcmp(&m.init, &init, sizeof init) == 0) return FMHIP_OK;
    HIP_TRY(hipStreamSynchronize(m.stream));
    TRY(m.NV.alloc(m.vfloats()));
    TRY(m.Nw.alloc((size_t)m.n1));
    TRY(m.N0.alloc(1));
    TRY(NX.alloc(xfloats));
    const std::vector<float> fill(std::max({m.vfloats(), (size_t)m.n1, xfloats}), (float)init);
    HIP_TRY(hipMemcpy(m.NV.p, fill.data(), m.vfloats() * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(m.Nw.p, fill.data(), (size_t)m.n1 * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(m.N0.p, fill.data(), sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(NX.p, fill.data(), xfloats * sizeof(float), hipMemcpyHostToDevice));
    m.opt = FMHIP_OPT_ADAGRAD;
    m.eps = eps;
    m.init = init;
    return FMHIP_OK;
}

// linear, train: 0 or 1
inline int set_flag(FieldCore &m, int FieldCore::*flag, const char *name, int value) {
    if (value != 0 && value != 1) return fail(FMHIP_ERR_INVALID, "%s = %d: 0 or 1", name, value);
    std::lock_guard<std::mutex> lock(m.mu);
    m.*flag = value;
    return FMHIP_OK;
}

// ---- parameters and accumulators -------------------------------------------------------------------------------------------------
// the table codec: the caller's `vecs` vectors of k doubles <-> the device's [vecs][Kp] fp32 (pad slots: `pad`)
inline std::vector<float> pack_table(size_t vecs, int k, int Kp, const double *v, float pad) {
    std::vector<float> t(vecs * Kp, pad);
    for (size_t j = 0; j < vecs; ++j)
        for (int d = 0; d < k; ++d) t[j * Kp + d] = (float)v[j * k + d];
    return t;
}

// src(array, layer) of a call that sets every array: -1, or the first layer one of whose arrays is NULL
template <class Map, class Src>
int first_null_layer(const Map &map, Src src) {
    int bad = -1;
    map.each([&](int a, int l, size_t, size_t) {
        if (bad < 0 && !src(a, l)) bad = l;
    });
    return bad;
}

// V, w, the model's own array (X, through its slot map), w0
template <class Map, class Src>
int write_params(FieldCore &m, float *V, float *w, float *w0, float *X, float pad, double x0, const double *xw, const double *xv, const Map &map, Src src) {
    TRY(set_device(m.device));
    TRY(write_floats(m.stream, V, pack_table((size_t)m.n1, m.k, m.Kp, xv, pad)));
    TRY(write_vector(m.stream, w, xw, (size_t)m.n1));
    TRY(write_floats(m.stream, X, pack_slots(map, src, pad)));
    return write_vector(m.stream, w0, &x0, 1);
}

// every one nullable; any_x: the caller wants some array of the model's own (dst(array, layer): where to, or NULL)
template <class Map, class Dst>
int read_params(FieldCore &m, const float *V, const float *w, const float *w0, const float *X, double *x0, double *xw, double *xv, const Map &map,
                bool any_x, Dst dst) {
    TRY(set_device(m.device));
    if (x0) TRY(read_vector(m.stream, w0, 1, x0));
    if (xw) TRY(read_vector(m.stream, w, (size_t)m.n1, xw));
    if (xv) TRY(read_vector(m.stream, V, m.vfloats(), xv, m.k, m.Kp));
    if (!any_x) return FMHIP_OK;
    std::vector<float> t;
    TRY(read_floats(m.stream, X, map.total(), t));
    unpack_slots(map, t.data(), dst);
    return FMHIP_OK;
}

template <class Map, class Src>
int set_params(FieldCore &m, double w0, const double *w, const double *v, float *X, const Map &map, Src src) {
    std::lock_guard<std::mutex> lock(m.mu);
    return write_params(m, m.V.p, m.w.p, m.w0.p, X, 0.f, w0, w, v, map, src);
}

template <class Map, class Dst>
int get_params(FieldCore &m, double *w0, double *w, double *v, const float *X, const Map &map, bool any_x, Dst dst) {
    std::lock_guard<std::mutex> lock(m.mu);
    return read_params(m, m.V.p, m.w.p, m.w0.p, X, w0, w, v, map, any_x, dst);
}

inline int check_adagrad(const FieldCore &m, const FieldNames &nm) {
    if (m.opt != FMHIP_OPT_ADAGRAD) return fail(FMHIP_ERR_INVALID, "the model is under SGD: it has no accumulators (fmhip_%s_model_set_rule)", nm.lower);
    return FMHIP_OK;
}

template <class Map, class Dst>
int get_accumulators(FieldCore &m, const FieldNames &nm, double *n0, double *nw, double *nv, const float *NX, const Map &map, bool any_x, Dst dst) {
    std::lock_guard<std::mutex> lock(m.mu);
    TRY(check_adagrad(m, nm));
    return read_params(m, m.NV.p, m.Nw.p, m.N0.p, NX, n0, nw, nv, map, any_x, dst);
}

inline int no_check() { return FMHIP_OK; }

// own(): the model's own refusal of valid accumulators (FwFM: symmetric, FmFM: mirrored)
template <class Map, class Src, class Own = int (*)()>
int set_accumulators(FieldCore &m, const FieldNames &nm, double n0, const double *nw, const double *nv, float *NX, const Map &map, Src src, Own own = no_check) {
    std::lock_guard<std::mutex> lock(m.mu);
    TRY(check_adagrad(m, nm));
    if (!rate_ok(n0)) return fail(FMHIP_ERR_INVALID, "n0 = %g: an accumulator is finite and >= 0", n0);
    for (int64_t i = 0; i < m.n1; ++i)
        if (!rate_ok(nw[i])) return fail(FMHIP_ERR_INVALID, "nw[%lld] = %g: an accumulator is finite and >= 0", (long long)i, nw[i]);
    for (size_t j = 0; j < (size_t)m.n1 * m.k; ++j)
        if (!rate_ok(nv[j])) return fail(FMHIP_ERR_INVALID, "nv[%zu] = %g: an accumulator is finite and >= 0", j, nv[j]);
    int rc = FMHIP_OK;
    map.each([&](int a, int l, size_t i, size_t) {
        const double x = src(a, l)[i];
        if (rc != FMHIP_OK || rate_ok(x)) return;
        rc = a < Map::kLayered ? fail(FMHIP_ERR_INVALID, "n%s[%d][%zu] = %g: an accumulator is finite and >= 0", Map::name(a), l, i, x)
                               : fail(FMHIP_ERR_INVALID, "n%s[%zu] = %g: an accumulator is finite and >= 0", Map::name(a), i, x);
    });
    TRY(rc);
    TRY(own());
    return write_params(m, m.NV.p, m.Nw.p, m.N0.p, NX, (float)m.init, n0, nw, nv, map, src);
}

// ---- a model and a dataset --------------------------------------------------------------------------------------------------------
// the refusals of (m, d) that need no launch; a model's own follow, then pair_workspace
inline int pair_refusals(const FieldCore &m, fmhip_ffm_dataset_t d, bool train) {
    if (!d) return fail(FMHIP_ERR_INVALID, "the FFM dataset handle is NULL");
    if (d->device != m.device) return fail(FMHIP_ERR_INVALID, "the dataset lives on device %d, the model on device %d", d->device, m.device);
    if (d->nnz > 0 && d->dim > m.n)
        return fail(FMHIP_ERR_INVALID, "the dataset holds feature id %d, above the model's num_attribute = %lld", d->dim, (long long)m.n);
    if (d->fields > m.F) return fail(FMHIP_ERR_INVALID, "the dataset holds field id %d, outside the model's [0, %d)", d->fields - 1, m.F);
    if (train && !d->labels) return fail(FMHIP_ERR_INVALID, "the dataset was created without labels (y = NULL): it can be scored, not trained on");
    return FMHIP_OK;
}

// the device, and the workspace every model has; blocks: the model's forward workgroups over d->max_rows rows
inline int pair_workspace(FieldCore &m, fmhip_ffm_dataset_t d, bool train, size_t blocks) {
    TRY(set_device(m.device));
    TRY(m.yhat.ensure((size_t)std::max<int64_t>(train ? d->max_rows : d->n_rows, 1)));
    if (train) {
        int32_t max_nnz = 1;
        for (const FfmBatch &b : d->batches) max_nnz = std::max(max_nnz, b.nnz);
        TRY(m.e.ensure((size_t)std::max<int64_t>(d->max_rows, 1)));
        TRY(m.dz.ensure((size_t)max_nnz * m.Kp));
        TRY(m.bsum.ensure(std::max<size_t>(blocks, 1) * 4));
        TRY(m.part.ensure((size_t)std::max(d->max_chunks, 1) * (m.Kp + kFwfmPartTail)));
    }
    return FMHIP_OK;
}

// what fm_fwfm.hip's launches are given of (m, d, batch b): everything but r, Nr, rpart and train_r, the model's own
inline FwfmArgs fwfm_args(const FieldCore &m, fmhip_ffm_dataset_t d, const FfmBatch &b, int32_t n_blocks) {
    FwfmArgs a{};
    a.V = m.V.p;
    a.w = m.w.p;
    a.w0 = m.w0.p;
    a.NV = m.NV.p;
    a.Nw = m.Nw.p;
    a.N0 = m.N0.p;
    a.F = m.F;
    a.Fp = m.Fp();
    a.Kp = m.Kp;
    a.row_ptr = d->row_ptr.p + b.row0;
    a.col = d->col.p;
    a.fld = d->fld.p;
    a.run = d->run.p;
    a.val = d->val.p;
    a.y = d->labels ? d->y.p + b.row0 : nullptr;
    a.nnz0 = b.nnz0;
    a.rows = (int32_t)b.rows;
    a.cfeat = d->cfeat.p + b.col_off;
    a.cptr = d->cptr.p + b.cptr_off;
    a.chunk0 = d->chunk0.p + b.cptr_off;
    a.chunk_col = d->chunk_col.p + b.chunk_off;
    a.occ_row = d->occ_row.p + b.nnz0;
    a.occ_pos = d->occ_pos.p + b.nnz0;
    a.n_cols = b.n_cols;
    a.n_chunks = b.n_chunks;
    a.yhat = m.yhat.p;
    a.e = m.e.p;
    a.dz = m.dz.p;
    a.bsum = m.bsum.p;
    a.n_blocks = n_blocks;
    a.part = m.part.p;
    a.stats = m.stats.p;
    a.loss = m.loss;
    a.linear = m.linear;
    a.eps = (float)m.eps;
    a.invb = b.rows > 0 ? 1.0f / (float)b.rows : 0.f;
    return a;
}

// ... and of a training step (the model's own regulariser goes where its kernels read it)
inline void set_rates(FwfmArgs &a, const Rates &q, double *acc, bool acc_reset) {
    a.eta = (float)q.eta;
    a.reg0 = (float)q.reg0;
    a.regw = (float)q.regw;
    a.regv = (float)q.regv;
    a.acc = acc;
    a.acc_reset = acc_reset;
}

inline int check_rates(const FieldNames &nm, const Rates &q) {
    if (!std::isfinite(q.eta) || !rate_ok(q.reg0) || !rate_ok(q.regw) || !rate_ok(q.regv) || !rate_ok(q.regx))
        return fail(FMHIP_ERR_INVALID, "eta = %g, reg0 = %g, regw = %g, regv = %g, %s = %g: the step size is finite, a regulariser finite and >= 0", q.eta,
                    q.reg0, q.regw, q.regv, nm.reg, q.regx);
    return FMHIP_OK;
}

// ---- predict, step, epoch ----------------------------------------------------------------------------------------------------------
// pair(m, d, train): the model's pair_up; forward(m, d, batch, yhat): its scoring launch, the batch's margins to yhat
template <class M, class Pair, class Forward>
int predict(M *m, fmhip_ffm_dataset_t d, double *yhat, Pair pair, Forward forward) {
    if (!d) return fail(FMHIP_ERR_INVALID, "the FFM dataset handle is NULL");
    if (!yhat) return fail(FMHIP_ERR_INVALID, "yhat is NULL");
    std::lock_guard<std::mutex> lock(m->mu);
    TRY(pair(m, d, false));
    for (const FfmBatch &b : d->batches) HIP_TRY(forward(m, d, b, m->yhat.p + b.row0));
    std::vector<float> h((size_t)d->n_rows);
    if (d->n_rows > 0) HIP_TRY(hipMemcpyAsync(h.data(), m->yhat.p, h.size() * sizeof(float), hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    std::copy(h.begin(), h.end(), yhat);
    return FMHIP_OK;
}

// one(m, d, batch id, q, acc, acc_reset): the model's launch sequence of one step, asynchronous on its stream; acc: the epoch's running
// sums on the device (nullable)
template <class M, class Pair, class One>
int step(M *m, const FieldNames &nm, fmhip_ffm_dataset_t d, int64_t batch, const Rates &q, fmhip_stats *stats, Pair pair, One one) {
    if (!d) return fail(FMHIP_ERR_INVALID, "the FFM dataset handle is NULL");
    TRY(check_rates(nm, q));
    std::lock_guard<std::mutex> lock(m->mu);
    if (batch < 0 || batch >= (int64_t)d->batches.size())
        return fail(FMHIP_ERR_INVALID, "batch = %lld: the dataset has %zu batches", (long long)batch, d->batches.size());
    TRY(pair(m, d, true));
    TRY(one(m, d, batch, q, nullptr, false));
    if (stats) TRY(read_stats(m->stream, m->stats.p, d->batches[(size_t)batch].nnz, 1, stats));
    return FMHIP_OK;
}

template <class M, class Pair, class One>
int epoch(M *m, const FieldNames &nm, fmhip_ffm_dataset_t d, const Rates &q, const int64_t *order, fmhip_stats *stats, Pair pair, One one) {
    if (!d) return fail(FMHIP_ERR_INVALID, "the FFM dataset handle is NULL");
    TRY(check_rates(nm, q));
    std::lock_guard<std::mutex> lock(m->mu);
    const int64_t nb = (int64_t)d->batches.size();
    TRY(check_order(order, nb));
    TRY(pair(m, d, true));
    // the epoch's sums: the first step's update launch overwrites them, the others add
    for (int64_t j = 0; j < nb; ++j) TRY(one(m, d, order ? order[j] : j, q, m->acc.p, j == 0));
    if (stats) TRY(read_stats(m->stream, m->acc.p, d->nnz, nb, stats));
    return FMHIP_OK;
}

}  // namespace host
}  // namespace fmhip
