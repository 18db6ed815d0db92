// fmhip_ffm.hip — the C ABI of the field-aware FM (include/fmhip_ffm.h): the model and dataset handles, the refusals, and the launch
// sequence of a step — fm_ffm.hip's three kernels.  The dataset's layout is built on the host (fmhip_host.cpp: ffm_validate, ffm_build).
#include "../../include/fmhip_ffm.h"
#include "fm_ffm.h"
#include "fmhip_field_model.h"

using namespace fmhip;
using namespace fmhip::host;

static_assert(FMHIP_FFM_MAX_FIELDS == kFfmMaxFields && FMHIP_FFM_MAX_FACTORS == kFfmMaxFactors && FMHIP_FFM_MAX_ROW == kFfmMaxRow,
              "fmhip_ffm.h and fmhip_host.h disagree on the limits");
static_assert(kFfmChunkLen == kFfmChunk, "fm_ffm.h and fmhip_host.h disagree on the chunk length");

struct fmhip_ffm_model {
    template <typename T> using DevBuf = fmhip::host::DevBuf<T>;
    std::mutex mu;
    int device = 0;
    int64_t n = 0, n1 = 0;
    int32_t F = 0, k = 0, Kp = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    DevBuf<float> V, w, w0, NV, Nw, N0;
    int loss = FMHIP_LOSS_SQUARED, opt = FMHIP_OPT_SGD, linear = 1;
    double eps = 0.0, init = 0.0;
    // workspace, grown to the largest dataset the model has been paired with (never inside a step of a dataset it already fits)
    DevBuf<float> yhat, e, part;
    DevBuf<double> bsum, stats, acc;
    size_t vfloats() const { return (size_t)n1 * F * Kp; }
};

namespace {

template <typename T>
int upload(DevBuf<T> &buf, const std::vector<T> &h) {
    TRY(buf.alloc(std::max<size_t>(h.size(), 1)));
    if (!h.empty()) HIP_TRY(hipMemcpy(buf.p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return FMHIP_OK;
}

// the table codec: the caller's v[((i F) + f) k + d] <-> the device's [i][f][Kp] fp32 (pad slots: `pad`)
std::vector<float> pack_vectors(const fmhip_ffm_model *m, const double *v, float pad) { return pack_table((size_t)m->n1 * m->F, m->k, m->Kp, v, pad); }

int read_table(fmhip_ffm_model *m, const float *dev, double *v) { return read_vector(m->stream, dev, m->vfloats(), v, m->k, m->Kp); }

// every refusal of (m, d) that needs no launch, then the device and the workspace
int pair_up(fmhip_ffm_model_t m, fmhip_ffm_dataset_t d, bool train) {
    if (!d) return fail(FMHIP_ERR_INVALID, "the FFM dataset handle is NULL");
    if (d->device != m->device) return fail(FMHIP_ERR_INVALID, "the dataset lives on device %d, the model on device %d", d->device, m->device);
    if (d->nnz > 0 && d->dim > m->n)
        return fail(FMHIP_ERR_INVALID, "the dataset holds feature id %d, above the model's num_attribute = %lld", d->dim, (long long)m->n);
    if (d->fields > m->F)
        return fail(FMHIP_ERR_INVALID, "the dataset holds field id %d, outside the model's [0, %d)", d->fields - 1, m->F);
    if (train && !d->labels) return fail(FMHIP_ERR_INVALID, "the dataset was created without labels (y = NULL): it can be scored, not trained on");
    TRY(set_device(m->device));
    TRY(m->yhat.ensure((size_t)std::max<int64_t>(train ? d->max_rows : d->n_rows, 1)));
    if (train) {
        TRY(m->e.ensure((size_t)std::max<int64_t>(d->max_rows, 1)));
        TRY(m->bsum.ensure((size_t)std::max(ffm_forward_blocks(d->max_rows), 1) * 4));
        TRY(m->part.ensure((size_t)std::max(d->max_chunks, 1) * ((size_t)m->F * m->Kp + kFfmPartTail)));
    }
    return FMHIP_OK;
}

FfmArgs batch_args(fmhip_ffm_model_t m, fmhip_ffm_dataset_t d, const FfmBatch &b) {
    FfmArgs a{};
    a.V = m->V.p;
    a.w = m->w.p;
    a.w0 = m->w0.p;
    a.NV = m->NV.p;
    a.Nw = m->Nw.p;
    a.N0 = m->N0.p;
    a.F = m->F;
    a.Kp = m->Kp;
    a.row_ptr = d->row_ptr.p + b.row0;
    a.col = d->col.p;
    a.fld = d->fld.p;
    a.run = d->run.p;
    a.val = d->val.p;
    a.y = d->labels ? d->y.p + b.row0 : nullptr;
    a.rows = (int32_t)b.rows;
    a.max_len = b.max_len;
    a.cfeat = d->cfeat.p + b.col_off;
    a.cptr = d->cptr.p + b.cptr_off;
    a.chunk0 = d->chunk0.p + b.cptr_off;
    a.chunk_col = d->chunk_col.p + b.chunk_off;
    a.occ_row = d->occ_row.p + b.nnz0;
    a.occ_pos = d->occ_pos.p + b.nnz0;
    a.n_cols = b.n_cols;
    a.n_chunks = b.n_chunks;
    a.yhat = m->yhat.p;
    a.e = m->e.p;
    a.bsum = m->bsum.p;
    a.n_blocks = ffm_forward_blocks(b.rows);
    a.part = m->part.p;
    a.stats = m->stats.p;
    a.loss = m->loss;
    a.linear = m->linear;
    a.eps = (float)m->eps;
    a.invb = b.rows > 0 ? 1.0f / (float)b.rows : 0.f;
    return a;
}

int check_rates(double eta, double reg0, double regw, double regv) {
    if (!std::isfinite(eta) || !rate_ok(reg0) || !rate_ok(regw) || !rate_ok(regv))
        return fail(FMHIP_ERR_INVALID, "eta = %g, reg0 = %g, regw = %g, regv = %g: the step size is finite, a regulariser finite and >= 0", eta, reg0, regw, regv);
    return FMHIP_OK;
}

// one step, asynchronous on the model's stream; acc: the epoch's running sums on the device (nullable)
int ffm_step(fmhip_ffm_model_t m, fmhip_ffm_dataset_t d, int64_t b, double eta, double reg0, double regw, double regv, double *acc, bool acc_reset = false) {
    FfmArgs a = batch_args(m, d, d->batches[(size_t)b]);
    a.eta = (float)eta;
    a.reg0 = (float)reg0;
    a.regw = (float)regw;
    a.regv = (float)regv;
    a.acc = acc;
    a.acc_reset = acc_reset;
    HIP_TRY(launch_ffm_forward(a, true, m->stream));
    HIP_TRY(launch_ffm_backward(a, m->stream));
    HIP_TRY(launch_ffm_update(a, m->opt == FMHIP_OPT_ADAGRAD, m->stream));
    return FMHIP_OK;
}

}  // namespace

extern "C" {

int fmhip_ffm_model_create(int device, int64_t num_attribute, int32_t num_fields, int32_t num_factor, void *stream, fmhip_ffm_model_t *out) {
    if (!out) return fail(FMHIP_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (num_attribute < 0) return fail(FMHIP_ERR_INVALID, "num_attribute = %lld: a model has at least feature 0", (long long)num_attribute);
    if (num_fields < 1) return fail(FMHIP_ERR_INVALID, "num_fields = %d: a model has at least one field", num_fields);
    if (num_fields > FMHIP_FFM_MAX_FIELDS) return fail(FMHIP_ERR_UNSUPPORTED, "num_fields = %d is above FMHIP_FFM_MAX_FIELDS = %d", num_fields, FMHIP_FFM_MAX_FIELDS);
    if (num_factor < 1) return fail(FMHIP_ERR_INVALID, "num_factor = %d: a model has at least one factor", num_factor);
    if (num_factor > FMHIP_FFM_MAX_FACTORS)
        return fail(FMHIP_ERR_UNSUPPORTED, "num_factor = %d is above FMHIP_FFM_MAX_FACTORS = %d", num_factor, FMHIP_FFM_MAX_FACTORS);
    if (num_attribute >= INT32_MAX) return fail(FMHIP_ERR_UNSUPPORTED, "num_attribute = %lld: feature ids are 32-bit", (long long)num_attribute);
    TRY(set_device(device));
    fmhip_ffm_model *m = new (std::nothrow) fmhip_ffm_model();
    if (!m) return fail(FMHIP_ERR_NOMEM, "out of host memory");
    m->device = device;
    m->n = num_attribute;
    m->n1 = num_attribute + 1;
    m->F = num_fields;
    m->k = num_factor;
    m->Kp = num_factor <= 4 ? 4 : (num_factor <= 8 ? 8 : 16);
    int rc = open_stream(m, stream);
    if (rc) {
        delete m;
        return rc;
    }
    hipError_t e = hipSuccess;
    if ((rc = m->V.alloc(m->vfloats())) || (rc = m->w.alloc((size_t)m->n1)) || (rc = m->w0.alloc(1)) || (rc = m->stats.alloc(4)) || (rc = m->acc.alloc(4))) {
        fmhip_ffm_model_destroy(m);
        return rc;
    }
    if (e == hipSuccess) e = hipMemset(m->V.p, 0, m->V.n * sizeof(float));
    if (e == hipSuccess) e = hipMemset(m->w.p, 0, m->w.n * sizeof(float));
    if (e == hipSuccess) e = hipMemset(m->w0.p, 0, sizeof(float));
    if (e == hipSuccess) e = hipMemset(m->stats.p, 0, 4 * sizeof(double));
    if (e == hipSuccess) e = hipMemset(m->acc.p, 0, 4 * sizeof(double));
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        fmhip_ffm_model_destroy(m);
        return fail(FMHIP_ERR_HIP, "setting up the FFM model failed: %s", hipGetErrorString(e));
    }
    *out = m;
    return FMHIP_OK;
}

int fmhip_ffm_model_destroy(fmhip_ffm_model_t m) { return destroy_model(m); }

int fmhip_ffm_model_info(fmhip_ffm_model_t m, int64_t *num_attribute, int32_t *num_fields, int32_t *num_factor, int32_t *padded_factors) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the FFM model handle is NULL");
    if (num_attribute) *num_attribute = m->n;
    if (num_fields) *num_fields = m->F;
    if (num_factor) *num_factor = m->k;
    if (padded_factors) *padded_factors = m->Kp;
    return FMHIP_OK;
}

int fmhip_ffm_model_set_params(fmhip_ffm_model_t m, double w0, const double *w, const double *v) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the FFM model handle is NULL");
    if (!w || !v) return fail(FMHIP_ERR_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lock(m->mu);
    TRY(set_device(m->device));
    TRY(write_floats(m->stream, m->V.p, pack_vectors(m, v, 0.f)));
    TRY(write_vector(m->stream, m->w.p, w, (size_t)m->n1));
    return write_vector(m->stream, m->w0.p, &w0, 1);
}

int fmhip_ffm_model_get_params(fmhip_ffm_model_t m, double *w0, double *w, double *v) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the FFM model handle is NULL");
    std::lock_guard<std::mutex> lock(m->mu);
    TRY(set_device(m->device));
    if (w0) TRY(read_vector(m->stream, m->w0.p, 1, w0));
    if (w) TRY(read_vector(m->stream, m->w.p, (size_t)m->n1, w));
    if (v) TRY(read_table(m, m->V.p, v));
    return FMHIP_OK;
}

int fmhip_ffm_model_set_rule(fmhip_ffm_model_t m, int loss, int optimizer, double eps, double init) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the FFM model handle is NULL");
    if (loss != FMHIP_LOSS_SQUARED && loss != FMHIP_LOSS_LOGISTIC) return fail(FMHIP_ERR_INVALID, "loss = %d: FMHIP_LOSS_SQUARED or FMHIP_LOSS_LOGISTIC", loss);
    if (optimizer != FMHIP_OPT_SGD && optimizer != FMHIP_OPT_ADAGRAD)
        return fail(FMHIP_ERR_INVALID, "optimizer = %d: FMHIP_OPT_SGD or FMHIP_OPT_ADAGRAD", optimizer);
    if (optimizer == FMHIP_OPT_ADAGRAD) {
        if (!(std::isfinite(eps) && eps > 0.0)) return fail(FMHIP_ERR_INVALID, "eps = %g: AdaGrad's eps is finite and > 0", eps);
        if (!rate_ok(init)) return fail(FMHIP_ERR_INVALID, "init = %g: AdaGrad's initial accumulator is finite and >= 0", init);
    }
    std::lock_guard<std::mutex> lock(m->mu);
    TRY(set_device(m->device));
    m->loss = loss;
    if (optimizer == FMHIP_OPT_SGD) {
        HIP_TRY(hipStreamSynchronize(m->stream));
        m->NV.release();
        m->Nw.release();
        m->N0.release();
        m->opt = FMHIP_OPT_SGD;
        return FMHIP_OK;
    }
    if (m->opt == FMHIP_OPT_ADAGRAD && memcmp(&m->eps, &eps, sizeof eps) == 0 && memcmp(&m->init, &init, sizeof init) == 0) return FMHIP_OK;
    HIP_TRY(hipStreamSynchronize(m->stream));
    TRY(m->NV.alloc(m->vfloats()));
    TRY(m->Nw.alloc((size_t)m->n1));
    TRY(m->N0.alloc(1));
    const std::vector<float> fill(std::max(m->vfloats(), (size_t)m->n1), (float)init);
    HIP_TRY(hipMemcpy(m->NV.p, fill.data(), m->vfloats() * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(m->Nw.p, fill.data(), (size_t)m->n1 * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(m->N0.p, fill.data(), sizeof(float), hipMemcpyHostToDevice));
    m->opt = FMHIP_OPT_ADAGRAD;
    m->eps = eps;
    m->init = init;
    return FMHIP_OK;
}

int fmhip_ffm_model_set_linear(fmhip_ffm_model_t m, int linear) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the FFM model handle is NULL");
    if (linear != 0 && linear != 1) return fail(FMHIP_ERR_INVALID, "linear = %d: 0 or 1", linear);
    std::lock_guard<std::mutex> lock(m->mu);
    m->linear = linear;
    return FMHIP_OK;
}

int fmhip_ffm_model_get_accumulators(fmhip_ffm_model_t m, double *n0, double *nw, double *nv) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the FFM model handle is NULL");
    std::lock_guard<std::mutex> lock(m->mu);
    if (m->opt != FMHIP_OPT_ADAGRAD) return fail(FMHIP_ERR_INVALID, "the model is under SGD: it has no accumulators (fmhip_ffm_model_set_rule)");
    TRY(set_device(m->device));
    if (n0) TRY(read_vector(m->stream, m->N0.p, 1, n0));
    if (nw) TRY(read_vector(m->stream, m->Nw.p, (size_t)m->n1, nw));
    if (nv) TRY(read_table(m, m->NV.p, nv));
    return FMHIP_OK;
}

int fmhip_ffm_model_set_accumulators(fmhip_ffm_model_t m, double n0, const double *nw, const double *nv) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the FFM model handle is NULL");
    if (!nw || !nv) return fail(FMHIP_ERR_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lock(m->mu);
    if (m->opt != FMHIP_OPT_ADAGRAD) return fail(FMHIP_ERR_INVALID, "the model is under SGD: it has no accumulators (fmhip_ffm_model_set_rule)");
    if (!rate_ok(n0)) return fail(FMHIP_ERR_INVALID, "n0 = %g: an accumulator is finite and >= 0", n0);
    for (int64_t i = 0; i < m->n1; ++i)
        if (!rate_ok(nw[i])) return fail(FMHIP_ERR_INVALID, "nw[%lld] = %g: an accumulator is finite and >= 0", (long long)i, nw[i]);
    const size_t nvals = (size_t)m->n1 * m->F * m->k;
    for (size_t j = 0; j < nvals; ++j)
        if (!rate_ok(nv[j])) return fail(FMHIP_ERR_INVALID, "nv[%zu] = %g: an accumulator is finite and >= 0", j, nv[j]);
    TRY(set_device(m->device));
    TRY(write_floats(m->stream, m->NV.p, pack_vectors(m, nv, (float)m->init)));
    TRY(write_vector(m->stream, m->Nw.p, nw, (size_t)m->n1));
    return write_vector(m->stream, m->N0.p, &n0, 1);
}

int fmhip_ffm_dataset_create(int device, int64_t n_rows, const int64_t *row_ptr, const int32_t *col, const int32_t *field, const double *val,
                             const double *y, int64_t batch_rows, fmhip_ffm_dataset_t *out) {
    if (!out) return fail(FMHIP_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (n_rows < 0) return fail(FMHIP_ERR_INVALID, "n_rows = %lld", (long long)n_rows);
    if (!row_ptr) return fail(FMHIP_ERR_INVALID, "row_ptr is NULL");
    if (n_rows > 0 && row_ptr[n_rows] > 0 && (!col || !field || !val)) return fail(FMHIP_ERR_INVALID, "col, field or val is NULL");
    if (n_rows >= INT32_MAX) return fail(FMHIP_ERR_UNSUPPORTED, "n_rows = %lld: batch-local rows are 32-bit", (long long)n_rows);
    const FfmCheck c = ffm_validate(n_rows, row_ptr, col, field, val);
    switch (c.kind) {
        case kFfmBadRowPtr:
            return c.row == 0 && row_ptr[0] != 0 ? fail(FMHIP_ERR_INVALID, "row_ptr[0] = %lld: it starts at 0", (long long)row_ptr[0])
                                                 : fail(FMHIP_ERR_INVALID, "row_ptr decreases at row %lld", (long long)c.row);
        case kFfmRowTooLong:
            return fail(FMHIP_ERR_UNSUPPORTED, "row %lld has %lld entries, above FMHIP_FFM_MAX_ROW = %d", (long long)c.row,
                        (long long)(row_ptr[c.row + 1] - row_ptr[c.row]), FMHIP_FFM_MAX_ROW);
        case kFfmBadFeature: return fail(FMHIP_ERR_INVALID, "row %lld holds feature id %d: ids are >= 0", (long long)c.row, col[c.entry]);
        case kFfmBadField:
            return fail(FMHIP_ERR_INVALID, "row %lld holds field id %d, outside [0, %d)", (long long)c.row, field[c.entry], FMHIP_FFM_MAX_FIELDS);
        case kFfmBadValue: return fail(FMHIP_ERR_INVALID, "row %lld holds the value %g for feature %d: values are finite as fp32", (long long)c.row, val[c.entry], col[c.entry]);
        case kFfmDupFeature: return fail(FMHIP_ERR_INVALID, "row %lld holds feature id %d twice", (long long)c.row, col[c.entry]);
        default: break;
    }
    const int64_t nnz = n_rows > 0 ? row_ptr[n_rows] : 0;
    // a batch's occurrence offsets are 32-bit
    for (int64_t br = batch_rows > 0 && batch_rows < n_rows ? batch_rows : n_rows, r0 = 0; r0 < n_rows; r0 += br) {
        const int64_t bn = row_ptr[std::min(r0 + br, n_rows)] - row_ptr[r0];
        if (bn >= INT32_MAX)
            return fail(FMHIP_ERR_UNSUPPORTED, "the batch at row %lld holds %lld entries: a batch's occurrence offsets are 32-bit (lower batch_rows)", (long long)r0, (long long)bn);
    }
    if (y)
        for (int64_t r = 0; r < n_rows; ++r)
            if (!std::isfinite((float)y[r])) return fail(FMHIP_ERR_INVALID, "y[%lld] = %g: labels are finite as fp32", (long long)r, y[r]);
    TRY(set_device(device));
    fmhip_ffm_dataset *d = new (std::nothrow) fmhip_ffm_dataset();
    if (!d) return fail(FMHIP_ERR_NOMEM, "out of host memory");
    FfmLayout L;
    ffm_build(n_rows, row_ptr, col, field, val, batch_rows, kFfmChunk, &L);
    d->device = device;
    d->n_rows = n_rows;
    d->nnz = nnz;
    d->batch_rows = L.batches.empty() ? 0 : L.batches[0].rows;
    d->max_rows = L.max_rows;
    d->dim = c.dim;
    d->fields = c.fields;
    d->max_len = c.max_len;
    d->max_chunks = L.max_chunks;
    d->labels = y != nullptr;
    d->batches = L.batches;
    std::vector<int64_t> rp(row_ptr, row_ptr + n_rows + 1);
    std::vector<float> yf;
    if (y) yf.assign(y, y + n_rows);
    int rc;
    if ((rc = upload(d->row_ptr, rp)) || (rc = upload(d->col, L.col)) || (rc = upload(d->fld, L.field)) || (rc = upload(d->run, L.run)) ||
        (rc = upload(d->val, L.val)) || (rc = upload(d->y, yf)) || (rc = upload(d->cfeat, L.cfeat)) || (rc = upload(d->cptr, L.cptr)) ||
        (rc = upload(d->chunk0, L.chunk0)) || (rc = upload(d->chunk_col, L.chunk_col)) || (rc = upload(d->occ_row, L.occ_row)) ||
        (rc = upload(d->occ_pos, L.occ_pos))) {
        delete d;
        return rc;
    }
    *out = d;
    return FMHIP_OK;
}

int fmhip_ffm_dataset_destroy(fmhip_ffm_dataset_t d) {
    if (!d) return FMHIP_OK;
    (void)hipSetDevice(d->device);
    (void)hipDeviceSynchronize();
    delete d;
    return FMHIP_OK;
}

int fmhip_ffm_dataset_info(fmhip_ffm_dataset_t d, int64_t *n_rows, int64_t *nnz, int64_t *dimension, int32_t *fields, int32_t *max_row,
                           int64_t *batch_rows, int64_t *n_batches) {
    if (!d) return fail(FMHIP_ERR_INVALID, "the FFM dataset handle is NULL");
    if (n_rows) *n_rows = d->n_rows;
    if (nnz) *nnz = d->nnz;
    if (dimension) *dimension = d->dim;
    if (fields) *fields = d->fields;
    if (max_row) *max_row = d->max_len;
    if (batch_rows) *batch_rows = d->batch_rows;
    if (n_batches) *n_batches = (int64_t)d->batches.size();
    return FMHIP_OK;
}

int fmhip_ffm_predict(fmhip_ffm_model_t m, fmhip_ffm_dataset_t d, double *yhat) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the FFM model handle is NULL");
    if (!d) return fail(FMHIP_ERR_INVALID, "the FFM dataset handle is NULL");
    if (!yhat) return fail(FMHIP_ERR_INVALID, "yhat is NULL");
    std::lock_guard<std::mutex> lock(m->mu);
    TRY(pair_up(m, d, false));
    for (const FfmBatch &b : d->batches) {
        FfmArgs a = batch_args(m, d, b);
        a.yhat = m->yhat.p + b.row0;
        HIP_TRY(launch_ffm_forward(a, false, m->stream));
    }
    std::vector<float> h((size_t)d->n_rows);
    if (d->n_rows > 0) HIP_TRY(hipMemcpyAsync(h.data(), m->yhat.p, h.size() * sizeof(float), hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    std::copy(h.begin(), h.end(), yhat);
    return FMHIP_OK;
}

int fmhip_ffm_step(fmhip_ffm_model_t m, fmhip_ffm_dataset_t d, int64_t batch, double eta, double reg0, double regw, double regv, fmhip_stats *stats) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the FFM model handle is NULL");
    if (!d) return fail(FMHIP_ERR_INVALID, "the FFM dataset handle is NULL");
    TRY(check_rates(eta, reg0, regw, regv));
    std::lock_guard<std::mutex> lock(m->mu);
    if (batch < 0 || batch >= (int64_t)d->batches.size())
        return fail(FMHIP_ERR_INVALID, "batch = %lld: the dataset has %zu batches", (long long)batch, d->batches.size());
    TRY(pair_up(m, d, true));
    TRY(ffm_step(m, d, batch, eta, reg0, regw, regv, nullptr));
    if (stats) TRY(read_stats(m->stream, m->stats.p, d->batches[(size_t)batch].nnz, 1, stats));
    return FMHIP_OK;
}

int fmhip_ffm_epoch(fmhip_ffm_model_t m, fmhip_ffm_dataset_t d, double eta, double reg0, double regw, double regv, const int64_t *order,
                    fmhip_stats *stats) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the FFM model handle is NULL");
    if (!d) return fail(FMHIP_ERR_INVALID, "the FFM dataset handle is NULL");
    TRY(check_rates(eta, reg0, regw, regv));
    std::lock_guard<std::mutex> lock(m->mu);
    const int64_t nb = (int64_t)d->batches.size();
    TRY(check_order(order, nb));
    TRY(pair_up(m, d, true));
    // the epoch's sums: the first step's update launch overwrites them, the others add
    for (int64_t j = 0; j < nb; ++j) TRY(ffm_step(m, d, order ? order[j] : j, eta, reg0, regw, regv, m->acc.p, j == 0));
    if (stats) TRY(read_stats(m->stream, m->acc.p, d->nnz, nb, stats));
    return FMHIP_OK;
}

}  // extern "C"
