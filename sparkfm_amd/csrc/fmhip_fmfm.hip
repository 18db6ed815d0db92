// fmhip_fmfm.hip — the C ABI of the field-matrixed FM (include/fmhip_fmfm.h): the model handle, the refusals, and the launch sequence
// of a step — fm_fmfm.hip's forward, its gradient product, fm_fwfm.hip's backward and update for v, w, w0 and the statistics, then
// M's own update.  The data handle is the FFM's (fmhip_ffm_dataset.h), read and never changed.
#include "../../include/fmhip_fmfm.h"
#include "fm_fmfm.h"
#include "fmhip_ffm_dataset.h"
#include "fmhip_internal.h"

#include <algorithm>
#include <cmath>
#include <mutex>
#include <new>
#include <vector>

using namespace fmhip;
using namespace fmhip::host;

static_assert(FMHIP_FMFM_MAX_FIELDS == kFfmMaxFields, "fmhip_fmfm.h and fmhip_host.h disagree on the fields");
static_assert(FMHIP_FMFM_MAX_WIDTH == kFmfmMaxWidth, "fmhip_fmfm.h and fm_fmfm.h disagree on the width");
static_assert(kFwfmChunkLen == kFfmChunk, "fm_fwfm.h and fmhip_host.h disagree on the chunk length");

struct fmhip_fmfm_model {
    template <typename T> using DevBuf = fmhip::host::DevBuf<T>;
    std::mutex mu;
    int device = 0;
    int64_t n = 0, n1 = 0;
    int32_t F = 0, k = 0, Kp = 0, Pp = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    DevBuf<float> V, w, w0, MM, NV, Nw, N0, NM;
    int loss = FMHIP_LOSS_SQUARED, opt = FMHIP_OPT_SGD, linear = 1, train_m = 1;
    double eps = 0.0, init = 0.0;
    // workspace, grown to the largest dataset the model has been paired with
    DevBuf<float> yhat, e, dz, part, sw, mpart;
    DevBuf<double> bsum, stats, acc;
    size_t vfloats() const { return (size_t)n1 * Kp; }
    size_t mfloats() const { return (size_t)Pp * Pp; }
    size_t mdoubles() const { return (size_t)F * F * k * k; }
    size_t at(int f, int g, int d, int d2) const { return (((size_t)f * F + g) * k + d) * k + d2; }           // the caller's m
    size_t dev_at(int f, int g, int d, int d2) const { return ((size_t)f * Kp + d) * Pp + (size_t)g * Kp + d2; }
};

namespace {

// the table codec: the caller's v[i k + d] <-> the device's [i][Kp] fp32 (pad slots: `pad`)
std::vector<float> pack_table(const fmhip_fmfm_model *m, const double *v, float pad) {
    std::vector<float> t(m->vfloats(), pad);
    for (size_t j = 0; j < (size_t)m->n1; ++j)
        for (int d = 0; d < m->k; ++d) t[j * m->Kp + d] = (float)v[j * m->k + d];
    return t;
}

// the caller's m[f][g][d][d'] <-> the device's MM[Pp][Pp] (pad slots: `pad`)
std::vector<float> pack_matrix(const fmhip_fmfm_model *m, const double *mm, float pad) {
    std::vector<float> t(m->mfloats(), pad);
    for (int f = 0; f < m->F; ++f)
        for (int g = 0; g < m->F; ++g)
            for (int d = 0; d < m->k; ++d)
                for (int d2 = 0; d2 < m->k; ++d2) t[m->dev_at(f, g, d, d2)] = (float)mm[m->at(f, g, d, d2)];
    return t;
}

int write_floats(fmhip_fmfm_model *m, float *dev, const std::vector<float> &t) {
    HIP_TRY(hipMemcpyAsync(dev, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    return FMHIP_OK;
}

int write_vector(fmhip_fmfm_model *m, float *dev, const double *src, size_t n) { return write_floats(m, dev, std::vector<float>(src, src + n)); }

// n floats of the device as doubles; stride > width: the first `width` of every `stride` (the factor table)
int read_vector(fmhip_fmfm_model *m, const float *dev, size_t n, double *out, int width = 1, int stride = 1) {
    std::vector<float> t(n);
    HIP_TRY(hipMemcpyAsync(t.data(), dev, n * sizeof(float), hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    for (size_t j = 0; j < n / stride; ++j)
        for (int d = 0; d < width; ++d) out[j * width + d] = t[j * stride + d];
    return FMHIP_OK;
}

int read_matrix(fmhip_fmfm_model *m, const float *dev, double *out) {
    std::vector<float> t(m->mfloats());
    HIP_TRY(hipMemcpyAsync(t.data(), dev, t.size() * sizeof(float), hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    for (int f = 0; f < m->F; ++f)
        for (int g = 0; g < m->F; ++g)
            for (int d = 0; d < m->k; ++d)
                for (int d2 = 0; d2 < m->k; ++d2) out[m->at(f, g, d, d2)] = t[m->dev_at(f, g, d, d2)];
    return FMHIP_OK;
}

// M[g][f] == M[f][g]^T as fp32; with `diagonal` also M[f][f] == 0
int check_mirrored(const fmhip_fmfm_model *m, const double *mm, const char *name, bool diagonal) {
    for (int f = 0; f < m->F; ++f)
        for (int g = f; g < m->F; ++g)
            for (int d = 0; d < m->k; ++d)
                for (int d2 = 0; d2 < m->k; ++d2) {
                    const double x = mm[m->at(f, g, d, d2)], y = mm[m->at(g, f, d2, d)];
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
    if (!d) return fail(FMHIP_ERR_INVALID, "the FFM dataset handle is NULL");
    if (d->device != m->device) return fail(FMHIP_ERR_INVALID, "the dataset lives on device %d, the model on device %d", d->device, m->device);
    if (d->nnz > 0 && d->dim > m->n)
        return fail(FMHIP_ERR_INVALID, "the dataset holds feature id %d, above the model's num_attribute = %lld", d->dim, (long long)m->n);
    if (d->fields > m->F) return fail(FMHIP_ERR_INVALID, "the dataset holds field id %d, outside the model's [0, %d)", d->fields - 1, m->F);
    if (train && !d->labels) return fail(FMHIP_ERR_INVALID, "the dataset was created without labels (y = NULL): it can be scored, not trained on");
    TRY(set_device(m->device));
    TRY(m->yhat.ensure((size_t)std::max<int64_t>(train ? d->max_rows : d->n_rows, 1)));
    if (train) {
        int32_t max_nnz = 1;
        for (const FfmBatch &b : d->batches) max_nnz = std::max(max_nnz, b.nnz);
        const size_t rows = (size_t)std::max<int64_t>(d->max_rows, 1);
        TRY(m->e.ensure(rows));
        TRY(m->dz.ensure((size_t)max_nnz * m->Kp));
        TRY(m->bsum.ensure((size_t)fmfm_forward_blocks(rows) * 4));
        TRY(m->part.ensure((size_t)std::max(d->max_chunks, 1) * (m->Kp + kFwfmPartTail)));
        TRY(m->sw.ensure(rows * m->Pp));
        TRY(m->mpart.ensure((size_t)fmfm_grad_splits(rows) * m->mfloats()));
    }
    return FMHIP_OK;
}

FmfmArgs batch_args(fmhip_fmfm_model_t m, fmhip_ffm_dataset_t d, const FfmBatch &b) {
    FmfmArgs q{};
    FwfmArgs &a = q.b;
    a.V = m->V.p;
    a.w = m->w.p;
    a.w0 = m->w0.p;
    a.NV = m->NV.p;
    a.Nw = m->Nw.p;
    a.N0 = m->N0.p;
    a.Nr = m->NM.p;               // (the FwFM's update launch wants the pointers; with train_r = 0 it reads neither)
    a.rpart = m->mpart.p;
    a.F = m->F;
    a.Fp = (m->F + 15) / 16 * 16;
    a.Kp = m->Kp;
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
    a.yhat = m->yhat.p;
    a.e = m->e.p;
    a.dz = m->dz.p;
    a.bsum = m->bsum.p;
    a.n_blocks = fmfm_forward_blocks(b.rows);
    a.part = m->part.p;
    a.stats = m->stats.p;
    a.loss = m->loss;
    a.linear = m->linear;
    a.train_r = 0;
    a.eps = (float)m->eps;
    a.invb = b.rows > 0 ? 1.0f / (float)b.rows : 0.f;
    q.MM = m->MM.p;
    q.NM = m->NM.p;
    q.k = m->k;
    q.Pp = m->Pp;
    q.sw = m->sw.p;
    q.mpart = m->mpart.p;
    q.n_splits = fmfm_grad_splits(b.rows);
    q.train_m = m->train_m;
    return q;
}

bool rate_ok(double x) { return std::isfinite(x) && x >= 0.0; }

int check_rates(double eta, double reg0, double regw, double regv, double regm) {
    if (!std::isfinite(eta) || !rate_ok(reg0) || !rate_ok(regw) || !rate_ok(regv) || !rate_ok(regm))
        return fail(FMHIP_ERR_INVALID, "eta = %g, reg0 = %g, regw = %g, regv = %g, regm = %g: the step size is finite, a regulariser finite and >= 0", eta, reg0,
                    regw, regv, regm);
    return FMHIP_OK;
}

struct Rates {
    double eta, reg0, regw, regv, regm;
};

// one step, asynchronous on the model's stream; acc: the epoch's running sums on the device (nullable)
int fmfm_step(fmhip_fmfm_model_t m, fmhip_ffm_dataset_t d, int64_t b, const Rates &q, double *acc, bool acc_reset = false) {
    FmfmArgs a = batch_args(m, d, d->batches[(size_t)b]);
    a.b.eta = (float)q.eta;
    a.b.reg0 = (float)q.reg0;
    a.b.regw = (float)q.regw;
    a.b.regv = (float)q.regv;
    a.regm = (float)q.regm;
    a.b.acc = acc;
    a.b.acc_reset = acc_reset;
    const bool ada = m->opt == FMHIP_OPT_ADAGRAD;
    HIP_TRY(launch_fmfm_forward(a, true, m->stream));
    if (m->train_m) HIP_TRY(launch_fmfm_mgrad(a, m->stream));
    HIP_TRY(launch_fwfm_backward(a.b, ada, m->stream));
    HIP_TRY(launch_fwfm_update(a.b, ada, m->stream));
    if (m->train_m) HIP_TRY(launch_fmfm_mupdate(a, ada, m->stream));
    return FMHIP_OK;
}

int read_stats(fmhip_fmfm_model_t m, const double *dev, int64_t nnz, int64_t steps, fmhip_stats *st) {
    double h[4];
    HIP_TRY(hipMemcpyAsync(h, dev, sizeof h, hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    memset(st, 0, sizeof *st);
    fill_stats(st, h);
    st->nnz = nnz;
    st->steps = steps;
    return FMHIP_OK;
}

}  // namespace

extern "C" {

int fmhip_fmfm_model_create(int device, int64_t num_attribute, int32_t num_fields, int32_t num_factor, void *stream, fmhip_fmfm_model_t *out) {
    if (!out) return fail(FMHIP_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (num_attribute < 0) return fail(FMHIP_ERR_INVALID, "num_attribute = %lld: a model has at least feature 0", (long long)num_attribute);
    if (num_fields < 1) return fail(FMHIP_ERR_INVALID, "num_fields = %d: a model has at least one field", num_fields);
    if (num_fields > FMHIP_FMFM_MAX_FIELDS) return fail(FMHIP_ERR_UNSUPPORTED, "num_fields = %d is above FMHIP_FMFM_MAX_FIELDS = %d", num_fields, FMHIP_FMFM_MAX_FIELDS);
    if (num_factor < 1) return fail(FMHIP_ERR_INVALID, "num_factor = %d: a model has at least one factor", num_factor);
    if (num_factor > FMHIP_FMFM_MAX_FACTORS)
        return fail(FMHIP_ERR_UNSUPPORTED, "num_factor = %d is above FMHIP_FMFM_MAX_FACTORS = %d", num_factor, FMHIP_FMFM_MAX_FACTORS);
    const int32_t Kp = num_factor <= 4 ? 4 : (num_factor <= 8 ? 8 : 16);
    if (num_fields * Kp > FMHIP_FMFM_MAX_WIDTH)
        return fail(FMHIP_ERR_UNSUPPORTED, "num_fields = %d at num_factor = %d (padded to %d): F·Kp = %d is above %d", num_fields, num_factor, Kp, num_fields * Kp,
                    FMHIP_FMFM_MAX_WIDTH);
    if (num_attribute >= INT32_MAX) return fail(FMHIP_ERR_UNSUPPORTED, "num_attribute = %lld: feature ids are 32-bit", (long long)num_attribute);
    TRY(set_device(device));
    fmhip_fmfm_model *m = new (std::nothrow) fmhip_fmfm_model();
    if (!m) return fail(FMHIP_ERR_NOMEM, "out of host memory");
    m->device = device;
    m->n = num_attribute;
    m->n1 = num_attribute + 1;
    m->F = num_fields;
    m->k = num_factor;
    m->Kp = Kp;
    m->Pp = (num_fields * Kp + 15) / 16 * 16;
    if (stream) {
        m->stream = reinterpret_cast<hipStream_t>(stream);
    } else {
        hipError_t e = hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking);
        if (e != hipSuccess) {
            delete m;
            return fail(FMHIP_ERR_HIP, "hipStreamCreate failed: %s", hipGetErrorString(e));
        }
        m->own_stream = true;
    }
    int rc;
    if ((rc = m->V.alloc(m->vfloats())) || (rc = m->w.alloc((size_t)m->n1)) || (rc = m->w0.alloc(1)) || (rc = m->MM.alloc(m->mfloats())) ||
        (rc = m->stats.alloc(4)) || (rc = m->acc.alloc(4))) {
        fmhip_fmfm_model_destroy(m);
        return rc;
    }
    std::vector<float> eye(m->mfloats(), 0.f);
    for (int f = 0; f < m->F; ++f)
        for (int g = 0; g < m->F; ++g)
            for (int d = 0; d < m->k && f != g; ++d) eye[m->dev_at(f, g, d, d)] = 1.f;
    hipError_t e = hipMemset(m->V.p, 0, m->V.n * sizeof(float));
    if (e == hipSuccess) e = hipMemset(m->w.p, 0, m->w.n * sizeof(float));
    if (e == hipSuccess) e = hipMemset(m->w0.p, 0, sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(m->MM.p, eye.data(), eye.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(m->stats.p, 0, 4 * sizeof(double));
    if (e == hipSuccess) e = hipMemset(m->acc.p, 0, 4 * sizeof(double));
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        fmhip_fmfm_model_destroy(m);
        return fail(FMHIP_ERR_HIP, "setting up the FmFM model failed: %s", hipGetErrorString(e));
    }
    *out = m;
    return FMHIP_OK;
}

int fmhip_fmfm_model_destroy(fmhip_fmfm_model_t m) {
    if (!m) return FMHIP_OK;
    (void)hipSetDevice(m->device);
    if (m->stream) (void)hipStreamSynchronize(m->stream);
    if (m->own_stream && m->stream) (void)hipStreamDestroy(m->stream);
    delete m;
    return FMHIP_OK;
}

int fmhip_fmfm_model_info(fmhip_fmfm_model_t m, int64_t *num_attribute, int32_t *num_fields, int32_t *num_factor, int32_t *padded_factors) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the FmFM model handle is NULL");
    if (num_attribute) *num_attribute = m->n;
    if (num_fields) *num_fields = m->F;
    if (num_factor) *num_factor = m->k;
    if (padded_factors) *padded_factors = m->Kp;
    return FMHIP_OK;
}

int fmhip_fmfm_model_set_params(fmhip_fmfm_model_t m, double w0, const double *w, const double *v, const double *mm) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the FmFM model handle is NULL");
    if (!w || !v || !mm) return fail(FMHIP_ERR_INVALID, "NULL argument");
    TRY(check_mirrored(m, mm, "m", true));
    std::lock_guard<std::mutex> lock(m->mu);
    TRY(set_device(m->device));
    TRY(write_floats(m, m->V.p, pack_table(m, v, 0.f)));
    TRY(write_vector(m, m->w.p, w, (size_t)m->n1));
    TRY(write_floats(m, m->MM.p, pack_matrix(m, mm, 0.f)));
    return write_vector(m, m->w0.p, &w0, 1);
}

int fmhip_fmfm_model_get_params(fmhip_fmfm_model_t m, double *w0, double *w, double *v, double *mm) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the FmFM model handle is NULL");
    std::lock_guard<std::mutex> lock(m->mu);
    TRY(set_device(m->device));
    if (w0) TRY(read_vector(m, m->w0.p, 1, w0));
    if (w) TRY(read_vector(m, m->w.p, (size_t)m->n1, w));
    if (v) TRY(read_vector(m, m->V.p, m->vfloats(), v, m->k, m->Kp));
    if (mm) TRY(read_matrix(m, m->MM.p, mm));
    return FMHIP_OK;
}

int fmhip_fmfm_model_set_rule(fmhip_fmfm_model_t m, int loss, int optimizer, double eps, double init) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the FmFM model handle is NULL");
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
        m->NM.release();
        m->opt = FMHIP_OPT_SGD;
        return FMHIP_OK;
    }
    if (m->opt == FMHIP_OPT_ADAGRAD && memcmp(&m->eps, &eps, sizeof eps) == 0 && memcmp(&m->init, &init, sizeof init) == 0) return FMHIP_OK;
    HIP_TRY(hipStreamSynchronize(m->stream));
    TRY(m->NV.alloc(m->vfloats()));
    TRY(m->Nw.alloc((size_t)m->n1));
    TRY(m->N0.alloc(1));
    TRY(m->NM.alloc(m->mfloats()));
    const std::vector<float> fill(std::max({m->vfloats(), (size_t)m->n1, m->mfloats()}), (float)init);
    HIP_TRY(hipMemcpy(m->NV.p, fill.data(), m->vfloats() * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(m->Nw.p, fill.data(), (size_t)m->n1 * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(m->N0.p, fill.data(), sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(m->NM.p, fill.data(), m->mfloats() * sizeof(float), hipMemcpyHostToDevice));
    m->opt = FMHIP_OPT_ADAGRAD;
    m->eps = eps;
    m->init = init;
    return FMHIP_OK;
}

int fmhip_fmfm_model_set_linear(fmhip_fmfm_model_t m, int linear) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the FmFM model handle is NULL");
    if (linear != 0 && linear != 1) return fail(FMHIP_ERR_INVALID, "linear = %d: 0 or 1", linear);
    std::lock_guard<std::mutex> lock(m->mu);
    m->linear = linear;
    return FMHIP_OK;
}

int fmhip_fmfm_model_set_field_matrices(fmhip_fmfm_model_t m, int train) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the FmFM model handle is NULL");
    if (train != 0 && train != 1) return fail(FMHIP_ERR_INVALID, "train = %d: 0 or 1", train);
    std::lock_guard<std::mutex> lock(m->mu);
    m->train_m = train;
    return FMHIP_OK;
}

int fmhip_fmfm_model_get_accumulators(fmhip_fmfm_model_t m, double *n0, double *nw, double *nv, double *nm) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the FmFM model handle is NULL");
    std::lock_guard<std::mutex> lock(m->mu);
    if (m->opt != FMHIP_OPT_ADAGRAD) return fail(FMHIP_ERR_INVALID, "the model is under SGD: it has no accumulators (fmhip_fmfm_model_set_rule)");
    TRY(set_device(m->device));
    if (n0) TRY(read_vector(m, m->N0.p, 1, n0));
    if (nw) TRY(read_vector(m, m->Nw.p, (size_t)m->n1, nw));
    if (nv) TRY(read_vector(m, m->NV.p, m->vfloats(), nv, m->k, m->Kp));
    if (nm) TRY(read_matrix(m, m->NM.p, nm));
    return FMHIP_OK;
}

int fmhip_fmfm_model_set_accumulators(fmhip_fmfm_model_t m, double n0, const double *nw, const double *nv, const double *nm) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the FmFM model handle is NULL");
    if (!nw || !nv || !nm) return fail(FMHIP_ERR_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lock(m->mu);
    if (m->opt != FMHIP_OPT_ADAGRAD) return fail(FMHIP_ERR_INVALID, "the model is under SGD: it has no accumulators (fmhip_fmfm_model_set_rule)");
    if (!rate_ok(n0)) return fail(FMHIP_ERR_INVALID, "n0 = %g: an accumulator is finite and >= 0", n0);
    for (int64_t i = 0; i < m->n1; ++i)
        if (!rate_ok(nw[i])) return fail(FMHIP_ERR_INVALID, "nw[%lld] = %g: an accumulator is finite and >= 0", (long long)i, nw[i]);
    for (size_t j = 0; j < (size_t)m->n1 * m->k; ++j)
        if (!rate_ok(nv[j])) return fail(FMHIP_ERR_INVALID, "nv[%zu] = %g: an accumulator is finite and >= 0", j, nv[j]);
    for (size_t j = 0; j < m->mdoubles(); ++j)
        if (!rate_ok(nm[j])) return fail(FMHIP_ERR_INVALID, "nm[%zu] = %g: an accumulator is finite and >= 0", j, nm[j]);
    TRY(check_mirrored(m, nm, "nm", false));
    TRY(set_device(m->device));
    TRY(write_floats(m, m->NV.p, pack_table(m, nv, (float)m->init)));
    TRY(write_vector(m, m->Nw.p, nw, (size_t)m->n1));
    TRY(write_floats(m, m->NM.p, pack_matrix(m, nm, (float)m->init)));
    return write_vector(m, m->N0.p, &n0, 1);
}

int fmhip_fmfm_predict(fmhip_fmfm_model_t m, fmhip_ffm_dataset_t d, double *yhat) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the FmFM model handle is NULL");
    if (!d) return fail(FMHIP_ERR_INVALID, "the FFM dataset handle is NULL");
    if (!yhat) return fail(FMHIP_ERR_INVALID, "yhat is NULL");
    std::lock_guard<std::mutex> lock(m->mu);
    TRY(pair_up(m, d, false));
    for (const FfmBatch &b : d->batches) {
        FmfmArgs a = batch_args(m, d, b);
        a.b.yhat = m->yhat.p + b.row0;
        HIP_TRY(launch_fmfm_forward(a, false, m->stream));
    }
    std::vector<float> h((size_t)d->n_rows);
    if (d->n_rows > 0) HIP_TRY(hipMemcpyAsync(h.data(), m->yhat.p, h.size() * sizeof(float), hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    std::copy(h.begin(), h.end(), yhat);
    return FMHIP_OK;
}

int fmhip_fmfm_step(fmhip_fmfm_model_t m, fmhip_ffm_dataset_t d, int64_t batch, double eta, double reg0, double regw, double regv, double regm,
                    fmhip_stats *stats) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the FmFM model handle is NULL");
    if (!d) return fail(FMHIP_ERR_INVALID, "the FFM dataset handle is NULL");
    TRY(check_rates(eta, reg0, regw, regv, regm));
    std::lock_guard<std::mutex> lock(m->mu);
    if (batch < 0 || batch >= (int64_t)d->batches.size())
        return fail(FMHIP_ERR_INVALID, "batch = %lld: the dataset has %zu batches", (long long)batch, d->batches.size());
    TRY(pair_up(m, d, true));
    TRY(fmfm_step(m, d, batch, Rates{eta, reg0, regw, regv, regm}, nullptr));
    if (stats) TRY(read_stats(m, m->stats.p, d->batches[(size_t)batch].nnz, 1, stats));
    return FMHIP_OK;
}

int fmhip_fmfm_epoch(fmhip_fmfm_model_t m, fmhip_ffm_dataset_t d, double eta, double reg0, double regw, double regv, double regm,
                     const int64_t *order, fmhip_stats *stats) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the FmFM model handle is NULL");
    if (!d) return fail(FMHIP_ERR_INVALID, "the FFM dataset handle is NULL");
    TRY(check_rates(eta, reg0, regw, regv, regm));
    std::lock_guard<std::mutex> lock(m->mu);
    const int64_t nb = (int64_t)d->batches.size();
    if (order)
        for (int64_t j = 0; j < nb; ++j)
            if (order[j] < 0 || order[j] >= nb) return fail(FMHIP_ERR_INVALID, "order[%lld] = %lld: the dataset has %lld batches", (long long)j, (long long)order[j], (long long)nb);
    TRY(pair_up(m, d, true));
    // the epoch's sums: the first step's update launch overwrites them, the others add
    for (int64_t j = 0; j < nb; ++j) TRY(fmfm_step(m, d, order ? order[j] : j, Rates{eta, reg0, regw, regv, regm}, m->acc.p, j == 0));
    if (stats) TRY(read_stats(m, m->acc.p, d->nnz, nb, stats));
    return FMHIP_OK;
}

}  // extern "C"
