// fmhip_autoint.hip — the C ABI of AutoInt (include/fmhip_autoint.h): the model handle, the refusals, and the launch sequence of a
// step — fm_autoint.hip's forward (the attention layers forwards and backwards, a row at a time), fm_fwfm.hip's backward and update for
// v, w, w0 and the statistics, then the dense part's own update.  The data handle is the FFM's (fmhip_ffm_dataset.h), read and never
// changed.
#include "../../include/fmhip_autoint.h"
#include "fm_autoint.h"
#include "fmhip_ffm_dataset.h"
#include "fmhip_internal.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

using namespace fmhip;
using namespace fmhip::host;

static_assert(FMHIP_AUTOINT_MAX_FIELDS == kFfmMaxFields, "fmhip_autoint.h and fmhip_host.h disagree on the fields");
static_assert(FMHIP_AUTOINT_MAX_FACTORS == kAutoIntMaxFactors && FMHIP_AUTOINT_MAX_WIDTH == kAutoIntMaxWidth, "fmhip_autoint.h and fm_autoint.h disagree on the widths");
static_assert(FMHIP_AUTOINT_MAX_LAYERS == kAutoIntMaxLayers && FMHIP_AUTOINT_MAX_HEADS == kAutoIntMaxHeads && FMHIP_AUTOINT_MAX_HEAD_DIM == kAutoIntMaxHeadDim,
              "fmhip_autoint.h and fm_autoint.h disagree on the layers");
static_assert(kFwfmChunkLen == kFfmChunk, "fm_fwfm.h and fmhip_host.h disagree on the chunk length");
// the largest accepted model runs inside gfx950's 160 KB of LDS a workgroup may ask for
static_assert(autoint_forward_lds(64, kAutoIntMaxWidth, kAutoIntMaxLayers, true) <= 160 * 1024, "the largest model's row");

struct fmhip_autoint_model {
    template <typename T> using DevBuf = fmhip::host::DevBuf<T>;
    std::mutex mu;
    int device = 0;
    int64_t n = 0, n1 = 0;
    int32_t F = 0, Fp = 0, k = 0, Kp = 0, L = 0, H = 0, d = 0, A = 0;
    int32_t woff[kAutoIntMaxLayers] = {}, hoff = 0, total = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    DevBuf<float> V, w, w0, D, NV, Nw, N0, ND;
    int loss = FMHIP_LOSS_SQUARED, opt = FMHIP_OPT_SGD, linear = 1, train_d = 1;
    double eps = 0.0, init = 0.0;
    // workspace (fm_autoint.h), grown to the largest dataset the model has been paired with
    DevBuf<float> yhat, e, dz, part, scratch, gpart;
    DevBuf<double> bsum, stats, acc;
    size_t vfloats() const { return (size_t)n1 * Kp; }
    int rows_of(int l) const { return l == 0 ? k : A; }               // the caller's D_l
    int stride_of(int l) const { return l == 0 ? kAutoIntD0 : A; }     // ... and the device's
};

namespace {

// the table codec: the caller's v[i k + d] <-> the device's [i][Kp] fp32 (pad slots: `pad`)
std::vector<float> pack_table(const fmhip_autoint_model *m, const double *v, float pad) {
    std::vector<float> t(m->vfloats(), pad);
    for (size_t j = 0; j < (size_t)m->n1; ++j)
        for (int d = 0; d < m->k; ++d) t[j * m->Kp + d] = (float)v[j * m->k + d];
    return t;
}

// the caller's W_l [D_l][4A] and u <-> the device's one array (fm_autoint.h: W_l transposed, WT_0's rows padded to 16); the elements no
// caller's slot maps to: `pad`
std::vector<float> pack_dense(const fmhip_autoint_model *m, const double *const *W, const double *u, float pad) {
    std::vector<float> t((size_t)m->total, pad);
    const int N = 4 * m->A;
    for (int l = 0; l < m->L; ++l)
        for (int dd = 0; dd < m->rows_of(l); ++dd)
            for (int n = 0; n < N; ++n) t[m->woff[l] + (size_t)n * m->stride_of(l) + dd] = (float)W[l][(size_t)dd * N + n];
    for (int i = 0; i < m->F * m->A; ++i) t[m->hoff + i] = (float)u[i];
    return t;
}

int write_floats(fmhip_autoint_model *m, float *dev, const std::vector<float> &t) {
    HIP_TRY(hipMemcpyAsync(dev, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    return FMHIP_OK;
}

int write_vector(fmhip_autoint_model *m, float *dev, const double *src, size_t n) { return write_floats(m, dev, std::vector<float>(src, src + n)); }

// n floats of the device as doubles; stride > width: the first `width` of every `stride` (the factor table)
int read_vector(fmhip_autoint_model *m, const float *dev, size_t n, double *out, int width = 1, int stride = 1) {
    std::vector<float> t(n);
    HIP_TRY(hipMemcpyAsync(t.data(), dev, n * sizeof(float), hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    for (size_t j = 0; j < n / stride; ++j)
        for (int d = 0; d < width; ++d) out[j * width + d] = t[j * stride + d];
    return FMHIP_OK;
}

int read_dense(fmhip_autoint_model *m, const float *dev, double *const *W, double *u) {
    if (!W && !u) return FMHIP_OK;
    std::vector<float> t((size_t)m->total);
    HIP_TRY(hipMemcpyAsync(t.data(), dev, t.size() * sizeof(float), hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    const int N = 4 * m->A;
    for (int l = 0; l < m->L; ++l)
        if (W && W[l])
            for (int dd = 0; dd < m->rows_of(l); ++dd)
                for (int n = 0; n < N; ++n) W[l][(size_t)dd * N + n] = t[m->woff[l] + (size_t)n * m->stride_of(l) + dd];
    if (u)
        for (int i = 0; i < m->F * m->A; ++i) u[i] = t[m->hoff + i];
    return FMHIP_OK;
}

int check_dense_pointers(const fmhip_autoint_model *m, const double *const *W, const double *u) {
    if (!W || !u) return fail(FMHIP_ERR_INVALID, "NULL argument");
    for (int l = 0; l < m->L; ++l)
        if (!W[l]) return fail(FMHIP_ERR_INVALID, "layer %d: NULL argument", l);
    return FMHIP_OK;
}

// every refusal of (m, d) that needs no launch, then the device and the workspace
int pair_up(fmhip_autoint_model_t m, fmhip_ffm_dataset_t d, bool train) {
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
        const size_t rows = (size_t)std::max<int64_t>(d->max_rows, 1), blocks = (size_t)autoint_forward_blocks(rows);
        TRY(m->e.ensure(rows));
        TRY(m->dz.ensure((size_t)max_nnz * m->Kp));
        TRY(m->bsum.ensure(blocks * 4));
        TRY(m->part.ensure((size_t)std::max(d->max_chunks, 1) * (m->Kp + kFwfmPartTail)));
        if (m->L > 1) TRY(m->scratch.ensure(blocks * autoint_scratch(m->Fp, m->A, m->L)));
        TRY(m->gpart.ensure(blocks * m->total));          // (also what the FwFM's update launch is handed as rpart)
    }
    return FMHIP_OK;
}

AutoIntArgs batch_args(fmhip_autoint_model_t m, fmhip_ffm_dataset_t d, const FfmBatch &b) {
    AutoIntArgs q{};
    FwfmArgs &a = q.b;
    a.V = m->V.p;
    a.w = m->w.p;
    a.w0 = m->w0.p;
    a.NV = m->NV.p;
    a.Nw = m->Nw.p;
    a.N0 = m->N0.p;
    a.Nr = m->ND.p;               // (the FwFM's update launch wants the pointers; with train_r = 0 it reads neither)
    a.rpart = m->gpart.p;
    a.F = m->F;
    a.Fp = m->Fp;
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
    a.n_blocks = autoint_forward_blocks(b.rows);
    a.part = m->part.p;
    a.stats = m->stats.p;
    a.loss = m->loss;
    a.linear = m->linear;
    a.train_r = 0;
    a.eps = (float)m->eps;
    a.invb = b.rows > 0 ? 1.0f / (float)b.rows : 0.f;
    q.D = m->D.p;
    q.ND = m->ND.p;
    q.k = m->k;
    q.L = m->L;
    q.H = m->H;
    q.d = m->d;
    q.A = m->A;
    for (int l = 0; l < m->L; ++l) q.woff[l] = m->woff[l];
    q.hoff = m->hoff;
    q.total = m->total;
    q.scratch = m->scratch.p;
    q.gpart = m->gpart.p;
    q.n_splits = autoint_forward_blocks(b.rows);
    q.train_d = m->train_d;
    return q;
}

bool rate_ok(double x) { return std::isfinite(x) && x >= 0.0; }

int check_rates(double eta, double reg0, double regw, double regv, double regd) {
    if (!std::isfinite(eta) || !rate_ok(reg0) || !rate_ok(regw) || !rate_ok(regv) || !rate_ok(regd))
        return fail(FMHIP_ERR_INVALID, "eta = %g, reg0 = %g, regw = %g, regv = %g, regd = %g: the step size is finite, a regulariser finite and >= 0", eta, reg0,
                    regw, regv, regd);
    return FMHIP_OK;
}

struct Rates {
    double eta, reg0, regw, regv, regd;
};

// one step, asynchronous on the model's stream; acc: the epoch's running sums on the device (nullable)
int autoint_step(fmhip_autoint_model_t m, fmhip_ffm_dataset_t d, int64_t b, const Rates &q, double *acc, bool acc_reset = false) {
    AutoIntArgs a = batch_args(m, d, d->batches[(size_t)b]);
    a.b.eta = (float)q.eta;
    a.b.reg0 = (float)q.reg0;
    a.b.regw = (float)q.regw;
    a.b.regv = (float)q.regv;
    a.regd = (float)q.regd;
    a.b.acc = acc;
    a.b.acc_reset = acc_reset;
    const bool ada = m->opt == FMHIP_OPT_ADAGRAD;
    HIP_TRY(launch_autoint_forward(a, true, m->stream));
    HIP_TRY(launch_fwfm_backward(a.b, ada, m->stream));
    HIP_TRY(launch_fwfm_update(a.b, ada, m->stream));
    if (m->train_d) HIP_TRY(launch_autoint_dupdate(a, ada, m->stream));
    return FMHIP_OK;
}

int read_stats(fmhip_autoint_model_t m, const double *dev, int64_t nnz, int64_t steps, fmhip_stats *st) {
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

int fmhip_autoint_model_create(int device, int64_t num_attribute, int32_t num_fields, int32_t num_factor, int32_t n_layers, int32_t heads, int32_t head_dim,
                               void *stream, fmhip_autoint_model_t *out) {
    if (!out) return fail(FMHIP_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (num_attribute < 0) return fail(FMHIP_ERR_INVALID, "num_attribute = %lld: a model has at least feature 0", (long long)num_attribute);
    if (num_fields < 1) return fail(FMHIP_ERR_INVALID, "num_fields = %d: a model has at least one field", num_fields);
    if (num_fields > FMHIP_AUTOINT_MAX_FIELDS)
        return fail(FMHIP_ERR_UNSUPPORTED, "num_fields = %d is above FMHIP_AUTOINT_MAX_FIELDS = %d", num_fields, FMHIP_AUTOINT_MAX_FIELDS);
    if (num_factor < 1) return fail(FMHIP_ERR_INVALID, "num_factor = %d: a model has at least one factor", num_factor);
    if (num_factor > FMHIP_AUTOINT_MAX_FACTORS)
        return fail(FMHIP_ERR_UNSUPPORTED, "num_factor = %d is above FMHIP_AUTOINT_MAX_FACTORS = %d", num_factor, FMHIP_AUTOINT_MAX_FACTORS);
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
    if (num_attribute >= INT32_MAX) return fail(FMHIP_ERR_UNSUPPORTED, "num_attribute = %lld: feature ids are 32-bit", (long long)num_attribute);
    TRY(set_device(device));
    const int32_t Fp = (num_fields + 15) / 16 * 16, A = heads * head_dim;
    int lds_limit = 0;
    hipError_t e = hipDeviceGetAttribute(&lds_limit, hipDeviceAttributeMaxSharedMemoryPerBlock, device);
    if (e != hipSuccess) return fail(FMHIP_ERR_HIP, "hipDeviceGetAttribute failed: %s", hipGetErrorString(e));
    if (autoint_forward_lds(Fp, A, n_layers, true) > (size_t)lds_limit)
        return fail(FMHIP_ERR_UNSUPPORTED, "num_fields = %d at heads·head_dim = %d and n_layers = %d: a row takes %zu bytes of LDS, the device gives a workgroup %d",
                    num_fields, A, n_layers, autoint_forward_lds(Fp, A, n_layers, true), lds_limit);
    fmhip_autoint_model *m = new (std::nothrow) fmhip_autoint_model();
    if (!m) return fail(FMHIP_ERR_NOMEM, "out of host memory");
    m->device = device;
    m->n = num_attribute;
    m->n1 = num_attribute + 1;
    m->F = num_fields;
    m->Fp = Fp;
    m->k = num_factor;
    m->Kp = num_factor <= 4 ? 4 : (num_factor <= 8 ? 8 : 16);
    m->L = n_layers;
    m->H = heads;
    m->d = head_dim;
    m->A = A;
    int32_t at = 0;
    for (int l = 0; l < n_layers; ++l) {
        m->woff[l] = at;
        at += 4 * A * m->stride_of(l);
    }
    m->hoff = at;
    m->total = at + num_fields * A;
    if (stream) {
        m->stream = reinterpret_cast<hipStream_t>(stream);
    } else {
        e = hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking);
        if (e != hipSuccess) {
            delete m;
            return fail(FMHIP_ERR_HIP, "hipStreamCreate failed: %s", hipGetErrorString(e));
        }
        m->own_stream = true;
    }
    int rc;
    if ((rc = m->V.alloc(m->vfloats())) || (rc = m->w.alloc((size_t)m->n1)) || (rc = m->w0.alloc(1)) || (rc = m->D.alloc((size_t)m->total)) ||
        (rc = m->stats.alloc(4)) || (rc = m->acc.alloc(4))) {
        fmhip_autoint_model_destroy(m);
        return rc;
    }
    e = hipMemset(m->V.p, 0, m->V.n * sizeof(float));
    if (e == hipSuccess) e = hipMemset(m->w.p, 0, m->w.n * sizeof(float));
    if (e == hipSuccess) e = hipMemset(m->w0.p, 0, sizeof(float));
    if (e == hipSuccess) e = hipMemset(m->D.p, 0, m->D.n * sizeof(float));
    if (e == hipSuccess) e = hipMemset(m->stats.p, 0, 4 * sizeof(double));
    if (e == hipSuccess) e = hipMemset(m->acc.p, 0, 4 * sizeof(double));
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        fmhip_autoint_model_destroy(m);
        return fail(FMHIP_ERR_HIP, "setting up the AutoInt model failed: %s", hipGetErrorString(e));
    }
    *out = m;
    return FMHIP_OK;
}

int fmhip_autoint_model_destroy(fmhip_autoint_model_t m) {
    if (!m) return FMHIP_OK;
    (void)hipSetDevice(m->device);
    if (m->stream) (void)hipStreamSynchronize(m->stream);
    if (m->own_stream && m->stream) (void)hipStreamDestroy(m->stream);
    delete m;
    return FMHIP_OK;
}

int fmhip_autoint_model_info(fmhip_autoint_model_t m, int64_t *num_attribute, int32_t *num_fields, int32_t *num_factor, int32_t *padded_factors,
                             int32_t *n_layers, int32_t *heads, int32_t *head_dim) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the AutoInt model handle is NULL");
    if (num_attribute) *num_attribute = m->n;
    if (num_fields) *num_fields = m->F;
    if (num_factor) *num_factor = m->k;
    if (padded_factors) *padded_factors = m->Kp;
    if (n_layers) *n_layers = m->L;
    if (heads) *heads = m->H;
    if (head_dim) *head_dim = m->d;
    return FMHIP_OK;
}

int fmhip_autoint_model_set_params(fmhip_autoint_model_t m, double w0, const double *w, const double *v, const double *const *W, const double *u) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the AutoInt model handle is NULL");
    if (!w || !v) return fail(FMHIP_ERR_INVALID, "NULL argument");
    TRY(check_dense_pointers(m, W, u));
    std::lock_guard<std::mutex> lock(m->mu);
    TRY(set_device(m->device));
    TRY(write_floats(m, m->V.p, pack_table(m, v, 0.f)));
    TRY(write_vector(m, m->w.p, w, (size_t)m->n1));
    TRY(write_floats(m, m->D.p, pack_dense(m, W, u, 0.f)));
    return write_vector(m, m->w0.p, &w0, 1);
}

int fmhip_autoint_model_get_params(fmhip_autoint_model_t m, double *w0, double *w, double *v, double *const *W, double *u) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the AutoInt model handle is NULL");
    std::lock_guard<std::mutex> lock(m->mu);
    TRY(set_device(m->device));
    if (w0) TRY(read_vector(m, m->w0.p, 1, w0));
    if (w) TRY(read_vector(m, m->w.p, (size_t)m->n1, w));
    if (v) TRY(read_vector(m, m->V.p, m->vfloats(), v, m->k, m->Kp));
    return read_dense(m, m->D.p, W, u);
}

int fmhip_autoint_model_set_rule(fmhip_autoint_model_t m, int loss, int optimizer, double eps, double init) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the AutoInt model handle is NULL");
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
        m->ND.release();
        m->opt = FMHIP_OPT_SGD;
        return FMHIP_OK;
    }
    if (m->opt == FMHIP_OPT_ADAGRAD && memcmp(&m->eps, &eps, sizeof eps) == 0 && memcmp(&m->init, &init, sizeof init) == 0) return FMHIP_OK;
    HIP_TRY(hipStreamSynchronize(m->stream));
    TRY(m->NV.alloc(m->vfloats()));
    TRY(m->Nw.alloc((size_t)m->n1));
    TRY(m->N0.alloc(1));
    TRY(m->ND.alloc((size_t)m->total));
    const std::vector<float> fill(std::max({m->vfloats(), (size_t)m->n1, (size_t)m->total}), (float)init);
    HIP_TRY(hipMemcpy(m->NV.p, fill.data(), m->vfloats() * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(m->Nw.p, fill.data(), (size_t)m->n1 * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(m->N0.p, fill.data(), sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(m->ND.p, fill.data(), (size_t)m->total * sizeof(float), hipMemcpyHostToDevice));
    m->opt = FMHIP_OPT_ADAGRAD;
    m->eps = eps;
    m->init = init;
    return FMHIP_OK;
}

int fmhip_autoint_model_set_linear(fmhip_autoint_model_t m, int linear) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the AutoInt model handle is NULL");
    if (linear != 0 && linear != 1) return fail(FMHIP_ERR_INVALID, "linear = %d: 0 or 1", linear);
    std::lock_guard<std::mutex> lock(m->mu);
    m->linear = linear;
    return FMHIP_OK;
}

int fmhip_autoint_model_set_attention(fmhip_autoint_model_t m, int train) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the AutoInt model handle is NULL");
    if (train != 0 && train != 1) return fail(FMHIP_ERR_INVALID, "train = %d: 0 or 1", train);
    std::lock_guard<std::mutex> lock(m->mu);
    m->train_d = train;
    return FMHIP_OK;
}

int fmhip_autoint_model_get_accumulators(fmhip_autoint_model_t m, double *n0, double *nw, double *nv, double *const *nW, double *nu) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the AutoInt model handle is NULL");
    std::lock_guard<std::mutex> lock(m->mu);
    if (m->opt != FMHIP_OPT_ADAGRAD) return fail(FMHIP_ERR_INVALID, "the model is under SGD: it has no accumulators (fmhip_autoint_model_set_rule)");
    TRY(set_device(m->device));
    if (n0) TRY(read_vector(m, m->N0.p, 1, n0));
    if (nw) TRY(read_vector(m, m->Nw.p, (size_t)m->n1, nw));
    if (nv) TRY(read_vector(m, m->NV.p, m->vfloats(), nv, m->k, m->Kp));
    return read_dense(m, m->ND.p, nW, nu);
}

int fmhip_autoint_model_set_accumulators(fmhip_autoint_model_t m, double n0, const double *nw, const double *nv, const double *const *nW, const double *nu) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the AutoInt model handle is NULL");
    if (!nw || !nv) return fail(FMHIP_ERR_INVALID, "NULL argument");
    TRY(check_dense_pointers(m, nW, nu));
    std::lock_guard<std::mutex> lock(m->mu);
    if (m->opt != FMHIP_OPT_ADAGRAD) return fail(FMHIP_ERR_INVALID, "the model is under SGD: it has no accumulators (fmhip_autoint_model_set_rule)");
    if (!rate_ok(n0)) return fail(FMHIP_ERR_INVALID, "n0 = %g: an accumulator is finite and >= 0", n0);
    for (int64_t i = 0; i < m->n1; ++i)
        if (!rate_ok(nw[i])) return fail(FMHIP_ERR_INVALID, "nw[%lld] = %g: an accumulator is finite and >= 0", (long long)i, nw[i]);
    for (size_t j = 0; j < (size_t)m->n1 * m->k; ++j)
        if (!rate_ok(nv[j])) return fail(FMHIP_ERR_INVALID, "nv[%zu] = %g: an accumulator is finite and >= 0", j, nv[j]);
    for (int l = 0; l < m->L; ++l)
        for (size_t j = 0; j < (size_t)m->rows_of(l) * 4 * m->A; ++j)
            if (!rate_ok(nW[l][j])) return fail(FMHIP_ERR_INVALID, "nW[%d][%zu] = %g: an accumulator is finite and >= 0", l, j, nW[l][j]);
    for (size_t j = 0; j < (size_t)m->F * m->A; ++j)
        if (!rate_ok(nu[j])) return fail(FMHIP_ERR_INVALID, "nu[%zu] = %g: an accumulator is finite and >= 0", j, nu[j]);
    TRY(set_device(m->device));
    TRY(write_floats(m, m->NV.p, pack_table(m, nv, (float)m->init)));
    TRY(write_vector(m, m->Nw.p, nw, (size_t)m->n1));
    TRY(write_floats(m, m->ND.p, pack_dense(m, nW, nu, (float)m->init)));
    return write_vector(m, m->N0.p, &n0, 1);
}

int fmhip_autoint_predict(fmhip_autoint_model_t m, fmhip_ffm_dataset_t d, double *yhat) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the AutoInt model handle is NULL");
    if (!d) return fail(FMHIP_ERR_INVALID, "the FFM dataset handle is NULL");
    if (!yhat) return fail(FMHIP_ERR_INVALID, "yhat is NULL");
    std::lock_guard<std::mutex> lock(m->mu);
    TRY(pair_up(m, d, false));
    for (const FfmBatch &b : d->batches) {
        AutoIntArgs a = batch_args(m, d, b);
        a.b.yhat = m->yhat.p + b.row0;
        HIP_TRY(launch_autoint_forward(a, false, m->stream));
    }
    std::vector<float> h((size_t)d->n_rows);
    if (d->n_rows > 0) HIP_TRY(hipMemcpyAsync(h.data(), m->yhat.p, h.size() * sizeof(float), hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    std::copy(h.begin(), h.end(), yhat);
    return FMHIP_OK;
}

int fmhip_autoint_step(fmhip_autoint_model_t m, fmhip_ffm_dataset_t d, int64_t batch, double eta, double reg0, double regw, double regv, double regd,
                   fmhip_stats *stats) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the AutoInt model handle is NULL");
    if (!d) return fail(FMHIP_ERR_INVALID, "the FFM dataset handle is NULL");
    TRY(check_rates(eta, reg0, regw, regv, regd));
    std::lock_guard<std::mutex> lock(m->mu);
    if (batch < 0 || batch >= (int64_t)d->batches.size())
        return fail(FMHIP_ERR_INVALID, "batch = %lld: the dataset has %zu batches", (long long)batch, d->batches.size());
    TRY(pair_up(m, d, true));
    TRY(autoint_step(m, d, batch, Rates{eta, reg0, regw, regv, regd}, nullptr));
    if (stats) TRY(read_stats(m, m->stats.p, d->batches[(size_t)batch].nnz, 1, stats));
    return FMHIP_OK;
}

int fmhip_autoint_epoch(fmhip_autoint_model_t m, fmhip_ffm_dataset_t d, double eta, double reg0, double regw, double regv, double regd, const int64_t *order,
                    fmhip_stats *stats) {
    if (!m) return fail(FMHIP_ERR_INVALID, "the AutoInt model handle is NULL");
    if (!d) return fail(FMHIP_ERR_INVALID, "the FFM dataset handle is NULL");
    TRY(check_rates(eta, reg0, regw, regv, regd));
    std::lock_guard<std::mutex> lock(m->mu);
    const int64_t nb = (int64_t)d->batches.size();
    if (order)
        for (int64_t j = 0; j < nb; ++j)
            if (order[j] < 0 || order[j] >= nb) return fail(FMHIP_ERR_INVALID, "order[%lld] = %lld: the dataset has %lld batches", (long long)j, (long long)order[j], (long long)nb);
    TRY(pair_up(m, d, true));
    // the epoch's sums: the first step's update launch overwrites them, the others add
    for (int64_t j = 0; j < nb; ++j) TRY(autoint_step(m, d, order ? order[j] : j, Rates{eta, reg0, regw, regv, regd}, m->acc.p, j == 0));
    if (stats) TRY(read_stats(m, m->acc.p, d->nnz, nb, stats));
    return FMHIP_OK;
}

}  // extern "C"
