// fmhip_api.hip — the C ABI declared in include/fmhip.h, less its scoring calls: library / model entry points (with the one
// codec between the device's padded tables and the reference's layout), the training calls, the reference's ALS learner, the
// split step a host-orchestrated exchange drives, profiling.  The rest of the library:
//   fmhip_score.hip     the scoring calls (predictions, metrics, top-K) and the pass they share
//   fmhip_dataset.hip   datasets (host passes, device transposes, layout queries, feature relabelling)
//   fmhip_step.hip      the launch sequence of one mini-batch step
//   fmhip_comm.hip      the data-parallel step (RCCL / caller's transport)
//   fm_forward / fm_backward / fm_apply / als_kernels / csc_build / fm_topk / fm_pairing / fm_auc .hip   the kernels
#include "fmhip_internal.h"
#include "als_kernels.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

using namespace fmhip;

namespace fmhip {
namespace host {

thread_local std::string g_err;

int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

}  // namespace host
}  // namespace fmhip

using namespace fmhip::host;

namespace fmhip {
namespace host {

int set_device(int device) {
    HIP_TRY(hipSetDevice(device));
    return FMHIP_OK;
}

// ---- the table codec.  On the device a table is padded [n1p][Kp] fp32 rows; with packed rows (k < Kp) slot k of row i carries
// the row's linear entry (w_i, its AdaGrad accumulator, its gradient), otherwise a vector beside the table does.  The reference's
// layout is w[i], v[f + i*k].  These three functions are the only ones that know where the linear entry lives.

// the linear entry of row i of a host copy (T: the table, wsep: the vector beside it)
inline float table_w(const fmhip_model *m, const float *T, const float *wsep, int64_t i) {
    return m->pack_k() >= 0 ? T[(size_t)i * m->Kp + m->k] : wsep[i];
}

// `rows` rows of a host copy -> w[rows] * sw, v[k * rows] * sv (either may be NULL); the products are formed in fp64 (exact at
// scale 1) and then converted to FT
template <typename FT>
void table_unpack(const fmhip_model *m, const float *T, const float *wsep, int64_t rows, double sw, double sv, FT *w, FT *v) {
    for (int64_t i = 0; i < rows; ++i) {
        if (w) w[i] = (FT)((double)table_w(m, T, wsep, i) * sw);
        if (v)
            for (int f = 0; f < m->k; ++f) v[f + i * (int64_t)m->k] = (FT)((double)T[(size_t)i * m->Kp + f] * sv);
    }
}

// w[n1], v[k * n1] -> a whole host table T [n1p][Kp] and, where asked for, the vector wsep [n1p]; everything else holds `fill`
template <typename FT>
void table_pack(const fmhip_model *m, const FT *w, const FT *v, float fill, std::vector<float> &T, std::vector<float> *wsep) {
    T.assign((size_t)m->n1p * m->Kp, fill);
    if (wsep) wsep->assign((size_t)m->n1p, fill);
    for (int64_t i = 0; i < m->n1; ++i) {
        for (int f = 0; f < m->k; ++f) T[(size_t)i * m->Kp + f] = (float)v[f + i * (int64_t)m->k];
        if (m->pack_k() >= 0) T[(size_t)i * m->Kp + m->k] = (float)w[i];
        if (wsep) (*wsep)[(size_t)i] = (float)w[i];
    }
}

// An FTRL model's parameters were replaced (set_params, init_normal, ALS through set_params_impl): zeta = -theta (beta + sqrt(n)) from
// the new theta and the current n, on the model's stream — theta and zeta never disagree.  `old` (set_params): the tables before the
// call — a parameter whose fp32 bits did not change keeps its zeta (a model's own values written back, as a host mirror that uploads
// before every call does, lose no state).  Any other model: nothing
struct FtrlBefore {
    DevBuf<float> V, w, w0;
    int take(fmhip_model_t m) {      // the tables as they are, queued on the model's stream
        if (!m->rule.ftrl()) return FMHIP_OK;
        TRY(fold_scales(m));         // (FTRL tables are at scale 1 already; a no-op that states it)
        TRY(V.alloc((size_t)m->n1p * m->Kp));
        TRY(w.alloc((size_t)m->n1p));
        TRY(w0.alloc(1));
        HIP_TRY(hipMemcpyAsync(V.p, m->V.p, V.n * sizeof(float), hipMemcpyDeviceToDevice, m->stream));
        HIP_TRY(hipMemcpyAsync(w.p, m->w.p, w.n * sizeof(float), hipMemcpyDeviceToDevice, m->stream));
        HIP_TRY(hipMemcpyAsync(w0.p, m->w0.p, sizeof(float), hipMemcpyDeviceToDevice, m->stream));
        return FMHIP_OK;
    }
};

int ftrl_rederive(fmhip_model_t m, const FtrlBefore *old = nullptr) {
    if (!m->rule.ftrl()) return FMHIP_OK;
    HIP_TRY(launch_ftrl_init(m->Kp, m->V.p, m->w.p, m->w0.p, m->NV.p, m->Nw.p, m->N0.p, m->ZV.p, m->Zw.p, m->Z0.p, old ? old->V.p : nullptr,
                             old ? old->w.p : nullptr, old ? old->w0.p : nullptr, m->n1p, (float)m->rule.ftrl_beta, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));      // (`old` is freed by the caller)
    return FMHIP_OK;
}

template <typename FT>
int set_params_impl(fmhip_model_t m, FT w0, const FT *w, const FT *v) {
    if (!m || !w || !v) return fail(FMHIP_ERR_INVALID, "NULL argument");
    TRY(set_device(m->device));
    std::vector<float> hV, hw;
    table_pack(m, w, v, 0.f, hV, &hw);          // (the vector is filled for packed rows too)
    const float hw0 = (float)w0;
    m->h_w0 = (double)w0;
    m->h_w.assign(w, w + m->n1);
    m->h_v.assign(v, v + m->n1 * m->k);
    m->host64_fresh = true;
    FtrlBefore before;
    TRY(before.take(m));
    m->sv = m->sw = 1.0;
    HIP_TRY(hipMemcpyAsync(m->V.p, hV.data(), hV.size() * sizeof(float), hipMemcpyHostToDevice, m->stream));
    HIP_TRY(hipMemcpyAsync(m->w.p, hw.data(), hw.size() * sizeof(float), hipMemcpyHostToDevice, m->stream));
    HIP_TRY(hipMemcpyAsync(m->w0.p, &hw0, sizeof(float), hipMemcpyHostToDevice, m->stream));
    TRY(ftrl_rederive(m, &before));
    HIP_TRY(hipStreamSynchronize(m->stream));
    return FMHIP_OK;
}

template <typename FT>
int get_params_impl(fmhip_model_t m, FT *w0, FT *w, FT *v) {
    if (!m) return fail(FMHIP_ERR_INVALID, "model is NULL");
    TRY(set_device(m->device));
    if (m->host64_fresh) {   // nothing has trained in fp32 since the masters were written: return them exactly
        if (w0) *w0 = (FT)m->h_w0;
        if (w) for (int64_t i = 0; i < m->n1; ++i) w[i] = (FT)m->h_w[(size_t)i];
        if (v) for (int64_t j = 0; j < m->n1 * m->k; ++j) v[j] = (FT)m->h_v[(size_t)j];
        return FMHIP_OK;
    }
    std::vector<float> hV((size_t)m->n1p * m->Kp), hw((size_t)m->n1p);
    float hw0 = 0.f;
    HIP_TRY(hipMemcpyAsync(hV.data(), m->V.p, hV.size() * sizeof(float), hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipMemcpyAsync(hw.data(), m->w.p, hw.size() * sizeof(float), hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipMemcpyAsync(&hw0, m->w0.p, sizeof(float), hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    if (w0) *w0 = (FT)hw0;
    // a lazily decayed model stores U with V = sv*U (fm_apply.hip); with sv = sw = 1 the products are exact
    table_unpack(m, hV.data(), hw.data(), m->n1, m->sw, m->sv, w, v);
    return FMHIP_OK;
}

// ---- the column walk's epoch in pieces (fmhip_als_epoch below; fmhip_mcmc_epoch, fmhip_mcmc.hip) — the model's lock is the caller's

// every reason the column walk refuses (m, d) — the model is untouched
int als_check(fmhip_model_t m, fmhip_dataset_t d) {
    TRY(check_train(m, d));
    if (const char *why = refusal(Path::kAls, m->rule, d->weighted)) return fail(FMHIP_ERR_UNSUPPORTED, "%s", why);
    if (d->batches.size() > 1 || (d->nnz > 0 && !d->val64.p))
        return fail(FMHIP_ERR_UNSUPPORTED, "ALS walks the whole-dataset transpose: create the dataset with batch_rows <= 0 "
                                           "(single batch, at most 2^27 stored nonzeros) and without asking for the dense hot "
                                           "block (fmhip_dataset_opts::hot_block <= 0)");
    if (d->rb_rows > 0) return fail(FMHIP_ERR_UNSUPPORTED, "ALS needs a dataset without row blocks (FMHIP_TUNE_ROW_BLOCK = 0)");
    if (d->als_dup)
        return fail(FMHIP_ERR_UNSUPPORTED, "ALS: a row stores the same feature index twice; the column walk updates every row of a "
                                           "column at once and needs the (row, feature) pairs to be distinct");
    return FMHIP_OK;
}

// the walk's arguments over dataset d with the model's fp64 device parameters: the dataset's and the parameters' fields, and the
// chip-wide column step's partials (the model's, whatever dataset is walked); y, the regularisers, e and q are the caller's
AlsArgs als_args(fmhip_model_t m, fmhip_dataset_t d) {
    AlsArgs a{};
    a.k = m->k;
    a.num_attribute = m->n;
    a.n_rows = d->n_rows;
    a.nnz = d->nnz;
    a.row_ptr = d->row_ptr.p;
    a.col = d->col.p;
    a.val = d->val64.p;
    a.scol = d->scol.p;
    a.sval = d->sval64.p;
    a.n_cols = d->n_rows > 0 ? d->batches[0].n_cols : 0;
    a.cfeat = d->cfeat.p;
    a.cptr = d->cptr.p;
    a.crow = d->crow.p;
    a.cval = d->cval64.p;
    a.w0 = m->als_w0.p;
    a.w = m->als_w.p;
    a.v = m->als_v.p;
    a.part = m->als_part.p;
    a.lev_cols = d->als_lev_cols.p;
    return a;
}

// the host's view of d's columns, which the walk's launch plan follows
ColumnPlan als_plan(fmhip_dataset_t d) {
    const int n_levels = d->als_lev_ptr.empty() ? 0 : (int)d->als_lev_ptr.size() - 1;
    return ColumnPlan{d->h_cfeat.data(), d->h_cptr.data(), n_levels ? d->als_lev_ptr.data() : nullptr, d->h_als_lev_cols.data(), n_levels};
}

// the fp64 masters onto the device and the walk's arguments (the workspace is the model's); *a is meaningful when d has rows
int als_begin(fmhip_model_t m, fmhip_dataset_t d, double reg0, double regw, double regv, AlsArgs *out) {
    TRY(als_check(m, d));
    if (!m->host64_fresh) {   // parameters last changed by fp32 SGD: start from their fp64 widening
        std::vector<double> w((size_t)m->n1), v((size_t)m->n1 * m->k);
        double w0 = 0.0;
        TRY(get_params_impl<double>(m, &w0, w.data(), v.data()));
        m->h_w0 = w0;
        m->h_w.swap(w);
        m->h_v.swap(v);
        m->host64_fresh = true;
    }
    const size_t n1 = (size_t)m->n1, nv = n1 * (size_t)m->k, nr = (size_t)std::max<int64_t>(d->n_rows, 1);
    TRY(m->als_w0.ensure(1));
    TRY(m->als_w.ensure(n1));
    TRY(m->als_v.ensure(nv));
    TRY(m->als_e.ensure(nr));
    TRY(m->als_q.ensure(nr * (size_t)m->k));
    TRY(m->als_part.ensure(2 * (size_t)kAlsMaxParts + 2));
    HIP_TRY(hipMemcpyAsync(m->als_w0.p, &m->h_w0, sizeof(double), hipMemcpyHostToDevice, m->stream));
    HIP_TRY(hipMemcpyAsync(m->als_w.p, m->h_w.data(), n1 * sizeof(double), hipMemcpyHostToDevice, m->stream));
    HIP_TRY(hipMemcpyAsync(m->als_v.p, m->h_v.data(), nv * sizeof(double), hipMemcpyHostToDevice, m->stream));
    AlsArgs a{};
    if (d->n_rows > 0) {
        a = als_args(m, d);
        a.y = d->y64.p;
        a.reg0 = reg0;
        a.regw = regw;
        a.regv = regv;
        a.e = m->als_e.p;
        a.q = m->als_q.p;
    }
    *out = a;
    return FMHIP_OK;
}

// the device's fp64 parameters back into the masters and the fp32 device copy (synchronises)
int als_end(fmhip_model_t m) {
    const size_t n1 = (size_t)m->n1, nv = n1 * (size_t)m->k;
    std::vector<double> w(n1), v(nv);
    double w0 = 0.0;
    HIP_TRY(hipMemcpyAsync(&w0, m->als_w0.p, sizeof(double), hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipMemcpyAsync(w.data(), m->als_w.p, n1 * sizeof(double), hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipMemcpyAsync(v.data(), m->als_v.p, nv * sizeof(double), hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    return set_params_impl<double>(m, w0, w.data(), v.data());   // refreshes the fp64 masters and the fp32 device copy
}

}  // namespace host
}  // namespace fmhip

// =================================================================== C ABI

extern "C" {

int fmhip_version(void) { return FMHIP_VERSION; }

int fmhip_ablation_mask(void) { return forward_ablations() | backward_ablations(); }

const char *fmhip_last_error(void) { return g_err.c_str(); }

// enum fmhip_tune_key (include/fmhip_experimental.h) names the kernels' own keys (fm_kernels.h)
static_assert(FMHIP_TUNE_FORWARD_KERNEL == kTuneFwd && FMHIP_TUNE_BACKWARD_KERNEL == kTuneBwd && FMHIP_TUNE_TILE_ROWS == kTuneTile &&
              FMHIP_TUNE_ROW_BLOCK == kTuneRowBlock && FMHIP_TUNE_XCD_PLACEMENT == kTuneXcd && FMHIP_TUNE_HOT_BLOCK == kTuneHot &&
              FMHIP_TUNE_FORWARD_OCCUPANCY == kTuneFwdOcc && FMHIP_TUNE_ROW_ORDER == kTuneRowOrder && FMHIP_TUNE_FLAT_ADDRESS == kTuneFlat &&
              FMHIP_TUNE_LAZY_DECAY == kTuneLazy && FMHIP_TUNE_FUSED_UPDATE == kTuneFused && FMHIP_TUNE_MERGED_FINISH == kTuneMerged &&
              FMHIP_TUNE_HOT_PAGES == kTuneHotPages && FMHIP_TUNE_KEY_COUNT == kTuneCount, "fmhip_experimental.h and fm_kernels.h disagree on the tuning keys");

int fmhip_tune(int key, int value) {
    if (key < 0 || key >= kTuneCount) return fail(FMHIP_ERR_INVALID, "unknown tuning key %d", key);
    g_tune[key] = value;
    return FMHIP_OK;
}

int fmhip_model_tune(fmhip_model_t m, int key, int value) {
    WriteLock lock(m);
    if (!m) return fail(FMHIP_ERR_INVALID, "model is NULL");
    if (key < 0 || key >= kTuneCount) return fail(FMHIP_ERR_INVALID, "unknown tuning key %d", key);
    if (key == kTuneRowBlock || key == kTuneHot || key == kTuneHotPages)
        return fail(FMHIP_ERR_INVALID, "tuning key %d decides a DATASET's layout: state it in fmhip_dataset_opts (or the process default, fmhip_tune)", key);
    m->tune[key] = value < 0 ? -1 : value;
    return FMHIP_OK;
}

int fmhip_device_count(int *count) {
    if (!count) return fail(FMHIP_ERR_INVALID, "count is NULL");
    *count = 0;
    HIP_TRY(hipGetDeviceCount(count));
    return FMHIP_OK;
}

int fmhip_model_create(int device, int64_t num_attribute, int32_t num_factor, void *stream, fmhip_model_t *out) {
    if (!out) return fail(FMHIP_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (num_attribute < 0 || num_attribute >= ((int64_t)1 << 31) - 8)
        return fail(FMHIP_ERR_INVALID, "num_attribute %lld out of range", (long long)num_attribute);
    if (num_factor < 1) return fail(FMHIP_ERR_INVALID, "num_factor must be >= 1");
    if (num_factor > FMHIP_MAX_FACTORS)
        return fail(FMHIP_ERR_UNSUPPORTED, "num_factor %d > FMHIP_MAX_FACTORS (%d)", num_factor, FMHIP_MAX_FACTORS);
    TRY(set_device(device));
    fmhip_model *m = new (std::nothrow) fmhip_model();
    if (!m) return fail(FMHIP_ERR_NOMEM, "out of host memory");
    m->device = device;
    for (int &t : m->tune) t = -1;          // every key follows the process-wide default until fmhip_model_tune says otherwise
    m->n = num_attribute;
    m->n1 = num_attribute + 1;
    m->n1p = (m->n1 + 3) & ~(int64_t)3;
    m->k = num_factor;
    m->Kp = padded_factors(num_factor);
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
    const size_t slack = (size_t)fmhip_model::kSlackRows * m->Kp;       // zero rows behind the tables (sharded exchange)
    if ((rc = m->V.alloc((size_t)m->n1p * m->Kp + slack)) || (rc = m->w.alloc((size_t)m->n1p)) || (rc = m->w0.alloc(1)) ||
        (rc = m->grad_own.alloc(m->grad_floats() + slack)) || (rc = m->acc.alloc(4))) {
        fmhip_model_destroy(m);
        return rc;
    }
    m->grad = m->grad_own.p;
    hipError_t e = hipSuccess;
    if (e == hipSuccess) e = hipMemsetAsync(m->V.p, 0, m->V.n * sizeof(float), m->stream);
    if (e == hipSuccess) e = hipMemsetAsync(m->w.p, 0, m->w.n * sizeof(float), m->stream);
    if (e == hipSuccess) e = hipMemsetAsync(m->w0.p, 0, sizeof(float), m->stream);
    if (e == hipSuccess) e = hipMemsetAsync(m->grad, 0, m->grad_own.n * sizeof(float), m->stream);
    if (e == hipSuccess) e = hipMemsetAsync(m->acc.p, 0, 4 * sizeof(double), m->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(m->stream);
    if (e != hipSuccess) {
        fmhip_model_destroy(m);
        return fail(FMHIP_ERR_HIP, "zero-initialisation failed: %s", hipGetErrorString(e));
    }
    *out = m;
    return FMHIP_OK;
}

int fmhip_model_destroy(fmhip_model_t m) {
    if (!m) return FMHIP_OK;
    (void)hipSetDevice(m->device);
    if (m->stream) (void)hipStreamSynchronize(m->stream);
    for (auto &r : m->prof) {
        (void)hipEventDestroy(r.a);
        (void)hipEventDestroy(r.b);
    }
    if (m->own_stream && m->stream) (void)hipStreamDestroy(m->stream);
    delete m;
    return FMHIP_OK;
}

int fmhip_model_info(fmhip_model_t m, int64_t *num_attribute, int32_t *num_factor, int32_t *padded) {
    ReadLock lock(m);
    if (!m) return fail(FMHIP_ERR_INVALID, "model is NULL");
    if (num_attribute) *num_attribute = m->n;
    if (num_factor) *num_factor = m->k;
    if (padded) *padded = m->Kp;
    return FMHIP_OK;
}

static_assert((int)FMHIP_LOSS_SQUARED == (int)kLossSquared && (int)FMHIP_LOSS_LOGISTIC == (int)kLossLogistic, "fmhip.h and fm_kernels.h disagree on the losses");

int fmhip_model_set_loss(fmhip_model_t m, int loss) {
    if (loss != FMHIP_LOSS_SQUARED && loss != FMHIP_LOSS_LOGISTIC)
        return fail(FMHIP_ERR_INVALID, "loss %d: FMHIP_LOSS_SQUARED (0) or FMHIP_LOSS_LOGISTIC (1)", loss);
    WriteLock lock(m);
    if (!m) return fail(FMHIP_ERR_INVALID, "model is NULL");
    m->rule.loss = loss;
    return FMHIP_OK;
}

int fmhip_model_set_pairing(fmhip_model_t m, int pairing) {
    if (pairing != FMHIP_PAIRING_NONE && pairing != FMHIP_PAIRING_ADJACENT)
        return fail(FMHIP_ERR_INVALID, "pairing %d: FMHIP_PAIRING_NONE (0) or FMHIP_PAIRING_ADJACENT (1)", pairing);
    WriteLock lock(m);
    if (!m) return fail(FMHIP_ERR_INVALID, "model is NULL");
    m->rule.pairing = pairing;
    return FMHIP_OK;
}

// back to plain SGD: the accumulators (AdaGrad's or FTRL's) and FTRL's zeta are freed, the rule's settings cleared
static int drop_optimizer_state(fmhip_model_t m) {
    if (m->rule.adagrad() || m->rule.ftrl()) HIP_TRY(hipStreamSynchronize(m->stream));    // no queued update may still use them
    m->NV.release();
    m->Nw.release();
    m->N0.release();
    m->ZV.release();
    m->Zw.release();
    m->Z0.release();
    m->rule.opt = FMHIP_OPT_SGD;
    m->rule.ada_eps = m->rule.ada_init = 0.0;
    m->rule.ftrl_beta = m->rule.ftrl_init = m->rule.ftrl_l1w = m->rule.ftrl_l1v = 0.0;
    return FMHIP_OK;
}

int fmhip_model_set_optimizer(fmhip_model_t m, int optimizer, double eps, double initial_accumulator) {
    if (optimizer != FMHIP_OPT_SGD && optimizer != FMHIP_OPT_ADAGRAD)
        return fail(FMHIP_ERR_INVALID, "optimizer %d: FMHIP_OPT_SGD (0) or FMHIP_OPT_ADAGRAD (1) (FTRL-Proximal has settings of its own: "
                                       "fmhip_model_set_ftrl, fmhip_ftrl.h)", optimizer);
    if (optimizer == FMHIP_OPT_ADAGRAD && !(std::isfinite(eps) && eps > 0.0))
        return fail(FMHIP_ERR_INVALID, "AdaGrad eps must be finite and > 0 (got %g)", eps);
    if (optimizer == FMHIP_OPT_ADAGRAD && !(std::isfinite(initial_accumulator) && initial_accumulator >= 0.0))
        return fail(FMHIP_ERR_INVALID, "AdaGrad initial_accumulator must be finite and >= 0 (got %g)", initial_accumulator);
    WriteLock lock(m);
    if (!m) return fail(FMHIP_ERR_INVALID, "model is NULL");
    TRY(set_device(m->device));
    if (m->rule.ftrl()) TRY(drop_optimizer_state(m));      // an FTRL model: its state goes first, whatever comes next
    if (optimizer == FMHIP_OPT_SGD) return drop_optimizer_state(m);
    TrainRule want = m->rule;
    want.opt = FMHIP_OPT_ADAGRAD;
    want.ada_eps = eps;
    want.ada_init = initial_accumulator;
    if (m->rule == want) return FMHIP_OK;
    TRY(fold_scales(m));          // the AdaGrad kernels work on tables at scale 1
    m->rule.opt = FMHIP_OPT_SGD;  // (until the accumulators are in place)
    TRY(m->NV.ensure((size_t)m->n1p * m->Kp));
    if (m->pack_k() < 0) TRY(m->Nw.ensure((size_t)m->n1p));
    TRY(m->N0.ensure(1));
    const float init = (float)initial_accumulator;
    uint32_t bits;
    memcpy(&bits, &init, sizeof bits);
    HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(m->NV.p), (int)bits, m->NV.n, m->stream));
    if (m->Nw.p) HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(m->Nw.p), (int)bits, m->Nw.n, m->stream));
    HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(m->N0.p), (int)bits, 1, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    m->rule = want;
    return FMHIP_OK;
}

int fmhip_model_get_optimizer_state(fmhip_model_t m, double *n0, double *nw, double *nv) {
    ReadLock lock(m);
    if (!m) return fail(FMHIP_ERR_INVALID, "model is NULL");
    if (!m->rule.adagrad()) return fail(FMHIP_ERR_INVALID, "the model has no optimizer state (fmhip_model_set_optimizer: FMHIP_OPT_ADAGRAD)");
    TRY(set_device(m->device));
    std::vector<float> hN((size_t)m->n1p * m->Kp), hw(m->Nw.p ? (size_t)m->n1p : 0);
    float h0 = 0.f;
    HIP_TRY(hipMemcpyAsync(hN.data(), m->NV.p, hN.size() * sizeof(float), hipMemcpyDeviceToHost, m->stream));
    if (m->Nw.p) HIP_TRY(hipMemcpyAsync(hw.data(), m->Nw.p, hw.size() * sizeof(float), hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipMemcpyAsync(&h0, m->N0.p, sizeof(float), hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    if (n0) *n0 = h0;
    table_unpack(m, hN.data(), hw.data(), m->n1, 1.0, 1.0, nw, nv);     // (the accumulators carry no scale)
    return FMHIP_OK;
}

int fmhip_model_set_optimizer_state(fmhip_model_t m, double n0, const double *nw, const double *nv) {
    WriteLock lock(m);
    if (!m || !nw || !nv) return fail(FMHIP_ERR_INVALID, "NULL argument");
    if (!m->rule.adagrad()) return fail(FMHIP_ERR_INVALID, "the model has no optimizer state (fmhip_model_set_optimizer: FMHIP_OPT_ADAGRAD)");
    auto ok = [](double x) { return std::isfinite(x) && x >= 0.0; };
    if (!ok(n0)) return fail(FMHIP_ERR_INVALID, "accumulator of w0 is negative or not finite");
    for (int64_t i = 0; i < m->n1; ++i)
        if (!ok(nw[i])) return fail(FMHIP_ERR_INVALID, "accumulator nw[%lld] is negative or not finite", (long long)i);
    for (int64_t j = 0; j < m->n1 * m->k; ++j)
        if (!ok(nv[j])) return fail(FMHIP_ERR_INVALID, "accumulator nv[%lld] is negative or not finite", (long long)j);
    TRY(set_device(m->device));
    std::vector<float> hN, hw;
    table_pack(m, nw, nv, (float)m->rule.ada_init, hN, m->Nw.p ? &hw : nullptr);     // padding: what set_optimizer filled in
    const float h0 = (float)n0;
    HIP_TRY(hipMemcpyAsync(m->NV.p, hN.data(), hN.size() * sizeof(float), hipMemcpyHostToDevice, m->stream));
    if (m->Nw.p) HIP_TRY(hipMemcpyAsync(m->Nw.p, hw.data(), hw.size() * sizeof(float), hipMemcpyHostToDevice, m->stream));
    HIP_TRY(hipMemcpyAsync(m->N0.p, &h0, sizeof(float), hipMemcpyHostToDevice, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    return FMHIP_OK;
}

// ---- FTRL-Proximal (include/fmhip_ftrl.h)

static_assert((int)FMHIP_OPT_SGD == (int)kRuleSgd && (int)FMHIP_OPT_ADAGRAD == (int)kRuleAdaGrad && (int)FMHIP_OPT_FTRL == (int)kRuleFtrl,
              "fmhip.h / fmhip_ftrl.h and fm_kernels.h disagree on the update rules");

int fmhip_model_set_ftrl(fmhip_model_t m, double beta, double initial_accumulator, double l1w, double l1v) {
    auto ok = [](double x) { return std::isfinite(x) && x >= 0.0; };
    if (!ok(beta)) return fail(FMHIP_ERR_INVALID, "FTRL beta must be finite and >= 0 (got %g)", beta);
    if (!ok(initial_accumulator)) return fail(FMHIP_ERR_INVALID, "FTRL initial_accumulator must be finite and >= 0 (got %g)", initial_accumulator);
    if (!ok(l1w)) return fail(FMHIP_ERR_INVALID, "FTRL l1w must be finite and >= 0 (got %g)", l1w);
    if (!ok(l1v)) return fail(FMHIP_ERR_INVALID, "FTRL l1v must be finite and >= 0 (got %g)", l1v);
    // (in the fp32 the kernels divide in)
    if (!((float)beta + std::sqrt((float)initial_accumulator) > 0.f))
        return fail(FMHIP_ERR_INVALID, "FTRL needs beta + sqrt(initial_accumulator) > 0 (got beta %g, initial_accumulator %g): the first "
                                       "step would divide by zero", beta, initial_accumulator);
    WriteLock lock(m);
    if (!m) return fail(FMHIP_ERR_INVALID, "model is NULL");
    TRY(set_device(m->device));
    TrainRule want = m->rule;
    want.opt = FMHIP_OPT_FTRL;
    want.ada_eps = want.ada_init = 0.0;
    want.ftrl_beta = beta;
    want.ftrl_init = initial_accumulator;
    want.ftrl_l1w = l1w;
    want.ftrl_l1v = l1v;
    if (m->rule == want) return FMHIP_OK;
    TRY(fold_scales(m));          // the FTRL kernels work on tables at scale 1
    TRY(drop_optimizer_state(m));  // (SGD until the state is in place; AdaGrad's accumulators are not FTRL's)
    TRY(m->NV.ensure((size_t)m->n1p * m->Kp));
    TRY(m->ZV.ensure((size_t)m->n1p * m->Kp));
    if (m->pack_k() < 0) {
        TRY(m->Nw.ensure((size_t)m->n1p));
        TRY(m->Zw.ensure((size_t)m->n1p));
    }
    TRY(m->N0.ensure(1));
    TRY(m->Z0.ensure(1));
    const float init = (float)initial_accumulator;
    uint32_t bits;
    memcpy(&bits, &init, sizeof bits);
    HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(m->NV.p), (int)bits, m->NV.n, m->stream));
    if (m->Nw.p) HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(m->Nw.p), (int)bits, m->Nw.n, m->stream));
    HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(m->N0.p), (int)bits, 1, m->stream));
    m->rule = want;
    const int rc = ftrl_rederive(m);
    if (rc != FMHIP_OK) {
        (void)drop_optimizer_state(m);
        return rc;
    }
    return FMHIP_OK;
}

int fmhip_model_get_ftrl_state(fmhip_model_t m, double *z0, double *zw, double *zv, double *n0, double *nw, double *nv) {
    ReadLock lock(m);
    if (!m) return fail(FMHIP_ERR_INVALID, "model is NULL");
    if (!m->rule.ftrl()) return fail(FMHIP_ERR_INVALID, "the model has no FTRL state (fmhip_model_set_ftrl)");
    TRY(set_device(m->device));
    std::vector<float> hT((size_t)m->n1p * m->Kp), hw(m->Nw.p ? (size_t)m->n1p : 0);
    float h0 = 0.f;
    for (int pass = 0; pass < 2; ++pass) {      // zeta, then n
        const float *T = pass ? m->NV.p : m->ZV.p, *wv = pass ? m->Nw.p : m->Zw.p, *s0 = pass ? m->N0.p : m->Z0.p;
        HIP_TRY(hipMemcpyAsync(hT.data(), T, hT.size() * sizeof(float), hipMemcpyDeviceToHost, m->stream));
        if (wv) HIP_TRY(hipMemcpyAsync(hw.data(), wv, hw.size() * sizeof(float), hipMemcpyDeviceToHost, m->stream));
        HIP_TRY(hipMemcpyAsync(&h0, s0, sizeof(float), hipMemcpyDeviceToHost, m->stream));
        HIP_TRY(hipStreamSynchronize(m->stream));
        if (double *o0 = pass ? n0 : z0) *o0 = h0;
        table_unpack(m, hT.data(), hw.data(), m->n1, 1.0, 1.0, pass ? nw : zw, pass ? nv : zv);     // (the state carries no scale)
    }
    return FMHIP_OK;
}

int fmhip_model_set_ftrl_state(fmhip_model_t m, double z0, const double *zw, const double *zv, double n0, const double *nw, const double *nv) {
    if (!std::isfinite(z0)) return fail(FMHIP_ERR_INVALID, "z0 is not finite");
    if (!(std::isfinite(n0) && n0 >= 0.0)) return fail(FMHIP_ERR_INVALID, "n0 is negative or not finite");
    WriteLock lock(m);
    if (!m || !zw || !zv || !nw || !nv) return fail(FMHIP_ERR_INVALID, "NULL argument");
    if (!m->rule.ftrl()) return fail(FMHIP_ERR_INVALID, "the model has no FTRL state (fmhip_model_set_ftrl)");
    for (int64_t i = 0; i < m->n1; ++i) {
        if (!std::isfinite(zw[i])) return fail(FMHIP_ERR_INVALID, "zw[%lld] is not finite", (long long)i);
        if (!(std::isfinite(nw[i]) && nw[i] >= 0.0)) return fail(FMHIP_ERR_INVALID, "nw[%lld] is negative or not finite", (long long)i);
    }
    for (int64_t j = 0; j < m->n1 * m->k; ++j) {
        if (!std::isfinite(zv[j])) return fail(FMHIP_ERR_INVALID, "zv[%lld] is not finite", (long long)j);
        if (!(std::isfinite(nv[j]) && nv[j] >= 0.0)) return fail(FMHIP_ERR_INVALID, "nv[%lld] is negative or not finite", (long long)j);
    }
    TRY(set_device(m->device));
    std::vector<float> hT, hw;
    for (int pass = 0; pass < 2; ++pass) {      // zeta, then n; padding: what fmhip_model_set_ftrl leaves there (theta = 0: zeta = -0)
        float *T = pass ? m->NV.p : m->ZV.p, *wv = pass ? m->Nw.p : m->Zw.p, *s0 = pass ? m->N0.p : m->Z0.p;
        table_pack(m, pass ? nw : zw, pass ? nv : zv, pass ? (float)m->rule.ftrl_init : -0.f, hT, wv ? &hw : nullptr);
        const float h0 = (float)(pass ? n0 : z0);
        HIP_TRY(hipMemcpyAsync(T, hT.data(), hT.size() * sizeof(float), hipMemcpyHostToDevice, m->stream));
        if (wv) HIP_TRY(hipMemcpyAsync(wv, hw.data(), hw.size() * sizeof(float), hipMemcpyHostToDevice, m->stream));
        HIP_TRY(hipMemcpyAsync(s0, &h0, sizeof(float), hipMemcpyHostToDevice, m->stream));
        HIP_TRY(hipStreamSynchronize(m->stream));
    }
    return FMHIP_OK;
}

int fmhip_model_nonzeros(fmhip_model_t m, int64_t *w_nonzero, int64_t *v_nonzero, int64_t *features_all_zero) {
    ReadLock lock(m);
    if (!m) return fail(FMHIP_ERR_INVALID, "model is NULL");
    TRY(set_device(m->device));
    DevBuf<int64_t> part;       // (a workspace of this call: readers run side by side)
    TRY(part.alloc(3 * (size_t)kCountBlocks));
    int nb = 0;
    HIP_TRY(launch_count_nonzeros(m->Kp, m->V.p, m->w.p, m->n1, m->k, m->pack_k(), part.p, &nb, m->stream));
    std::vector<int64_t> h(3 * (size_t)nb);
    HIP_TRY(hipMemcpyAsync(h.data(), part.p, h.size() * sizeof(int64_t), hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    int64_t t[3] = {0, 0, 0};
    for (int b = 0; b < nb; ++b)
        for (int j = 0; j < 3; ++j) t[j] += h[3 * (size_t)b + j];
    if (w_nonzero) *w_nonzero = t[0];
    if (v_nonzero) *v_nonzero = t[1];
    if (features_all_zero) *features_all_zero = t[2];
    return FMHIP_OK;
}

int fmhip_model_init_normal(fmhip_model_t m, uint64_t seed, double mean, double stdev) {
    WriteLock lock(m);
    if (!m) return fail(FMHIP_ERR_INVALID, "model is NULL");
    TRY(set_device(m->device));
    HIP_TRY(launch_init_normal(m->Kp, m->V.p, m->w.p, m->w0.p, m->n1, m->n1p, m->k, seed, (float)mean, (float)stdev, m->stream));
    TRY(ftrl_rederive(m));
    HIP_TRY(hipStreamSynchronize(m->stream));
    m->sv = m->sw = 1.0;
    m->host64_fresh = false;     // the device holds the parameters; the fp64 masters are refreshed on demand
    std::vector<double>().swap(m->h_w);
    std::vector<double>().swap(m->h_v);
    return FMHIP_OK;
}

int fmhip_model_get_rows(fmhip_model_t m, int64_t n, const int32_t *ids, double *w, double *v) {
    ReadLock lock(m);
    if (!m || n < 0 || (n > 0 && !ids)) return fail(FMHIP_ERR_INVALID, "NULL argument or negative count");
    for (int64_t j = 0; j < n; ++j)
        if (ids[j] < 0 || ids[j] > m->n) return fail(FMHIP_ERR_SHAPE, "feature id %d outside [0, %lld]", ids[j], (long long)m->n);
    if (n == 0) return FMHIP_OK;
    if (m->host64_fresh) {   // nothing has trained in fp32 since the masters were written: the exact fp64 values, as get_params
        for (int64_t j = 0; j < n; ++j) {
            if (w) w[j] = m->h_w[(size_t)ids[j]];
            if (v)
                for (int f = 0; f < m->k; ++f) v[f + j * (int64_t)m->k] = m->h_v[(size_t)f + (size_t)ids[j] * m->k];
        }
        return FMHIP_OK;
    }
    TRY(set_device(m->device));
    DevBuf<int32_t> dids;
    DevBuf<float> dv, dw;
    TRY(dids.alloc((size_t)n));
    TRY(dv.alloc((size_t)n * m->Kp));
    TRY(dw.alloc((size_t)n));
    HIP_TRY(hipMemcpyAsync(dids.p, ids, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, m->stream));
    HIP_TRY(launch_gather_rows(m->Kp, m->V.p, m->w.p, dids.p, n, dv.p, dw.p, m->stream));
    std::vector<float> hv((size_t)n * m->Kp), hw((size_t)n);
    HIP_TRY(hipMemcpyAsync(hv.data(), dv.p, hv.size() * sizeof(float), hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipMemcpyAsync(hw.data(), dw.p, hw.size() * sizeof(float), hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    table_unpack(m, hv.data(), hw.data(), n, m->sw, m->sv, w, v);       // scales of a lazily decayed model: as get_params
    return FMHIP_OK;
}

int fmhip_model_set_params(fmhip_model_t m, double w0, const double *w, const double *v) {
    WriteLock lock(m);
    return set_params_impl<double>(m, w0, w, v);
}
int fmhip_model_get_params(fmhip_model_t m, double *w0, double *w, double *v) {
    ReadLock lock(m);
    return get_params_impl<double>(m, w0, w, v);
}
int fmhip_model_set_params_f32(fmhip_model_t m, float w0, const float *w, const float *v) {
    WriteLock lock(m);
    return set_params_impl<float>(m, w0, w, v);
}
int fmhip_model_get_params_f32(fmhip_model_t m, float *w0, float *w, float *v) {
    ReadLock lock(m);
    return get_params_impl<float>(m, w0, w, v);
}

int fmhip_synchronize(fmhip_model_t m) {
    ReadLock lock(m);
    if (!m) return fail(FMHIP_ERR_INVALID, "model is NULL");
    TRY(set_device(m->device));
    HIP_TRY(hipStreamSynchronize(m->stream));
    return FMHIP_OK;
}

// ---- training

int fmhip_sgd_step(fmhip_model_t m, fmhip_dataset_t d, int64_t batch, double eta, double reg0, double regw,
                   double regv, fmhip_stats *stats) {
    WriteLock lock(m);
    TRY(check_train(m, d));
    TRY(check_batch(d, batch));
    const Sgd sgd{eta, reg0, regw, regv};
    FusedPlan fp{};
    const bool fused = plan_fused(m, d, batch, sgd, &fp);
    TRY(step_compute(m, d, batch, nullptr, fused ? &fp : nullptr));
    if (stats) {
        memset(stats, 0, sizeof *stats);
        TRY(read_scal(m, stats));
        stats->nnz = d->batches[(size_t)batch].nnz_total;
        stats->steps = 1;
    }
    return fused ? finish_fused(m, fp) : step_apply(m, sgd, d, batch);
}

int fmhip_sgd_epoch(fmhip_model_t m, fmhip_dataset_t d, double eta, double reg0, double regw, double regv,
                    const int64_t *order, fmhip_stats *stats) {
    WriteLock lock(m);
    TRY(check_train(m, d));
    const int64_t nb = (int64_t)d->batches.size();
    if (order)
        for (int64_t j = 0; j < nb; ++j) TRY(check_batch(d, order[j]));
    HIP_TRY(hipMemsetAsync(m->acc.p, 0, 4 * sizeof(double), m->stream));
    const Sgd sgd{eta, reg0, regw, regv};
    for (int64_t j = 0; j < nb; ++j) {
        const int64_t b = order ? order[j] : j;
        FusedPlan fp{};
        const bool fused = plan_fused(m, d, b, sgd, &fp);
        TRY(step_compute(m, d, b, m->acc.p, fused ? &fp : nullptr));
        TRY(fused ? finish_fused(m, fp) : step_apply(m, sgd, d, b));
    }
    if (stats) {
        memset(stats, 0, sizeof *stats);
        TRY(read_acc(m, stats));
        stats->nnz = d->nnz;
        stats->steps = nb;
    }
    return FMHIP_OK;
}

int fmhip_batch_grad(fmhip_model_t m, fmhip_dataset_t d, int64_t batch, double *gv, double *gw, double *gw0,
                     fmhip_stats *stats) {
    WriteLock lock(m);
    TRY(check_train(m, d));
    TRY(check_batch(d, batch));
    TRY(step_compute(m, d, batch, nullptr));
    std::vector<float> hG(m->grad_floats()), hV((size_t)m->n1p * m->Kp);
    HIP_TRY(hipMemcpyAsync(hG.data(), m->grad, hG.size() * sizeof(float), hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipMemcpyAsync(hV.data(), m->V.p, hV.size() * sizeof(float), hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipMemsetAsync(m->grad, 0, m->grad_floats() * sizeof(float), m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    m->step.grad_consumed();
    const float *sc = hG.data(), *Gw = sc + kGradHead, *Gb = Gw + m->n1p, *GV = sc + m->head_floats();
    for (int64_t i = 0; i < m->n1; ++i) {
        if (gw) gw[i] = table_w(m, GV, Gw, i);
        if (gv)
            for (int f = 0; f < m->k; ++f)
                gv[f + i * (int64_t)m->k] = (double)GV[(size_t)i * m->Kp + f] - (double)hV[(size_t)i * m->Kp + f] * m->sv * (double)Gb[i];
    }
    if (gw0) *gw0 = sc[0];
    if (stats) {
        memset(stats, 0, sizeof *stats);
        fill_stats(stats, sc);
        stats->nnz = d->batches[(size_t)batch].nnz_total;
    }
    return FMHIP_OK;
}

// ---- ALS (the reference's own learner), fp64

int fmhip_als_epoch(fmhip_model_t m, fmhip_dataset_t d, double reg0, double regw, double regv) {
    WriteLock lock(m);
    AlsArgs a{};
    TRY(als_begin(m, d, reg0, regw, regv, &a));
    if (d->n_rows > 0) HIP_TRY(launch_als_epoch(a, als_plan(d), m->stream));
    return als_end(m);
}

// ---- data-parallel split step

int fmhip_grad_floats(fmhip_model_t m, int64_t *n_floats) {
    ReadLock lock(m);
    if (!m || !n_floats) return fail(FMHIP_ERR_INVALID, "NULL argument");
    *n_floats = (int64_t)m->grad_floats();
    return FMHIP_OK;
}

int fmhip_grad_bind(fmhip_model_t m, void *device_ptr) {
    WriteLock lock(m);
    if (!m) return fail(FMHIP_ERR_INVALID, "model is NULL");
    if (device_ptr && (reinterpret_cast<uintptr_t>(device_ptr) & 15u))
        return fail(FMHIP_ERR_INVALID, "gradient buffer must be 16-byte aligned");
    m->grad = device_ptr ? static_cast<float *>(device_ptr) : m->grad_own.p;
    m->step.grad_consumed();      // (taken as clean: the buffer itself is not touched)
    return FMHIP_OK;
}

int fmhip_grad_ptr(fmhip_model_t m, void **device_ptr) {
    ReadLock lock(m);
    if (!m || !device_ptr) return fail(FMHIP_ERR_INVALID, "NULL argument");
    *device_ptr = m->grad;
    return FMHIP_OK;
}

int fmhip_step_compute(fmhip_model_t m, fmhip_dataset_t d, int64_t batch) {
    WriteLock lock(m);
    TRY(check_train(m, d));
    TRY(check_batch(d, batch));
    return step_compute(m, d, batch, nullptr);
}

int fmhip_step_forward(fmhip_model_t m, fmhip_dataset_t d, int64_t batch) {
    WriteLock lock(m);
    TRY(check_train(m, d));
    TRY(check_batch(d, batch));
    return step_forward(m, d, batch);
}

int fmhip_step_forward_pass(fmhip_model_t m, fmhip_dataset_t d, int64_t batch, int pass) {
    WriteLock lock(m);
    TRY(check_train(m, d));
    TRY(check_batch(d, batch));
    if (pass != 0 && pass != 1) return fail(FMHIP_ERR_INVALID, "pass must be 0 (features below the cut) or 1 (the others, and the row's finish)");
    return step_forward_pass(m, d, batch, pass);
}

int fmhip_step_backward(fmhip_model_t m, fmhip_dataset_t d, int64_t batch, int64_t feat_lo, int64_t feat_hi, int finish) {
    WriteLock lock(m);
    TRY(check_train(m, d));
    TRY(check_batch(d, batch));
    if (feat_lo < 0 || feat_hi < feat_lo) return fail(FMHIP_ERR_INVALID, "bad feature interval [%lld, %lld)", (long long)feat_lo, (long long)feat_hi);
    // (the tiling rule — descending, or ascending from feature 0 — is bw_window_step's, fmhip_host.h)
    const BwVerdict v = bw_window_step(m->step.bw, m->n1, feat_lo, feat_hi, finish != 0);
    if (v.refusal != BwRefusal::kNone) return fail(FMHIP_ERR_INVALID, "%s", bw_refusal_text(v).c_str());
    TRY(step_backward(m, d, batch, feat_lo, feat_hi, finish != 0, nullptr, nullptr, v.own));
    m->step.backward_walked(v.next);
    return FMHIP_OK;
}

int fmhip_grad_layout(fmhip_model_t m, int64_t *row_floats, int64_t *gv_offset) {
    ReadLock lock(m);
    if (!m) return fail(FMHIP_ERR_INVALID, "model is NULL");
    if (row_floats) *row_floats = m->Kp;
    if (gv_offset) *gv_offset = (int64_t)m->head_floats();
    return FMHIP_OK;
}

int fmhip_step_apply(fmhip_model_t m, double eta, double reg0, double regw, double regv) {
    WriteLock lock(m);
    if (!m) return fail(FMHIP_ERR_INVALID, "model is NULL");
    TRY(set_device(m->device));
    return step_apply(m, Sgd{eta, reg0, regw, regv});
}

int fmhip_step_stats(fmhip_model_t m, fmhip_stats *stats) {
    WriteLock lock(m);
    if (!m || !stats) return fail(FMHIP_ERR_INVALID, "NULL argument");
    TRY(set_device(m->device));
    memset(stats, 0, sizeof *stats);
    TRY(read_scal(m, stats));
    stats->nnz = m->step.last_nnz;
    stats->steps = 1;
    return FMHIP_OK;
}

// ---- measurement

static int profile_begin(fmhip_model_t m, bool rotate, int period) {
    if (!m) return fail(FMHIP_ERR_INVALID, "model is NULL");
    if (period < 1) return fail(FMHIP_ERR_INVALID, "period must be >= 1");
    WriteLock lock(m);
    for (auto &r : m->prof) {
        (void)hipEventDestroy(r.a);
        (void)hipEventDestroy(r.b);
    }
    m->prof.clear();
    m->profiling = true;
    m->prof_rotate = rotate;
    m->prof_period = period;
    m->prof_step = 0;
    return FMHIP_OK;
}

int fmhip_profile_begin(fmhip_model_t m) { return profile_begin(m, false, 1); }
int fmhip_profile_begin_rotating(fmhip_model_t m) { return profile_begin(m, true, 1); }
int fmhip_profile_begin_sampled(fmhip_model_t m, int period) { return profile_begin(m, true, period); }

int fmhip_profile_end(fmhip_model_t m, fmhip_profile *p) {
    WriteLock lock(m);
    if (!m || !p) return fail(FMHIP_ERR_INVALID, "NULL argument");
    TRY(set_device(m->device));
    m->profiling = false;
    memset(p, 0, sizeof *p);
    HIP_TRY(hipStreamSynchronize(m->stream));
    int64_t last_step[FMHIP_K_COUNT];
    for (int64_t &x : last_step) x = -1;
    for (auto &r : m->prof) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
            p->ms[r.kind] += ms;
            p->launches[r.kind] += 1;
            p->nnz[r.kind] += r.nnz;
            p->rows[r.kind] += r.rows;
            if (r.step != last_step[r.kind]) {       // records are in launch order: a new step index = one more timed step
                p->steps[r.kind] += 1;
                last_step[r.kind] = r.step;
            }
        }
        (void)hipEventDestroy(r.a);
        (void)hipEventDestroy(r.b);
    }
    m->prof.clear();
    return FMHIP_OK;
}

}  // extern "C"
