// fmhip_sgda.hip — the C ABI of the SGDA learner (include/fmhip_sgda.h): the handle (group table, lambda, shadow tables, the plan of
// the grouped sums) and the launch sequence of its step — fmhip_step.hip's pieces around fm_sgda.hip's three kernels.
#include "../../include/fmhip_sgda.h"
#include "fm_sgda.h"
#include "fmhip_internal.h"

#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

using namespace fmhip;
using namespace fmhip::host;

static_assert(FMHIP_SGDA_MAX_GROUPS == kSgdaMaxGroups, "fmhip_sgda.h and fmhip_host.h disagree on the group limit");

struct fmhip_sgda {
    template <typename T> using DevBuf = fmhip::host::DevBuf<T>;
    fmhip_model_t m = nullptr;
    int32_t G = 1;
    McmcGroupPlan plan;
    DevBuf<int32_t> group, order, chunk_ptr, group_chunks;
    DevBuf<float> L, Lw, SV, Sw, part;
    DevBuf<double> S, acc_val;
    int64_t steps = 0;
};

namespace {

bool lambda_ok(double x) { return std::isfinite(x) && x >= 0.0; }

// every refusal of a step that depends on the model's rule and the datasets; the model is untouched
int sgda_check(fmhip_sgda_t h, fmhip_dataset_t train, fmhip_dataset_t val, double eta_lambda) {
    if (!h) return fail(FMHIP_ERR_INVALID, "the SGDA handle is NULL");
    fmhip_model_t m = h->m;
    if (m->rule.adagrad() || m->rule.ftrl())
        return fail(FMHIP_ERR_UNSUPPORTED, "SGDA adapts the regularisers of plain SGD: this model is under %s (fmhip_model_set_optimizer(FMHIP_OPT_SGD) first)",
                    m->rule.ftrl() ? "FTRL-Proximal" : "AdaGrad");
    if (m->rule.paired()) return fail(FMHIP_ERR_UNSUPPORTED, "SGDA trains on single rows: this model is set to pairs (fmhip_model_set_pairing)");
    TRY(check_train(m, train));
    if (train->weighted) return fail(FMHIP_ERR_UNSUPPORTED, "SGDA does not take example weights yet (the train set was made by fmhip_dataset_create_weighted)");
    if (!val) {
        if (eta_lambda != 0.0) return fail(FMHIP_ERR_INVALID, "eta_lambda = %g needs a validation set (val is NULL): lambda steps on held-out rows", eta_lambda);
        return FMHIP_OK;
    }
    TRY(check_pair(m, val));
    if (val->scoring_only)
        return fail(FMHIP_ERR_INVALID, "the validation set was created with fmhip_rows_create (scoring only): the lambda step needs its gradient, "
                                       "and so its transposes (fmhip_dataset_create)");
    if (val->weighted) return fail(FMHIP_ERR_UNSUPPORTED, "SGDA does not take example weights yet (the validation set was made by fmhip_dataset_create_weighted)");
    if (val->batches.empty()) return fail(FMHIP_ERR_INVALID, "the validation set has no rows");
    return FMHIP_OK;
}

SgdaArgs sgda_args(fmhip_sgda_t h, double eta, double eta_lambda, double reg0) {
    fmhip_model_t m = h->m;
    SgdaArgs a{};
    a.V = m->V.p;
    a.w = m->w.p;
    a.w0 = m->w0.p;
    a.GV = m->GV();
    a.Gw = m->Gw();
    a.Gb = m->Gb();
    a.scal = m->scal();
    a.n1 = m->n1;
    a.pack_k = m->pack_k();
    a.eta = (float)eta;
    a.reg0 = (float)reg0;
    a.group = h->group.p;
    a.L = h->L.p;
    a.Lw = h->Lw.p;
    a.SV = h->SV.p;
    a.Sw = h->Sw.p;
    a.order = h->order.p;
    a.chunk_ptr = h->chunk_ptr.p;
    a.group_chunks = h->group_chunks.p;
    a.n_chunks = (int32_t)h->plan.chunk_group.size();
    a.n_groups = h->G;
    a.part = h->part.p;
    a.S = h->S.p;
    a.rate = eta_lambda * eta;
    return a;
}

int read_scal_of(fmhip_model_t m, fmhip_dataset_t d, int64_t b, fmhip_stats *st) {
    memset(st, 0, sizeof *st);
    TRY(read_scal(m, st));
    st->nnz = d->batches[(size_t)b].nnz_total;
    st->steps = 1;
    return FMHIP_OK;
}

// one step, asynchronous on the model's stream unless a stats pointer asks for numbers; acc_t / acc_v: the epoch's fp64 accumulators
int sgda_step(fmhip_sgda_t h, fmhip_dataset_t train, int64_t b, fmhip_dataset_t val, int64_t vb, double eta, double eta_lambda, double reg0,
              double *acc_t, double *acc_v, fmhip_stats *st_t, fmhip_stats *st_v) {
    fmhip_model_t m = h->m;
    TRY(fold_scales(m));
    const SgdaArgs a = sgda_args(h, eta, eta_lambda, reg0);
    TRY(step_compute(m, train, b, acc_t));
    if (st_t) TRY(read_scal_of(m, train, b, st_t));
    HIP_TRY(launch_sgda_apply(m->Kp, a, m->stream));
    TRY(finish_fused(m, FusedPlan{}));          // the step's bookkeeping: scale 1, the gradient consumed
    if (val) {
        TRY(step_compute(m, val, vb, acc_v));   // the validation gradient at theta'
        if (st_v) TRY(read_scal_of(m, val, vb, st_v));
        HIP_TRY(launch_sgda_lambda_partials(m->Kp, a, m->stream));
        HIP_TRY(launch_sgda_lambda_step(m->Kp, a, m->stream));
        HIP_TRY(hipMemsetAsync(m->scal(), 0, (size_t)kGradHead * sizeof(float), m->stream));
        m->step.grad_consumed();
    }
    ++h->steps;
    return FMHIP_OK;
}

}  // namespace

extern "C" {

int fmhip_sgda_create(fmhip_model_t m, const int32_t *group, int64_t n, int32_t n_groups, double init_lambda_w, double init_lambda_v,
                      fmhip_sgda_t *out) {
    if (!out) return fail(FMHIP_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!group) return fail(FMHIP_ERR_INVALID, "the group table is NULL");
    if (n_groups < 1) return fail(FMHIP_ERR_INVALID, "n_groups = %d: a handle has at least one feature group", n_groups);
    if (n_groups > FMHIP_SGDA_MAX_GROUPS)
        return fail(FMHIP_ERR_UNSUPPORTED, "n_groups = %d is above FMHIP_SGDA_MAX_GROUPS = %d", n_groups, FMHIP_SGDA_MAX_GROUPS);
    if (!lambda_ok(init_lambda_w) || !lambda_ok(init_lambda_v))
        return fail(FMHIP_ERR_INVALID, "init_lambda_w = %g, init_lambda_v = %g: a regulariser is finite and >= 0", init_lambda_w, init_lambda_v);
    if (!m) return fail(FMHIP_ERR_INVALID, "model is NULL");
    WriteLock lock(m);
    if (n != m->n1)
        return fail(FMHIP_ERR_INVALID, "the group table holds n = %lld ids but the model has num_attribute + 1 = %lld feature rows", (long long)n, (long long)m->n1);
    const int64_t bad = mcmc_bad_group(group, n, n_groups);
    if (bad >= 0) return fail(FMHIP_ERR_INVALID, "feature %lld has group id %d, outside [0, %d)", (long long)bad, group[bad], n_groups);
    if (m->rule.adagrad() || m->rule.ftrl())
        return fail(FMHIP_ERR_UNSUPPORTED, "SGDA adapts the regularisers of plain SGD: this model is under %s", m->rule.ftrl() ? "FTRL-Proximal" : "AdaGrad");
    if (m->rule.paired()) return fail(FMHIP_ERR_UNSUPPORTED, "SGDA trains on single rows: this model is set to pairs (fmhip_model_set_pairing)");
    TRY(set_device(m->device));
    fmhip_sgda *h = new (std::nothrow) fmhip_sgda();
    if (!h) return fail(FMHIP_ERR_NOMEM, "out of host memory");
    h->m = m;
    h->G = n_groups;
    sgda_group_plan(group, n, n_groups, kSgdaChunk, &h->plan);
    const size_t G = (size_t)n_groups, Kp = (size_t)m->Kp, n_chunks = h->plan.chunk_group.size();
    std::vector<float> L(G * Kp, 0.f), Lw(G, (float)init_lambda_w);
    for (size_t a = 0; a < G; ++a) {
        for (int f = 0; f < m->k; ++f) L[a * Kp + (size_t)f] = (float)init_lambda_v;
        if (m->pack_k() >= 0) L[a * Kp + (size_t)m->pack_k()] = (float)init_lambda_w;
    }
    int rc = FMHIP_OK;
    hipError_t e = hipSuccess;
    if ((rc = h->group.alloc((size_t)m->n1p)) || (rc = h->order.alloc(std::max<size_t>(h->plan.order.size(), 1))) ||
        (rc = h->chunk_ptr.alloc(n_chunks + 1)) || (rc = h->group_chunks.alloc(G + 1)) || (rc = h->L.alloc(G * Kp)) || (rc = h->Lw.alloc(G)) ||
        (rc = h->SV.alloc((size_t)m->n1p * Kp)) || (rc = h->Sw.alloc((size_t)m->n1p)) ||
        (rc = h->part.alloc(std::max<size_t>(n_chunks, 1) * (Kp + kSgdaPartPad))) || (rc = h->S.alloc(G * (Kp + kSgdaSlots))) ||
        (rc = h->acc_val.alloc(4))) {
        delete h;
        return rc;
    }
    std::vector<int32_t> padded(group, group + n);
    padded.resize((size_t)m->n1p, 0);
    if (e == hipSuccess) e = hipMemcpy(h->group.p, padded.data(), padded.size() * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess && !h->plan.order.empty())
        e = hipMemcpy(h->order.p, h->plan.order.data(), h->plan.order.size() * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(h->chunk_ptr.p, h->plan.chunk_ptr.data(), (n_chunks + 1) * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(h->group_chunks.p, h->plan.group_chunks.data(), (G + 1) * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(h->L.p, L.data(), L.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(h->Lw.p, Lw.data(), Lw.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(h->SV.p, 0, h->SV.n * sizeof(float));
    if (e == hipSuccess) e = hipMemset(h->Sw.p, 0, h->Sw.n * sizeof(float));
    if (e == hipSuccess) e = hipMemset(h->part.p, 0, h->part.n * sizeof(float));
    if (e == hipSuccess) e = hipMemset(h->S.p, 0, h->S.n * sizeof(double));
    if (e == hipSuccess) e = hipMemset(h->acc_val.p, 0, 4 * sizeof(double));
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        delete h;
        return fail(FMHIP_ERR_HIP, "setting up the SGDA handle failed: %s", hipGetErrorString(e));
    }
    ++m->sgda_handles;
    *out = h;
    return FMHIP_OK;
}

int fmhip_sgda_destroy(fmhip_sgda_t h) {
    if (!h) return FMHIP_OK;
    {
        WriteLock lock(h->m);
        (void)hipSetDevice(h->m->device);
        if (h->m->stream) (void)hipStreamSynchronize(h->m->stream);
        --h->m->sgda_handles;
    }
    delete h;
    return FMHIP_OK;
}

int fmhip_sgda_step(fmhip_sgda_t h, fmhip_dataset_t train, int64_t batch, fmhip_dataset_t val, int64_t val_batch, double eta,
                    double eta_lambda, double reg0, fmhip_stats *stats_train, fmhip_stats *stats_val) {
    if (!h) return fail(FMHIP_ERR_INVALID, "the SGDA handle is NULL");
    WriteLock lock(h->m);
    TRY(sgda_check(h, train, val, eta_lambda));
    TRY(check_batch(train, batch));
    if (val) TRY(check_batch(val, val_batch));
    if (stats_val) memset(stats_val, 0, sizeof *stats_val);
    return sgda_step(h, train, batch, val, val_batch, eta, eta_lambda, reg0, nullptr, nullptr, stats_train, val ? stats_val : nullptr);
}

int fmhip_sgda_epoch(fmhip_sgda_t h, fmhip_dataset_t train, fmhip_dataset_t val, double eta, double eta_lambda, double reg0,
                     const int64_t *order, fmhip_stats *stats_train, fmhip_stats *stats_val) {
    if (!h) return fail(FMHIP_ERR_INVALID, "the SGDA handle is NULL");
    fmhip_model_t m = h->m;
    WriteLock lock(m);
    TRY(sgda_check(h, train, val, eta_lambda));
    const int64_t nb = (int64_t)train->batches.size(), nvb = val ? (int64_t)val->batches.size() : 0;
    if (order)
        for (int64_t j = 0; j < nb; ++j) TRY(check_batch(train, order[j]));
    HIP_TRY(hipMemsetAsync(m->acc.p, 0, 4 * sizeof(double), m->stream));
    HIP_TRY(hipMemsetAsync(h->acc_val.p, 0, 4 * sizeof(double), m->stream));
    int64_t val_nnz = 0;
    for (int64_t j = 0; j < nb; ++j) {
        const int64_t vb = val ? h->steps % nvb : 0;
        if (val) val_nnz += val->batches[(size_t)vb].nnz_total;
        TRY(sgda_step(h, train, order ? order[j] : j, val, vb, eta, eta_lambda, reg0, m->acc.p, val ? h->acc_val.p : nullptr, nullptr, nullptr));
    }
    if (stats_train) {
        memset(stats_train, 0, sizeof *stats_train);
        TRY(read_acc(m, stats_train));
        stats_train->nnz = train->nnz;
        stats_train->steps = nb;
    }
    if (stats_val) {
        memset(stats_val, 0, sizeof *stats_val);
        if (val) {
            double acc[4];
            HIP_TRY(hipMemcpyAsync(acc, h->acc_val.p, sizeof acc, hipMemcpyDeviceToHost, m->stream));
            HIP_TRY(hipStreamSynchronize(m->stream));
            fill_stats(stats_val, acc);
            stats_val->nnz = val_nnz;
            stats_val->steps = nb;
        }
    }
    return FMHIP_OK;
}

int fmhip_sgda_get_lambda(fmhip_sgda_t h, double *lw, double *lv) {
    if (!h) return fail(FMHIP_ERR_INVALID, "the SGDA handle is NULL");
    fmhip_model_t m = h->m;
    WriteLock lock(m);
    TRY(set_device(m->device));
    const size_t G = (size_t)h->G, Kp = (size_t)m->Kp;
    std::vector<float> L(G * Kp), Lw(G);
    HIP_TRY(hipMemcpyAsync(L.data(), h->L.p, L.size() * sizeof(float), hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipMemcpyAsync(Lw.data(), h->Lw.p, Lw.size() * sizeof(float), hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    for (size_t a = 0; a < G; ++a) {
        if (lw) lw[a] = Lw[a];
        if (lv)
            for (int f = 0; f < m->k; ++f) lv[(size_t)f * G + a] = L[a * Kp + (size_t)f];
    }
    return FMHIP_OK;
}

int fmhip_sgda_set_lambda(fmhip_sgda_t h, const double *lw, const double *lv) {
    if (!h) return fail(FMHIP_ERR_INVALID, "the SGDA handle is NULL");
    if (!lw || !lv) return fail(FMHIP_ERR_INVALID, "NULL argument");
    fmhip_model_t m = h->m;
    WriteLock lock(m);
    const size_t G = (size_t)h->G, Kp = (size_t)m->Kp;
    for (size_t a = 0; a < G; ++a) {
        if (!lambda_ok(lw[a])) return fail(FMHIP_ERR_INVALID, "lambda_w of group %zu = %g: a regulariser is finite and >= 0", a, lw[a]);
        for (int f = 0; f < m->k; ++f)
            if (!lambda_ok(lv[(size_t)f * G + a]))
                return fail(FMHIP_ERR_INVALID, "lambda_v of factor %d, group %zu = %g: a regulariser is finite and >= 0", f, a, lv[(size_t)f * G + a]);
    }
    TRY(set_device(m->device));
    std::vector<float> L(G * Kp, 0.f), Lw(G);
    for (size_t a = 0; a < G; ++a) {
        Lw[a] = (float)lw[a];
        for (int f = 0; f < m->k; ++f) L[a * Kp + (size_t)f] = (float)lv[(size_t)f * G + a];
        if (m->pack_k() >= 0) L[a * Kp + (size_t)m->pack_k()] = Lw[a];
    }
    HIP_TRY(hipMemcpyAsync(h->L.p, L.data(), L.size() * sizeof(float), hipMemcpyHostToDevice, m->stream));
    HIP_TRY(hipMemcpyAsync(h->Lw.p, Lw.data(), Lw.size() * sizeof(float), hipMemcpyHostToDevice, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    return FMHIP_OK;
}

int fmhip_sgda_last_sums(fmhip_sgda_t h, double *sw, double *sv) {
    if (!h) return fail(FMHIP_ERR_INVALID, "the SGDA handle is NULL");
    fmhip_model_t m = h->m;
    WriteLock lock(m);
    TRY(set_device(m->device));
    const size_t G = (size_t)h->G, width = (size_t)m->Kp + kSgdaSlots;
    std::vector<double> S(G * width);
    HIP_TRY(hipMemcpyAsync(S.data(), h->S.p, S.size() * sizeof(double), hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    const size_t wslot = m->pack_k() >= 0 ? (size_t)m->pack_k() : (size_t)m->Kp;
    for (size_t a = 0; a < G; ++a) {
        if (sw) sw[a] = S[a * width + wslot];
        if (sv)
            for (int f = 0; f < m->k; ++f) sv[(size_t)f * G + a] = S[a * width + (size_t)f];
    }
    return FMHIP_OK;
}

int fmhip_sgda_info(fmhip_sgda_t h, int32_t *n_groups, int64_t *counts, int64_t *steps) {
    if (!h) return fail(FMHIP_ERR_INVALID, "the SGDA handle is NULL");
    ReadLock lock(h->m);
    if (n_groups) *n_groups = h->G;
    if (counts) std::copy(h->plan.counts.begin(), h->plan.counts.end(), counts);
    if (steps) *steps = h->steps;
    return FMHIP_OK;
}

}  // extern "C"
