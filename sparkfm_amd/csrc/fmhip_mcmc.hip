// fmhip_mcmc.hip — the MCMC learner (include/fmhip_mcmc.h): the handle and the launch sequence of one Gibbs sweep, a sibling of
// fmhip_als_epoch (fmhip_api.hip), whose checks, uploads and read-back it shares (als_begin / als_end):
//     masters -> device, the state the epoch starts from -> hyp
//     k_mcmc_noise (the whole epoch's N(0,1), chip-wide, first) -> k_als_residual -> k_mcmc_sums -> THE epoch's one host sync
//     host: alpha, every lambda_g and mu_g (fmhip_host.cpp: mcmc_draw_alpha / mcmc_draw_group) -> hyp
//     the bias draw, the residuals again, q, the sweeps: launch_als_epoch's plan with the draw in computeTheta's place
//     k_als_residual over the test rows (labels of zero) + k_mcmc_accumulate -> the parameters back into the model
// A classification handle (include/fmhip_mcmc_task.h) differs in three places: k_mcmc_probit_targets stands where the first
// k_als_residual stood and fills the latent targets ystar, which the walk's y points at for the whole epoch; alpha is not drawn;
// the test rows' accumulation takes Phi of the score (a regression handle with a clip: the clamp).
// The kernels are in als_kernels.hip, the generator in mcmc_rng.h.
#include "fmhip_internal.h"
#include "als_kernels.h"
#include "../../include/fmhip_mcmc_task.h"

#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

using namespace fmhip;
using namespace fmhip::host;

struct fmhip_mcmc {
    fmhip_model_t m = nullptr;
    fmhip_dataset_t train = nullptr, test = nullptr;
    fmhip_mcmc_opts opts{};
    int32_t task = FMHIP_MCMC_REGRESSION;
    McmcLink link;                          // what a draw's test prediction becomes before it joins the sum
    McmcPriors priors;
    int32_t k = 0;
    int64_t n_trained = 0;                  // |T|: the column slots with id < num_attribute
    double alpha = 1.0;
    std::vector<double> lambda, mu;         // [k + 1]
    int64_t iterations = 0, draws = 0;
    DevBuf<double> z, hyp, sums;            // the epoch's noise; {alpha, lambda, mu}; k_mcmc_sums' partials
    DevBuf<double> ystar;                   // classification: the latent targets the last epoch trained on [train rows]
    DevBuf<double> test_sum, test_last, test_zero;     // [test rows]: the running sum, the last draw's predictions, zeros
    std::vector<double> h_sums, h_hyp;
};

namespace {

int upload_state(fmhip_mcmc_t s) {
    const size_t k1 = (size_t)s->k + 1;
    s->h_hyp[0] = s->alpha;
    std::copy(s->lambda.begin(), s->lambda.end(), s->h_hyp.begin() + 1);
    std::copy(s->mu.begin(), s->mu.end(), s->h_hyp.begin() + 1 + (ptrdiff_t)k1);
    HIP_TRY(hipMemcpyAsync(s->hyp.p, s->h_hyp.data(), s->h_hyp.size() * sizeof(double), hipMemcpyHostToDevice, s->m->stream));
    return FMHIP_OK;
}

int check_test(fmhip_model_t m, fmhip_dataset_t test) {
    if (test->device != m->device) return fail(FMHIP_ERR_INVALID, "model on device %d, test set on device %d", m->device, test->device);
    if (test->dimension > m->n)
        return fail(FMHIP_ERR_INVALID, "the test set has feature index %lld but the model has num_attribute = %lld", (long long)test->dimension,
                    (long long)m->n);
    if (test->batches.size() > 1 || (test->nnz > 0 && !test->val64.p))
        return fail(FMHIP_ERR_UNSUPPORTED, "the MCMC learner predicts its test rows in fp64: create the test set with fmhip_dataset_create and "
                                           "batch_rows <= 0 (single batch; fmhip_rows_create keeps no fp64 rows)");
    return FMHIP_OK;
}

// fmhip_mcmc_create (task_opts NULL) and fmhip_mcmc_create_task
int create(fmhip_model_t m, fmhip_dataset_t train, fmhip_dataset_t test, const fmhip_mcmc_opts *opts, const fmhip_mcmc_task_opts *task_opts,
           fmhip_mcmc_t *out) {
    if (!out) return fail(FMHIP_ERR_INVALID, "out is NULL");
    *out = nullptr;
    fmhip_mcmc_opts o;
    fmhip_mcmc_opts_default(&o);
    if (opts) o = *opts;
    const McmcPriors pri{o.alpha_0, o.beta_0, o.alpha_lambda, o.beta_lambda, o.gamma_0, o.mu_0};
    if (const char *bad = mcmc_bad_setting(pri, o.reg0, o.init_lambda))
        return fail(FMHIP_ERR_INVALID, "%s must be finite and > 0 (mu_0: finite; reg0: finite and >= 0)", bad);
    fmhip_mcmc_task_opts to{FMHIP_MCMC_REGRESSION, 0, 0.0, 0.0};
    if (task_opts) to = *task_opts;
    if (const char *bad = mcmc_bad_task(to.task, to.clip, to.clip_lo, to.clip_hi)) return fail(FMHIP_ERR_INVALID, "%s", bad);
    if (!m || !train) return fail(FMHIP_ERR_INVALID, "model or train set is NULL");
    ReadLock lock(m);
    TRY(als_check(m, train));
    if (test) TRY(check_test(m, test));
    fmhip_mcmc *s = new (std::nothrow) fmhip_mcmc;
    if (!s) return fail(FMHIP_ERR_NOMEM, "out of host memory");
    std::unique_ptr<fmhip_mcmc> guard(s);
    s->m = m;
    s->train = train;
    s->test = test;
    s->opts = o;
    s->priors = pri;
    s->task = to.task;
    if (to.task == FMHIP_MCMC_CLASSIFICATION) s->link.kind = kLinkProbit;
    else if (to.clip) s->link = McmcLink{kLinkClamp, to.clip_lo, to.clip_hi};
    s->k = m->k;
    const size_t k1 = (size_t)m->k + 1;
    s->lambda.assign(k1, o.init_lambda);
    s->mu.assign(k1, 0.0);
    s->h_hyp.assign(1 + 2 * k1, 0.0);
    s->h_sums.assign(2 * (k1 + 1) * (size_t)kMcmcSumParts, 0.0);
    const int64_t n_cols = train->n_rows > 0 ? train->batches[0].n_cols : 0;
    for (int64_t c = 0; c < n_cols; ++c) s->n_trained += train->h_cfeat[(size_t)c] < m->n;
    const size_t nz = k1 * (size_t)n_cols + 1;
    TRY(s->z.alloc(nz));
    TRY(s->hyp.alloc(s->h_hyp.size()));
    TRY(s->sums.alloc(s->h_sums.size()));
    HIP_TRY(hipMemset(s->z.p, 0, nz * sizeof(double)));
    if (s->task == FMHIP_MCMC_CLASSIFICATION) TRY(s->ystar.alloc((size_t)std::max<int64_t>(train->n_rows, 1)));
    if (test) {
        const size_t nt = (size_t)std::max<int64_t>(test->n_rows, 1);
        TRY(s->test_sum.alloc(nt));
        TRY(s->test_last.alloc(nt));
        TRY(s->test_zero.alloc(nt));
        HIP_TRY(hipMemset(s->test_sum.p, 0, nt * sizeof(double)));
        HIP_TRY(hipMemset(s->test_last.p, 0, nt * sizeof(double)));
        HIP_TRY(hipMemset(s->test_zero.p, 0, nt * sizeof(double)));
    }
    *out = guard.release();
    return FMHIP_OK;
}

}  // namespace

extern "C" {

int fmhip_mcmc_opts_default(fmhip_mcmc_opts *opts) {
    if (!opts) return fail(FMHIP_ERR_INVALID, "opts is NULL");
    const McmcPriors p;
    *opts = fmhip_mcmc_opts{0, 1, 0.0, 1.0, p.alpha_0, p.beta_0, p.alpha_lambda, p.beta_lambda, p.gamma_0, p.mu_0};
    return FMHIP_OK;
}

int fmhip_mcmc_task_opts_default(fmhip_mcmc_task_opts *task_opts) {
    if (!task_opts) return fail(FMHIP_ERR_INVALID, "task_opts is NULL");
    *task_opts = fmhip_mcmc_task_opts{FMHIP_MCMC_REGRESSION, 0, 0.0, 0.0};
    return FMHIP_OK;
}

int fmhip_mcmc_create(fmhip_model_t m, fmhip_dataset_t train, fmhip_dataset_t test, const fmhip_mcmc_opts *opts, fmhip_mcmc_t *out) {
    return create(m, train, test, opts, nullptr, out);
}

int fmhip_mcmc_create_task(fmhip_model_t m, fmhip_dataset_t train, fmhip_dataset_t test, const fmhip_mcmc_opts *opts,
                           const fmhip_mcmc_task_opts *task_opts, fmhip_mcmc_t *out) {
    return create(m, train, test, opts, task_opts, out);
}

int fmhip_mcmc_destroy(fmhip_mcmc_t s) {
    if (!s) return FMHIP_OK;
    (void)hipSetDevice(s->m->device);
    delete s;
    return FMHIP_OK;
}

int fmhip_mcmc_epoch(fmhip_mcmc_t s, fmhip_mcmc_stats *stats) {
    if (!s) return fail(FMHIP_ERR_INVALID, "the MCMC handle is NULL");
    fmhip_model_t m = s->m;
    fmhip_dataset_t d = s->train;
    WriteLock lock(m);
    if (m->k != s->k) return fail(FMHIP_ERR_INVALID, "the model's k changed under the MCMC handle");
    AlsArgs a{};
    TRY(als_begin(m, d, s->opts.reg0, 0.0, 0.0, &a));       // (what the handle was created for may have changed: checked again)
    const int k1 = s->k + 1, P = kMcmcSumParts;
    const bool probit = s->task == FMHIP_MCMC_CLASSIFICATION;
    const uint32_t t = (uint32_t)s->iterations;
    double sse = 0.0;
    if (d->n_rows > 0) {
        const McmcDev dev{s->hyp.p, s->z.p, s->opts.sample ? 1 : 0, 0};
        TRY(upload_state(s));                                // the means the sums are taken around
        const McmcProbit targets{d->y64.p, s->ystar.p, s->iterations == 0 ? kProbitStart : dev.sample ? kProbitSample : kProbitMean};
        if (probit) a.y = s->ystar.p;                        // the whole epoch trains on the latent targets
        HIP_TRY(launch_mcmc_begin(a, dev, s->z.p, s->opts.seed, t, s->sums.p, m->stream, probit ? &targets : nullptr));
        HIP_TRY(hipMemcpyAsync(s->h_sums.data(), s->sums.p, s->h_sums.size() * sizeof(double), hipMemcpyDeviceToHost, m->stream));
        HIP_TRY(hipStreamSynchronize(m->stream));
        for (int c = 0; c < P; ++c) sse += s->h_sums[2 * (size_t)c];
        if (dev.sample) {
            if (!probit) s->alpha = mcmc_draw_alpha(s->opts.seed, t, s->priors, d->n_rows, sse);   // (the probit link: alpha stays what the state holds)
            for (int g = 0; g < k1; ++g) {
                double sum_theta = 0.0, sum_dev2 = 0.0;
                for (int c = 0; c < P; ++c) {
                    sum_theta += s->h_sums[2 * ((size_t)(1 + g) * P + c)];
                    sum_dev2 += s->h_sums[2 * ((size_t)(1 + g) * P + c) + 1];
                }
                mcmc_draw_group(s->opts.seed, t, (uint32_t)g, s->priors, s->n_trained, sum_theta, sum_dev2, s->mu[(size_t)g], &s->lambda[(size_t)g],
                                &s->mu[(size_t)g]);
            }
            TRY(upload_state(s));
        }
        const int n_levels = d->als_lev_ptr.empty() ? 0 : (int)d->als_lev_ptr.size() - 1;
        HIP_TRY(launch_mcmc_sweeps(a, dev, d->h_cfeat.data(), d->h_cptr.data(), n_levels ? d->als_lev_ptr.data() : nullptr, d->h_als_lev_cols.data(),
                                   n_levels, m->stream));
    }
    if (s->test) {
        AlsArgs ta{};
        ta.k = s->k;
        ta.n_rows = s->test->n_rows;
        ta.row_ptr = s->test->row_ptr.p;
        ta.col = s->test->col.p;
        ta.val = s->test->val64.p;
        ta.w0 = m->als_w0.p;
        ta.w = m->als_w.p;
        ta.v = m->als_v.p;
        ta.y = s->test_zero.p;
        ta.e = s->test_last.p;
        HIP_TRY(launch_mcmc_accumulate(ta, s->test_sum.p, m->stream, s->link));
    }
    TRY(als_end(m));
    ++s->iterations;
    ++s->draws;
    if (stats) {
        stats->alpha = s->alpha;
        stats->train_rmse = d->n_rows > 0 ? std::sqrt(sse / (double)d->n_rows) : 0.0;
        stats->iterations = s->iterations;
    }
    return FMHIP_OK;
}

int fmhip_mcmc_get_state(fmhip_mcmc_t s, double *alpha, double *lambda, double *mu, int64_t *iterations) {
    if (!s) return fail(FMHIP_ERR_INVALID, "the MCMC handle is NULL");
    ReadLock lock(s->m);
    if (alpha) *alpha = s->alpha;
    if (lambda) std::copy(s->lambda.begin(), s->lambda.end(), lambda);
    if (mu) std::copy(s->mu.begin(), s->mu.end(), mu);
    if (iterations) *iterations = s->iterations;
    return FMHIP_OK;
}

int fmhip_mcmc_set_state(fmhip_mcmc_t s, double alpha, const double *lambda, const double *mu) {
    if (!s || !lambda || !mu) return fail(FMHIP_ERR_INVALID, "NULL argument");
    if (!(std::isfinite(alpha) && alpha > 0.0)) return fail(FMHIP_ERR_INVALID, "alpha must be finite and > 0");
    for (int g = 0; g <= s->k; ++g) {
        if (!(std::isfinite(lambda[g]) && lambda[g] > 0.0)) return fail(FMHIP_ERR_INVALID, "lambda[%d] must be finite and > 0", g);
        if (!std::isfinite(mu[g])) return fail(FMHIP_ERR_INVALID, "mu[%d] must be finite", g);
    }
    WriteLock lock(s->m);
    s->alpha = alpha;
    s->lambda.assign(lambda, lambda + s->k + 1);
    s->mu.assign(mu, mu + s->k + 1);
    return FMHIP_OK;
}

int fmhip_mcmc_reset_average(fmhip_mcmc_t s) {
    if (!s) return fail(FMHIP_ERR_INVALID, "the MCMC handle is NULL");
    WriteLock lock(s->m);
    TRY(set_device(s->m->device));
    if (s->test) {
        HIP_TRY(hipMemsetAsync(s->test_sum.p, 0, s->test_sum.n * sizeof(double), s->m->stream));
        HIP_TRY(hipStreamSynchronize(s->m->stream));
    }
    s->draws = 0;
    return FMHIP_OK;
}

int fmhip_mcmc_predictions(fmhip_mcmc_t s, double *mean, double *last, int64_t *draws) {
    if (!s) return fail(FMHIP_ERR_INVALID, "the MCMC handle is NULL");
    if (!s->test) return fail(FMHIP_ERR_INVALID, "the MCMC handle was created without a test set");
    ReadLock lock(s->m);
    TRY(set_device(s->m->device));
    const size_t n = (size_t)s->test->n_rows;
    if (mean && n) HIP_TRY(hipMemcpy(mean, s->test_sum.p, n * sizeof(double), hipMemcpyDeviceToHost));
    if (last && n) HIP_TRY(hipMemcpy(last, s->test_last.p, n * sizeof(double), hipMemcpyDeviceToHost));
    if (mean)
        for (size_t r = 0; r < n; ++r) mean[r] = s->draws > 0 ? mean[r] / (double)s->draws : 0.0;
    if (draws) *draws = s->draws;
    return FMHIP_OK;
}

int fmhip_mcmc_latent_targets(fmhip_mcmc_t s, double *out) {
    if (!s || !out) return fail(FMHIP_ERR_INVALID, "the MCMC handle or out is NULL");
    ReadLock lock(s->m);
    TRY(set_device(s->m->device));
    const size_t n = (size_t)s->train->n_rows;
    const bool drawn = s->task == FMHIP_MCMC_CLASSIFICATION && s->iterations > 0;
    if (n) HIP_TRY(hipMemcpy(out, drawn ? s->ystar.p : s->train->y64.p, n * sizeof(double), hipMemcpyDeviceToHost));
    return FMHIP_OK;
}

}  // extern "C"
