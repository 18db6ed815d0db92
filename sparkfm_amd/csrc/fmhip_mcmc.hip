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
// A handle with attribute groups (include/fmhip_mcmc_groups.h, G > 1) keeps lambda and mu as [(k + 1) x G], takes the groups' sums
// from k_mcmc_group_sums over the plan fmhip_mcmc_set_groups made (fmhip_host.cpp: mcmc_group_plan) — added here in chunk order,
// inside the same single sync — and walks with McmcGroupDev.  G = 1, set or not, is the sequence above, launch for launch: the epoch
// is ONE sequence over the walk's value, and its draws are fmhip_host.h's mcmc_draw_state, which the relational epoch calls too.
// A handle over relational data (include/fmhip_mcmc_relational.h) is made and stepped in fmhip_mcmc_relational.hip; the struct both
// share is fmhip_mcmc_handle.h's, with what the two creators and the two epochs have in common (the settings, the test buffers, the
// flat test set's accumulation, the epoch's end), and every call here but the epoch and set_groups serves it as it serves a flat handle.
// The kernels are in als_kernels.hip, the generator in mcmc_rng.h.
#include "fmhip_internal.h"
#include "fmhip_mcmc_handle.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <new>
#include <vector>

using namespace fmhip;
using namespace fmhip::host;

namespace {

int upload_state(fmhip_mcmc_t s) {
    const size_t k1 = ((size_t)s->k + 1) * (size_t)s->G;
    s->h_hyp[0] = s->alpha;
    std::copy(s->lambda.begin(), s->lambda.end(), s->h_hyp.begin() + 1);
    std::copy(s->mu.begin(), s->mu.end(), s->h_hyp.begin() + 1 + (ptrdiff_t)k1);
    HIP_TRY(hipMemcpyAsync(s->hyp.p, s->h_hyp.data(), s->h_hyp.size() * sizeof(double), hipMemcpyHostToDevice, s->m->stream));
    return FMHIP_OK;
}

// fmhip_mcmc_create (task_opts NULL) and fmhip_mcmc_create_task
int create(fmhip_model_t m, fmhip_dataset_t train, fmhip_dataset_t test, const fmhip_mcmc_opts *opts, const fmhip_mcmc_task_opts *task_opts,
           fmhip_mcmc_t *out) {
    if (!out) return fail(FMHIP_ERR_INVALID, "out is NULL");
    *out = nullptr;
    fmhip_mcmc_opts o;
    fmhip_mcmc_task_opts to;
    TRY(mcmc_settings(opts, task_opts, &o, &to));
    if (!m || !train) return fail(FMHIP_ERR_INVALID, "model or train set is NULL");
    ReadLock lock(m);
    TRY(als_check(m, train));
    if (test) TRY(mcmc_check_test(m, test));
    fmhip_mcmc *s = new (std::nothrow) fmhip_mcmc;
    if (!s) return fail(FMHIP_ERR_NOMEM, "out of host memory");
    std::unique_ptr<fmhip_mcmc> guard(s);
    mcmc_fill(s, m, o, to);
    s->train = train;
    s->test = test;
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
    if (test) TRY(mcmc_alloc_test(s, test->n_rows));
    *out = guard.release();
    return FMHIP_OK;
}

// dst frees what it held and owns src's buffer
template <class T>
void take(DevBuf<T> &dst, DevBuf<T> &src) {
    dst.release();
    dst.p = src.p;
    dst.n = src.n;
    src.p = nullptr;
    src.n = 0;
}

// lambda, mu: (k + 1) * G values each (the caller holds the model's lock)
int get_state(fmhip_mcmc_t s, double *alpha, double *lambda, double *mu, int64_t *iterations) {
    if (alpha) *alpha = s->alpha;
    if (lambda) std::copy(s->lambda.begin(), s->lambda.end(), lambda);
    if (mu) std::copy(s->mu.begin(), s->mu.end(), mu);
    if (iterations) *iterations = s->iterations;
    return FMHIP_OK;
}

// the rows of the handle's test set, flat or relational (-1: none)
int64_t test_rows(fmhip_mcmc_t s) {
    if (s->test) return s->test->n_rows;
    if (s->rel && s->rel->test) return s->rel->test->n_rows;
    return -1;
}

int set_state(fmhip_mcmc_t s, double alpha, const double *lambda, const double *mu) {
    if (!(std::isfinite(alpha) && alpha > 0.0)) return fail(FMHIP_ERR_INVALID, "alpha must be finite and > 0");
    const int G = s->G;
    for (int g = 0; g <= s->k; ++g)
        for (int a = 0; a < G; ++a) {
            const size_t at = (size_t)g * G + a;
            char name[32];
            if (G > 1) snprintf(name, sizeof name, "[%d][%d]", g, a);
            else snprintf(name, sizeof name, "[%d]", g);
            if (!(std::isfinite(lambda[at]) && lambda[at] > 0.0)) return fail(FMHIP_ERR_INVALID, "lambda%s must be finite and > 0", name);
            if (!std::isfinite(mu[at])) return fail(FMHIP_ERR_INVALID, "mu%s must be finite", name);
        }
    s->alpha = alpha;
    s->lambda.assign(lambda, lambda + s->lambda.size());
    s->mu.assign(mu, mu + s->mu.size());
    return FMHIP_OK;
}

}  // namespace

namespace fmhip {
namespace host {

int mcmc_settings(const fmhip_mcmc_opts *opts, const fmhip_mcmc_task_opts *task_opts, fmhip_mcmc_opts *o, fmhip_mcmc_task_opts *to) {
    fmhip_mcmc_opts_default(o);
    if (opts) *o = *opts;
    const McmcPriors pri{o->alpha_0, o->beta_0, o->alpha_lambda, o->beta_lambda, o->gamma_0, o->mu_0};
    if (const char *bad = mcmc_bad_setting(pri, o->reg0, o->init_lambda))
        return fail(FMHIP_ERR_INVALID, "%s must be finite and > 0 (mu_0: finite; reg0: finite and >= 0)", bad);
    fmhip_mcmc_task_opts_default(to);
    if (task_opts) *to = *task_opts;
    if (const char *bad = mcmc_bad_task(to->task, to->clip, to->clip_lo, to->clip_hi)) return fail(FMHIP_ERR_INVALID, "%s", bad);
    return FMHIP_OK;
}

int mcmc_check_test(fmhip_model_t m, fmhip_dataset_t test) {
    if (test->device != m->device) return fail(FMHIP_ERR_INVALID, "model on device %d, test set on device %d", m->device, test->device);
    if (test->dimension > m->n)
        return fail(FMHIP_ERR_INVALID, "the test set has feature index %lld but the model has num_attribute = %lld", (long long)test->dimension,
                    (long long)m->n);
    if (test->batches.size() > 1 || (test->nnz > 0 && !test->val64.p))
        return fail(FMHIP_ERR_UNSUPPORTED, "the MCMC learner predicts its test rows in fp64: create the test set with fmhip_dataset_create and "
                                           "batch_rows <= 0 (single batch; fmhip_rows_create keeps no fp64 rows)");
    return FMHIP_OK;
}

void mcmc_fill(fmhip_mcmc_t s, fmhip_model_t m, const fmhip_mcmc_opts &o, const fmhip_mcmc_task_opts &to) {
    s->m = m;
    s->opts = o;
    s->priors = McmcPriors{o.alpha_0, o.beta_0, o.alpha_lambda, o.beta_lambda, o.gamma_0, o.mu_0};
    s->task = to.task;
    if (to.task == FMHIP_MCMC_CLASSIFICATION) s->link.kind = kLinkProbit;
    else if (to.clip) s->link = McmcLink{kLinkClamp, to.clip_lo, to.clip_hi};
    s->k = m->k;
}

int mcmc_alloc_test(fmhip_mcmc_t s, int64_t n_rows) {
    const size_t nt = (size_t)std::max<int64_t>(n_rows, 1);
    for (DevBuf<double> *b : {&s->test_sum, &s->test_last, &s->test_zero}) {
        TRY(b->alloc(nt));
        HIP_TRY(hipMemset(b->p, 0, nt * sizeof(double)));
    }
    return FMHIP_OK;
}

int mcmc_accumulate_flat_test(fmhip_mcmc_t s) {
    AlsArgs ta{};
    ta.k = s->k;
    ta.n_rows = s->test->n_rows;
    ta.row_ptr = s->test->row_ptr.p;
    ta.col = s->test->col.p;
    ta.val = s->test->val64.p;
    ta.w0 = s->m->als_w0.p;
    ta.w = s->m->als_w.p;
    ta.v = s->m->als_v.p;
    ta.y = s->test_zero.p;
    ta.e = s->test_last.p;
    HIP_TRY(launch_mcmc_accumulate(ta, s->test_sum.p, s->m->stream, s->link));
    return FMHIP_OK;
}

int mcmc_finish_epoch(fmhip_mcmc_t s, double train_rmse, fmhip_mcmc_stats *stats) {
    TRY(als_end(s->m));
    ++s->iterations;
    ++s->draws;
    if (stats) {
        stats->alpha = s->alpha;
        stats->train_rmse = train_rmse;
        stats->iterations = s->iterations;
    }
    return FMHIP_OK;
}

}  // namespace host
}  // namespace fmhip

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
    if (s->rel) return mcmc_relational_epoch(s, stats);
    fmhip_model_t m = s->m;
    fmhip_dataset_t d = s->train;
    WriteLock lock(m);
    if (m->k != s->k) return fail(FMHIP_ERR_INVALID, "the model's k changed under the MCMC handle");
    AlsArgs a{};
    TRY(als_begin(m, d, s->opts.reg0, 0.0, 0.0, &a));       // (what the handle was created for may have changed: checked again)
    const int k1 = s->k + 1, P = kMcmcSumParts, G = s->G;
    const bool probit = s->task == FMHIP_MCMC_CLASSIFICATION;
    const uint32_t t = (uint32_t)s->iterations;
    double sse = 0.0;
    // The epoch's launches for the walk's value `dev`: a McmcDev, or with attribute groups a McmcGroupDev and the plan of its
    // sums — which then come from k_mcmc_group_sums' chunks, not from k_mcmc_sums' quantities 1 + g.  Nothing else differs.
    const auto run = [&](const auto &dev, const McmcGroupSums *groups) -> int {
        TRY(upload_state(s));                                // the means the sums are taken around
        const McmcProbit targets{d->y64.p, s->ystar.p, s->iterations == 0 ? kProbitStart : dev.sample ? kProbitSample : kProbitMean};
        if (probit) a.y = s->ystar.p;                        // the whole epoch trains on the latent targets
        HIP_TRY(launch_mcmc_begin(a, dev, s->z.p, s->opts.seed, t, s->sums.p, m->stream, probit ? &targets : nullptr, groups));
        HIP_TRY(hipMemcpyAsync(s->h_sums.data(), s->sums.p, (groups ? 2 * (size_t)P : s->h_sums.size()) * sizeof(double), hipMemcpyDeviceToHost, m->stream));
        if (groups && dev.sample && groups->n_chunks > 0)
            HIP_TRY(hipMemcpyAsync(s->h_gsums.data(), s->gsums.p, s->h_gsums.size() * sizeof(double), hipMemcpyDeviceToHost, m->stream));
        HIP_TRY(hipStreamSynchronize(m->stream));            // the epoch's one host sync
        for (int c = 0; c < P; ++c) sse += s->h_sums[2 * (size_t)c];
        if (dev.sample) {
            const auto count_of = [&](int ag) { return groups ? s->plan.counts[(size_t)ag] : s->n_trained; };
            const auto partials_of = [&](int g, int ag, auto add) {
                if (groups)      // the group's chunks in order; none: a draw from the prior
                    for (int c = s->plan.group_chunks[(size_t)ag]; c < s->plan.group_chunks[(size_t)ag + 1]; ++c)
                        add(s->h_gsums[2 * ((size_t)c * k1 + g)], s->h_gsums[2 * ((size_t)c * k1 + g) + 1]);
                else
                    for (int c = 0; c < P; ++c) add(s->h_sums[2 * ((size_t)(1 + g) * P + c)], s->h_sums[2 * ((size_t)(1 + g) * P + c) + 1]);
            };
            mcmc_draw_state(s->opts.seed, t, s->priors, probit, d->n_rows, sse, k1, G, count_of, partials_of, &s->alpha, s->lambda.data(), s->mu.data());
            TRY(upload_state(s));
        }
        HIP_TRY(launch_mcmc_sweeps(a, dev, als_plan(d), m->stream));
        return FMHIP_OK;
    };
    const McmcDev flat{s->hyp.p, s->z.p, s->opts.sample ? 1 : 0, 0};
    if (d->n_rows > 0 && G > 1) {
        if (a.n_cols != s->plan_cols)
            return fail(FMHIP_ERR_INVALID, "the train set's columns changed under the MCMC handle (%d, the groups were set over %lld)", a.n_cols,
                        (long long)s->plan_cols);
        const McmcGroupSums sums{s->d_order.p, s->d_chunk_ptr.p, s->d_chunk_group.p, (int)s->plan.chunk_group.size(), s->gsums.p};
        TRY(run(McmcGroupDev{flat, s->d_group.p, G}, &sums));
    } else if (d->n_rows > 0) {
        TRY(run(flat, nullptr));
    }
    if (s->test) TRY(mcmc_accumulate_flat_test(s));
    return mcmc_finish_epoch(s, d->n_rows > 0 ? std::sqrt(sse / (double)d->n_rows) : 0.0, stats);
}

int fmhip_mcmc_get_state(fmhip_mcmc_t s, double *alpha, double *lambda, double *mu, int64_t *iterations) {
    if (!s) return fail(FMHIP_ERR_INVALID, "the MCMC handle is NULL");
    ReadLock lock(s->m);
    if (s->G > 1 && (lambda || mu))
        return fail(FMHIP_ERR_INVALID, "this handle has %d attribute groups: its lambda and mu are (k + 1) x %d — read them with fmhip_mcmc_get_group_state",
                    s->G, s->G);
    return get_state(s, alpha, lambda, mu, iterations);
}

int fmhip_mcmc_set_state(fmhip_mcmc_t s, double alpha, const double *lambda, const double *mu) {
    if (!s || !lambda || !mu) return fail(FMHIP_ERR_INVALID, "NULL argument");
    WriteLock lock(s->m);
    if (s->G > 1)
        return fail(FMHIP_ERR_INVALID, "this handle has %d attribute groups: its lambda and mu are (k + 1) x %d — set them with fmhip_mcmc_set_group_state",
                    s->G, s->G);
    return set_state(s, alpha, lambda, mu);
}

int fmhip_mcmc_set_groups(fmhip_mcmc_t s, const int32_t *group, int64_t n, int32_t n_groups) {
    if (!group) return fail(FMHIP_ERR_INVALID, "the group table is NULL");
    if (n_groups < 1) return fail(FMHIP_ERR_INVALID, "n_groups = %d: a handle has at least one attribute group", n_groups);
    if (n_groups > FMHIP_MCMC_MAX_GROUPS)
        return fail(FMHIP_ERR_UNSUPPORTED, "n_groups = %d is above FMHIP_MCMC_MAX_GROUPS = %d", n_groups, FMHIP_MCMC_MAX_GROUPS);
    if (!s) return fail(FMHIP_ERR_INVALID, "the MCMC handle is NULL");
    fmhip_model_t m = s->m;
    WriteLock lock(m);
    if (s->rel)
        return fail(FMHIP_ERR_UNSUPPORTED, "a handle over relational data takes no group table: its attribute groups are its parts "
                                           "(fmhip_mcmc_create_relational with part_groups = 1)");
    if (s->iterations > 0)
        return fail(FMHIP_ERR_INVALID, "the attribute groups are set before the handle's first epoch: this one has completed %lld", (long long)s->iterations);
    if (n != m->n) return fail(FMHIP_ERR_INVALID, "the group table holds n = %lld ids but the model has num_attribute = %lld", (long long)n, (long long)m->n);
    const int64_t bad = mcmc_bad_group(group, n, n_groups);
    if (bad >= 0)
        return fail(FMHIP_ERR_INVALID, "feature %lld has group id %d, outside [0, %d)", (long long)bad, group[bad], n_groups);
    // everything that can fail comes first, into buffers of its own: a refusal leaves the handle as it was
    const size_t k1 = (size_t)s->k + 1, size = k1 * (size_t)n_groups;
    McmcGroupPlan plan;
    DevBuf<int32_t> d_group, d_order, d_chunk_ptr, d_chunk_group;
    DevBuf<double> hyp, gsums;
    if (n_groups > 1) {
        TRY(set_device(m->device));
        const int64_t n_cols = s->train->n_rows > 0 ? s->train->batches[0].n_cols : 0;
        mcmc_group_plan(s->train->h_cfeat.data(), n_cols, m->n, group, n_groups, kMcmcGroupChunk, &plan);
        std::vector<int32_t> padded(group, group + n);
        padded.push_back(0);                                 // quirk Q1's slot: read a step ahead by the walks, never used
        const size_t n_chunks = plan.chunk_group.size();
        TRY(d_group.alloc(padded.size()));
        TRY(d_order.alloc(std::max<size_t>(plan.order.size(), 1)));
        TRY(d_chunk_ptr.alloc(n_chunks + 1));
        TRY(d_chunk_group.alloc(std::max<size_t>(n_chunks, 1)));
        TRY(gsums.alloc(std::max<size_t>(2 * k1 * n_chunks, 1)));
        TRY(hyp.alloc(1 + 2 * size));
        HIP_TRY(hipMemcpy(d_group.p, padded.data(), padded.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        if (!plan.order.empty()) HIP_TRY(hipMemcpy(d_order.p, plan.order.data(), plan.order.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_chunk_ptr.p, plan.chunk_ptr.data(), (n_chunks + 1) * sizeof(int32_t), hipMemcpyHostToDevice));
        if (n_chunks) HIP_TRY(hipMemcpy(d_chunk_group.p, plan.chunk_group.data(), n_chunks * sizeof(int32_t), hipMemcpyHostToDevice));
    } else {
        plan.counts.assign(1, s->n_trained);                 // G = 1: the handle fmhip_mcmc.h describes (its hyp is large enough as it is)
    }
    s->G = n_groups;
    s->plan = std::move(plan);
    s->plan_cols = s->train->n_rows > 0 ? s->train->batches[0].n_cols : 0;
    take(s->d_group, d_group);
    take(s->d_order, d_order);
    take(s->d_chunk_ptr, d_chunk_ptr);
    take(s->d_chunk_group, d_chunk_group);
    take(s->gsums, gsums);
    if (hyp.p) take(s->hyp, hyp);
    s->h_gsums.assign(2 * k1 * s->plan.chunk_group.size(), 0.0);
    s->h_hyp.assign(1 + 2 * size, 0.0);
    s->lambda.assign(size, s->opts.init_lambda);
    s->mu.assign(size, 0.0);
    return FMHIP_OK;
}

int fmhip_mcmc_group_info(fmhip_mcmc_t s, int32_t *n_groups, int64_t *counts) {
    if (!s) return fail(FMHIP_ERR_INVALID, "the MCMC handle is NULL");
    ReadLock lock(s->m);
    if (n_groups) *n_groups = s->G;
    if (counts) {
        if (s->G > 1) std::copy(s->plan.counts.begin(), s->plan.counts.end(), counts);
        else counts[0] = s->n_trained;
    }
    return FMHIP_OK;
}

int fmhip_mcmc_get_group_state(fmhip_mcmc_t s, double *alpha, double *lambda, double *mu, int64_t *iterations) {
    if (!s) return fail(FMHIP_ERR_INVALID, "the MCMC handle is NULL");
    ReadLock lock(s->m);
    return get_state(s, alpha, lambda, mu, iterations);
}

int fmhip_mcmc_set_group_state(fmhip_mcmc_t s, double alpha, const double *lambda, const double *mu) {
    if (!s || !lambda || !mu) return fail(FMHIP_ERR_INVALID, "NULL argument");
    WriteLock lock(s->m);
    return set_state(s, alpha, lambda, mu);
}

int fmhip_mcmc_reset_average(fmhip_mcmc_t s) {
    if (!s) return fail(FMHIP_ERR_INVALID, "the MCMC handle is NULL");
    WriteLock lock(s->m);
    TRY(set_device(s->m->device));
    if (test_rows(s) >= 0) {
        HIP_TRY(hipMemsetAsync(s->test_sum.p, 0, s->test_sum.n * sizeof(double), s->m->stream));
        HIP_TRY(hipStreamSynchronize(s->m->stream));
    }
    s->draws = 0;
    return FMHIP_OK;
}

int fmhip_mcmc_predictions(fmhip_mcmc_t s, double *mean, double *last, int64_t *draws) {
    if (!s) return fail(FMHIP_ERR_INVALID, "the MCMC handle is NULL");
    if (test_rows(s) < 0) return fail(FMHIP_ERR_INVALID, "the MCMC handle was created without a test set");
    ReadLock lock(s->m);
    TRY(set_device(s->m->device));
    const size_t n = (size_t)test_rows(s);
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
    const size_t n = (size_t)(s->rel ? s->rel->train->n_rows : s->train->n_rows);
    const bool drawn = s->task == FMHIP_MCMC_CLASSIFICATION && s->iterations > 0;
    const double *labels = s->rel ? s->rel->train->y64.p : s->train->y64.p;
    if (n) HIP_TRY(hipMemcpy(out, drawn ? s->ystar.p : labels, n * sizeof(double), hipMemcpyDeviceToHost));
    return FMHIP_OK;
}

}  // extern "C"
