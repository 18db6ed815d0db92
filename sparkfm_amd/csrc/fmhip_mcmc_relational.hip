// fmhip_mcmc_relational.hip — the MCMC learner over relational data (include/fmhip_mcmc_relational.h): the handle and the launch
// sequence of one block-structure Gibbs sweep, a sibling of fmhip_mcmc_epoch (fmhip_mcmc.hip):
//     masters -> device, the state the epoch starts from -> hyp (one {alpha, lambda, mu} per part)
//     the parts' noise -> yhat_p and q_p of every block -> the combine (e, Q; probit: the latent targets) -> sum e^2 and the parts'
//     sums of theta -> THE epoch's one host sync -> host: alpha, every lambda and mu -> hyp
//     the bias draw, the blocks' forward and the combine again, then per parameter group the parts in range order: a relation's
//     cache build + column walk + scatter, the plain part's flat pass
//     the test rows (relational: forward + combine; flat: k_als_residual) + the accumulation -> the parameters back into the model
// The kernels are in als_kernels.hip (launchers: mcmc_blocks.h); the host arithmetic — the parts' order, n_p, the trained columns —
// in fmhip_host.cpp.
#include "fmhip_mcmc_handle.h"
#include "mcmc_blocks.h"
#include "../../include/fmhip_mcmc_relational.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <new>
#include <string>
#include <vector>

using namespace fmhip;
using namespace fmhip::host;

static_assert(kBlockPartsMax == FMHIP_RELATIONS_MAX + 1, "mcmc_blocks.h and the public header agree");

namespace {

template <typename T>
int upload(DevBuf<T> &dst, const std::vector<T> &src) {
    TRY(dst.alloc(std::max<size_t>(src.size(), 1)));
    if (!src.empty()) HIP_TRY(hipMemcpy(dst.p, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    return FMHIP_OK;
}

int zeros(DevBuf<double> &dst, size_t n) {
    n = std::max<size_t>(n, 1);
    TRY(dst.alloc(n));
    HIP_TRY(hipMemset(dst.p, 0, n * sizeof(double)));
    return FMHIP_OK;
}

std::string part_name(fmhip_relational_t R, int p) {
    return p < (int)R->rels.size() ? "relation " + std::to_string(p) : std::string("the plain part");
}

int n_parts(fmhip_relational_t R) { return (int)R->rels.size() + (R->plain ? 1 : 0); }
fmhip_dataset_t part_data(fmhip_relational_t R, int p) { return p < (int)R->rels.size() ? R->rels[(size_t)p]->block : R->plain; }

// als_check of one part, the refusal prefixed with the part's name
int check_part(fmhip_model_t m, fmhip_relational_t R, int p, const char *set) {
    const int rc = als_check(m, part_data(R, p));
    if (rc == FMHIP_OK) return rc;
    const std::string why = fmhip_last_error();
    return fail(rc, "%s, %s: %s", set, part_name(R, p).c_str(), why.c_str());
}

int check_relational(fmhip_model_t m, fmhip_relational_t R, const char *set) {
    if (R->device != m->device) return fail(FMHIP_ERR_INVALID, "model on device %d, %s on device %d", m->device, set, R->device);
    if (R->dimension > m->n)
        return fail(FMHIP_ERR_INVALID, "%s has feature index %lld but the model has num_attribute = %lld", set, (long long)R->dimension, (long long)m->n);
    if (R->batches.size() > 1)
        return fail(FMHIP_ERR_UNSUPPORTED, "%s has %zu batches: the MCMC learner walks whole blocks — create the relational dataset with batch_rows <= 0 "
                                           "(one batch)", set, R->batches.size());
    for (int p = 0; p < n_parts(R); ++p) TRY(check_part(m, R, p, set));
    return FMHIP_OK;
}

// per part {alpha, lambda[k + 1], mu[k + 1]}: McmcDev's layout, so that every walk takes the flat handle's step
int upload_state(fmhip_mcmc_t s) {
    McmcRelational &X = *s->rel;
    const size_t k1 = (size_t)s->k + 1, stride = 1 + 2 * k1, G = (size_t)s->G;
    for (size_t p = 0; p < X.parts.size(); ++p) {
        double *h = X.h_hyp.data() + p * stride;
        const size_t ag = X.part_groups ? p : 0;
        h[0] = s->alpha;
        for (size_t g = 0; g < k1; ++g) {
            h[1 + g] = s->lambda[g * G + ag];
            h[1 + k1 + g] = s->mu[g * G + ag];
        }
    }
    HIP_TRY(hipMemcpyAsync(X.hyp.p, X.h_hyp.data(), X.h_hyp.size() * sizeof(double), hipMemcpyHostToDevice, s->m->stream));
    return FMHIP_OK;
}

// yhat_p and (fresh_q) q_p of every part of R, then the combine into e (and Q).  fresh_q = false: only w0 changed since the last
// call over these buffers, and q_p does not depend on it
int residuals(fmhip_mcmc_t s, fmhip_relational_t R, const std::vector<AlsArgs> &fwd, const double *y, double *e, double *Q, const McmcProbit *probit,
              uint32_t t, bool fresh_q = true) {
    fmhip_model_t m = s->m;
    BlockCombine c{};
    c.n_parts = (int32_t)fwd.size();
    c.k = s->k;
    c.n_rows = R->n_rows;
    for (size_t p = 0; p < fwd.size(); ++p) {
        HIP_TRY(launch_block_forward(fwd[p], fresh_q, m->stream));
        c.yhat[p] = fwd[p].e;
        c.q[p] = fwd[p].q;
        c.map[p] = p < R->rels.size() ? R->rels[p]->map.p : nullptr;
        c.J[p] = fwd[p].n_rows;
    }
    c.w0 = m->als_w0.p;
    c.y = y;
    c.e = e;
    c.Q = Q;
    HIP_TRY(launch_block_combine(c, probit, s->opts.seed, t, m->stream));
    return FMHIP_OK;
}

}  // namespace

namespace fmhip {
namespace host {

int mcmc_relational_epoch(fmhip_mcmc_t s, fmhip_mcmc_stats *stats) {
    fmhip_model_t m = s->m;
    McmcRelational &X = *s->rel;
    fmhip_relational_t R = X.train;
    WriteLock lock(m);
    if (m->k != s->k) return fail(FMHIP_ERR_INVALID, "the model's k changed under the MCMC handle");
    TRY(check_relational(m, R, "the train set"));        // (what the handle was created for may have changed: checked again)
    if (X.test) TRY(check_relational(m, X.test, "the test set"));
    AlsArgs first{};
    TRY(als_begin(m, X.parts[0]->d, s->opts.reg0, 0.0, 0.0, &first));      // the fp64 masters onto the device
    const int k1 = s->k + 1, P = kMcmcSumParts, NP = (int)X.parts.size();
    const size_t stride = 1 + 2 * (size_t)k1;
    const bool probit = s->task == FMHIP_MCMC_CLASSIFICATION, sample = s->opts.sample != 0;
    const uint32_t t = (uint32_t)s->iterations;
    const int64_t N = R->n_rows;
    // the parts' arguments: `fwd` writes yhat_p / q_p over labels of zero; the plain part's walk works on e and Q directly
    std::vector<AlsArgs> fwd((size_t)NP);
    for (int p = 0; p < NP; ++p) {
        McmcRelational::Part &part = *X.parts[(size_t)p];
        AlsArgs a = als_args(m, part.d);
        a.reg0 = s->opts.reg0;
        a.y = X.zeros.p;
        a.e = part.yhat.p;
        a.q = part.q.p;
        fwd[(size_t)p] = a;
    }
    AlsArgs rows{};                                      // the data rows: the bias step and sum e^2
    rows.k = s->k;
    rows.n_rows = N;
    rows.e = X.e.p;
    rows.w0 = m->als_w0.p;
    rows.reg0 = s->opts.reg0;
    TRY(upload_state(s));                                // the means the sums are taken around
    if (sample) {
        for (int p = 0; p < NP; ++p) HIP_TRY(launch_mcmc_noise(fwd[(size_t)p], X.parts[(size_t)p]->z.p, s->opts.seed, t, m->stream));
        HIP_TRY(launch_mcmc_noise(rows, X.zbias.p, s->opts.seed, t, m->stream));
    }
    const McmcProbit targets{R->y64.p, s->ystar.p, s->iterations == 0 ? kProbitStart : sample ? kProbitSample : kProbitMean};
    const double *y = probit ? s->ystar.p : R->y64.p;    // the whole epoch trains on the latent targets
    TRY(residuals(s, R, fwd, y, X.e.p, X.Q.p, probit ? &targets : nullptr, t));
    HIP_TRY(launch_block_sse(rows, s->sums.p, m->stream));
    HIP_TRY(hipMemcpyAsync(s->h_sums.data(), s->sums.p, 2 * (size_t)P * sizeof(double), hipMemcpyDeviceToHost, m->stream));
    if (sample)
        for (int p = 0; p < NP; ++p) {
            McmcRelational::Part &part = *X.parts[(size_t)p];
            HIP_TRY(launch_block_theta_sums(fwd[(size_t)p], part.trained.p, X.hyp.p + (size_t)p * stride, part.sums.p, m->stream));
            HIP_TRY(hipMemcpyAsync(part.h_sums.data(), part.sums.p, part.h_sums.size() * sizeof(double), hipMemcpyDeviceToHost, m->stream));
        }
    HIP_TRY(hipStreamSynchronize(m->stream));            // the epoch's one host sync
    double sse = 0.0;
    for (int c = 0; c < P; ++c) sse += s->h_sums[2 * (size_t)c];
    if (sample) {
        // a (g, a)'s partials: every part's chunks in order, the parts in walk order — with part_groups part a's own
        const auto count_of = [&](int ag) { return X.part_groups ? X.parts[(size_t)ag]->n_trained : s->n_trained; };
        const auto partials_of = [&](int g, int ag, auto add) {
            const auto of_part = [&](const McmcRelational::Part &part) {
                for (int c = 0; c < P; ++c) add(part.h_sums[2 * ((size_t)g * P + c)], part.h_sums[2 * ((size_t)g * P + c) + 1]);
            };
            if (X.part_groups) of_part(*X.parts[(size_t)ag]);
            else
                for (int x = 0; x < NP; ++x) of_part(*X.parts[(size_t)X.order[(size_t)x]]);
        };
        mcmc_draw_state(s->opts.seed, t, s->priors, probit, N, sse, k1, s->G, count_of, partials_of, &s->alpha, s->lambda.data(), s->mu.data());
        TRY(upload_state(s));
    }
    // ---- behind the sync: the bias, the residuals again, the sweeps
    HIP_TRY(launch_block_bias(rows, McmcDev{X.hyp.p, X.zbias.p, sample ? 1 : 0, 0}, m->stream));
    TRY(residuals(s, R, fwd, y, X.e.p, nullptr, nullptr, t, false));
    for (int g = 0; g < k1; ++g)
        for (int x = 0; x < NP; ++x) {
            const int p = X.order[(size_t)x];
            McmcRelational::Part &part = *X.parts[(size_t)p];
            fmhip_dataset_t d = part.d;
            const McmcDev dev{X.hyp.p + (size_t)p * stride, part.z.p, sample ? 1 : 0, 0};
            if (part.rel < 0) {
                AlsArgs a = fwd[(size_t)p];
                a.e = X.e.p;
                a.q = X.Q.p;
                HIP_TRY(launch_plain_pass(a, g, dev, als_plan(d), m->stream));
                continue;
            }
            const fmhip_relational::Relation &rel = *R->rels[(size_t)part.rel];
            const RelationInverse::Batch &ib = rel.batches[0];
            BlockPart b{};
            b.a = fwd[(size_t)p];
            b.J = d->n_rows;
            b.n_rows = N;
            b.map = rel.map.p;
            b.trained = part.trained.p;
            b.n = part.n.p;
            b.trow = rel.trow.p + ib.row_off;
            b.tptr = rel.tptr.p + ib.tptr_off;
            b.tj = rel.tj.p + ib.t_off;
            b.wt = rel.wt.p + ib.w_off;
            b.wbeg = rel.wbeg.p + ib.w_off;
            b.wdst = rel.wdst.p + ib.w_off;
            b.n_work = ib.n_work;
            b.lt = rel.lt.p + ib.l_off;
            b.lfirst = rel.lfirst.p + ib.l_off;
            b.lcount = rel.lcount.p + ib.l_off;
            b.n_long = ib.n_long;
            b.cache = part.cache.p;
            b.part = part.part.p;
            b.qrest = X.qrest.p;
            HIP_TRY(launch_block_pass(b, BlockPlan{als_plan(d), part.h_trained.data()}, g, X.e.p, X.Q.p, dev, m->stream));
        }
    // ---- the test rows under the draw the epoch left
    if (X.test) {
        fmhip_relational_t T = X.test;
        std::vector<AlsArgs> tf((size_t)n_parts(T));
        for (size_t p = 0; p < tf.size(); ++p) {
            AlsArgs a = als_args(m, part_data(T, (int)p));
            a.y = X.test_zeros.p;
            a.e = X.test_parts[p]->yhat.p;
            a.q = X.test_parts[p]->q.p;
            tf[p] = a;
        }
        TRY(residuals(s, T, tf, X.test_zeros.p, s->test_last.p, nullptr, nullptr, t));
        HIP_TRY(launch_mcmc_accumulate_link(s->test_last.p, s->test_sum.p, T->n_rows, s->link, m->stream));
    } else if (s->test) {
        TRY(mcmc_accumulate_flat_test(s));
    }
    return mcmc_finish_epoch(s, std::sqrt(sse / (double)N), stats);
}

}  // namespace host
}  // namespace fmhip

extern "C" {

int fmhip_mcmc_create_relational(fmhip_model_t m, fmhip_relational_t train, fmhip_relational_t test_relational, fmhip_dataset_t test_flat,
                                 const fmhip_mcmc_opts *opts, const fmhip_mcmc_task_opts *task_opts, int32_t part_groups, fmhip_mcmc_t *out) {
    if (!out) return fail(FMHIP_ERR_INVALID, "out is NULL");
    *out = nullptr;
    fmhip_mcmc_opts o;
    fmhip_mcmc_task_opts to;
    TRY(mcmc_settings(opts, task_opts, &o, &to));
    if (!m || !train) return fail(FMHIP_ERR_INVALID, "model or train set is NULL");
    if (test_relational && test_flat) return fail(FMHIP_ERR_INVALID, "a relational test set and a flat one were both given: at most one of the two");
    ReadLock lock(m);
    fmhip_relational_t R = train;
    TRY(check_relational(m, R, "the train set"));
    if (test_relational) TRY(check_relational(m, test_relational, "the test set"));
    if (test_flat) TRY(mcmc_check_test(m, test_flat));
    const int NP = n_parts(R);
    if (part_groups && NP > FMHIP_MCMC_MAX_GROUPS) return fail(FMHIP_ERR_UNSUPPORTED, "%d parts are above FMHIP_MCMC_MAX_GROUPS", NP);
    McmcPartOrder po;
    {
        std::vector<const int32_t *> fp((size_t)NP);
        std::vector<int64_t> fn((size_t)NP);
        for (int p = 0; p < NP; ++p) {
            fp[(size_t)p] = part_data(R, p)->h_cfeat.data();
            fn[(size_t)p] = (int64_t)part_data(R, p)->h_cfeat.size();
        }
        po = mcmc_part_order(NP, fp.data(), fn.data());
        if (po.a >= 0)
            return fail(FMHIP_ERR_UNSUPPORTED, "feature %d of %s lies inside the id range of %s: the block sweep walks part after part, which is the flat "
                                               "sweep's ascending feature order only when the parts' id ranges do not interleave", (int)po.feature,
                        part_name(R, po.b).c_str(), part_name(R, po.a).c_str());
    }
    TRY(set_device(m->device));
    fmhip_mcmc *s = new (std::nothrow) fmhip_mcmc;
    if (!s) return fail(FMHIP_ERR_NOMEM, "out of host memory");
    std::unique_ptr<fmhip_mcmc> guard(s);
    s->rel.reset(new (std::nothrow) McmcRelational);
    if (!s->rel) return fail(FMHIP_ERR_NOMEM, "out of host memory");
    McmcRelational &X = *s->rel;
    mcmc_fill(s, m, o, to);
    s->test = test_flat;
    X.train = R;
    X.test = test_relational;
    X.order = po.order;
    X.part_groups = part_groups != 0;
    s->G = X.part_groups ? NP : 1;
    const size_t k1 = (size_t)m->k + 1, N = (size_t)R->n_rows;
    s->lambda.assign(k1 * (size_t)s->G, o.init_lambda);
    s->mu.assign(k1 * (size_t)s->G, 0.0);
    s->h_sums.assign(2 * (size_t)kMcmcSumParts, 0.0);
    TRY(s->sums.alloc(s->h_sums.size()));
    X.h_hyp.assign((size_t)NP * (1 + 2 * k1), 0.0);
    TRY(X.hyp.alloc(X.h_hyp.size()));
    size_t max_rows = N;
    std::vector<int32_t> h_map(N);
    std::vector<uint32_t> h_crow;
    std::vector<double> h_n;
    for (int p = 0; p < NP; ++p) {
        std::unique_ptr<McmcRelational::Part> part(new (std::nothrow) McmcRelational::Part);
        if (!part) return fail(FMHIP_ERR_NOMEM, "out of host memory");
        fmhip_dataset_t d = part_data(R, p);
        part->d = d;
        part->rel = p < (int)R->rels.size() ? p : -1;
        const size_t J = (size_t)d->n_rows, n_cols = d->n_rows > 0 ? (size_t)d->batches[0].n_cols : 0;
        max_rows = std::max(max_rows, J);
        const size_t col_nnz = n_cols ? (size_t)d->h_cptr[n_cols] : 0;
        h_crow.resize(col_nnz);
        if (col_nnz) HIP_TRY(hipMemcpy(h_crow.data(), d->crow.p, col_nnz * sizeof(uint32_t), hipMemcpyDeviceToHost));
        if (part->rel >= 0) {
            const fmhip_relational::Relation &rel = *R->rels[(size_t)p];
            HIP_TRY(hipMemcpy(h_map.data(), rel.map.p, N * sizeof(int32_t), hipMemcpyDeviceToHost));
            mcmc_block_counts(h_map.data(), (int64_t)N, (int64_t)J, h_n);
            TRY(upload(part->n, h_n));
            TRY(zeros(part->cache, (size_t)kBlockCaches * J));
            TRY(part->part.alloc(4 * (size_t)std::max<int32_t>(rel.max_part, 1)));
        }
        part->n_trained = mcmc_block_trained(d->h_cfeat.data(), d->h_cptr.data(), h_crow.data(), (int64_t)n_cols, m->n, part->rel >= 0 ? h_n.data() : nullptr,
                                             part->h_trained);
        s->n_trained += part->n_trained;
        TRY(upload(part->trained, part->h_trained));
        TRY(zeros(part->yhat, J));
        TRY(zeros(part->q, J * (size_t)m->k));
        TRY(zeros(part->z, k1 * n_cols + 1));
        part->h_sums.assign(2 * k1 * (size_t)kMcmcSumParts, 0.0);
        TRY(part->sums.alloc(part->h_sums.size()));
        X.parts.push_back(std::move(part));
    }
    if (X.part_groups) {
        s->plan.counts.clear();
        for (const auto &part : X.parts) s->plan.counts.push_back(part->n_trained);
    }
    TRY(zeros(X.e, N));
    TRY(zeros(X.Q, N * (size_t)m->k));
    TRY(zeros(X.qrest, N));
    TRY(zeros(X.zeros, max_rows));
    TRY(zeros(X.zbias, 1));
    if (s->task == FMHIP_MCMC_CLASSIFICATION) TRY(s->ystar.alloc(N));
    if (test_relational || test_flat) TRY(mcmc_alloc_test(s, test_relational ? test_relational->n_rows : test_flat->n_rows));
    if (test_relational) {
        size_t rows = (size_t)test_relational->n_rows;
        for (int p = 0; p < n_parts(test_relational); ++p) {
            std::unique_ptr<McmcRelational::TestPart> tp(new (std::nothrow) McmcRelational::TestPart);
            if (!tp) return fail(FMHIP_ERR_NOMEM, "out of host memory");
            const size_t J = (size_t)part_data(test_relational, p)->n_rows;
            rows = std::max(rows, J);
            TRY(zeros(tp->yhat, J));
            TRY(zeros(tp->q, J * (size_t)m->k));
            X.test_parts.push_back(std::move(tp));
        }
        TRY(zeros(X.test_zeros, rows));
    }
    *out = guard.release();
    return FMHIP_OK;
}

}  // extern "C"
