// cpp_mcmc_probit.cpp — include/sparkfm.hpp's HipMCMC with a task, on cpp_mcmc.cpp's integer formulas (tests/test_gpu_mcmc_probit.py
// builds the same problem): the classification task (labels cut at 0.5) for three Gibbs sweeps with a test set and one burn-in epoch,
// then the regression task with a clip and with clip_to_labels for two; prints parameters, state, latent targets, predictions and
// scores as hex floats.
#include <cstdio>
#include <vector>

#include "sparkfm.hpp"

using namespace sparkfm;

static DataSet *rows(int n, int shift, bool cut) {
    std::vector<int64_t> rp(1, 0);
    std::vector<int32_t> col;
    std::vector<double> val, y;
    for (int j = 0; j < n; ++j) {
        const int r = j + shift;
        for (int t = 0; t < 1 + r % 3; ++t) {
            col.push_back((r * 7 + t * 13) % 39);
            val.push_back(0.5 + ((r + t) % 4) / 8.0);
        }
        rp.push_back((int64_t)col.size());
        const double label = 0.5 + 0.1 * ((r * 7) % 11 - 5);
        y.push_back(cut ? (label > 0.5 ? 1.0 : 0.0) : label);
    }
    return new DataSet(rp, col, val, y);
}

static void start(FMModel &fm, int n1, int k) {
    fm.w0 = 0.1;
    for (int i = 0; i < n1; ++i) {
        fm.w[(size_t)i] = 0.02 * ((i % 7) - 3);
        for (int f = 0; f < k; ++f) fm.v[(size_t)(f + i * k)] = 0.01 * ((f * 7 + i * 3) % 11 - 5);
    }
}

static void line(const char *name, const std::vector<double> &x) {
    printf("%s", name);
    for (double d : x) printf(" %a", d);
    printf("\n");
}

int main() {
    try {
        const int n1 = 40, k = 3;
        {
            DataSet *train = rows(400, 0, true), *test = rows(100, 1000, true);
            FMModel fm(n1 - 1, k);
            start(fm, n1, k);
            {
                HipMCMC mcmc(12, test, 1, true, FMHIP_MCMC_CLASSIFICATION);
                for (int it = 0; it < 3; ++it) mcmc.learn(fm, *train);
                const HipMCMC::State st = mcmc.state();
                line("w0", {fm.w0});
                line("w", fm.w);
                line("v", fm.v);
                line("alpha", {st.alpha, mcmc.last_stats.alpha});
                line("lambda", st.lambda);
                line("mu", st.mu);
                line("ystar", mcmc.latentTargets());
                line("mean", mcmc.predictions());
                line("last", mcmc.lastPredictions());
                line("logloss", {mcmc.computeLogLoss()});
                line("accuracy", {mcmc.computeAccuracy()});
                printf("draws %lld %lld\n", (long long)mcmc.draws(), (long long)st.iterations);
                int refused = 0;
                try {
                    (void)mcmc.computeRMSE();
                } catch (const Error &) {
                    refused = 1;
                }
                printf("rmse_refused %d\n", refused);
            }
            delete train;
            delete test;
        }
        DataSet *train = rows(400, 0, false), *test = rows(100, 1000, false);
        {
            FMModel fm(n1 - 1, k);
            start(fm, n1, k);
            HipMCMC mcmc(12, test);
            mcmc.setClip(0.3, 0.7);
            for (int it = 0; it < 2; ++it) mcmc.learn(fm, *train);
            line("clip_mean", mcmc.predictions());
            line("clip_w", fm.w);
        }
        {
            FMModel fm(n1 - 1, k);
            start(fm, n1, k);
            HipMCMC mcmc(12, test);
            mcmc.clip_to_labels = true;
            for (int it = 0; it < 2; ++it) mcmc.learn(fm, *train);
            line("labels_mean", mcmc.predictions());
        }
        delete train;
        delete test;
    } catch (const Error &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
