// cpp_mcmc.cpp — include/sparkfm.hpp's HipMCMC on a problem made of integer formulas (tests/test_gpu_mcmc.py builds the same one):
// three Gibbs sweeps with a test set and one burn-in epoch; prints the parameters, the state and the predictions as hex floats.
#include <cstdio>
#include <vector>

#include "sparkfm.hpp"

using namespace sparkfm;

static DataSet *rows(int n, int shift) {
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
        y.push_back(0.5 + 0.1 * ((r * 7) % 11 - 5));
    }
    return new DataSet(rp, col, val, y);
}

static void line(const char *name, const std::vector<double> &x) {
    printf("%s", name);
    for (double d : x) printf(" %a", d);
    printf("\n");
}

int main() {
    try {
        const int n1 = 40, k = 3;
        DataSet *train = rows(400, 0), *test = rows(100, 1000);
        FMModel fm(n1 - 1, k);
        fm.w0 = 0.1;
        for (int i = 0; i < n1; ++i) {
            fm.w[(size_t)i] = 0.02 * ((i % 7) - 3);
            for (int f = 0; f < k; ++f) fm.v[(size_t)(f + i * k)] = 0.01 * ((f * 7 + i * 3) % 11 - 5);
        }
        {
            HipMCMC mcmc = HipMCMC::run(12, test, 1);
            for (int it = 0; it < 3; ++it) mcmc.learn(fm, *train);
            const HipMCMC::State st = mcmc.state();
            line("w0", {fm.w0});
            line("w", fm.w);
            line("v", fm.v);
            line("alpha", {st.alpha, mcmc.last_stats.alpha});
            line("lambda", st.lambda);
            line("mu", st.mu);
            line("mean", mcmc.predictions());
            line("last", mcmc.lastPredictions());
            line("rmse", {mcmc.computeRMSE()});
            printf("draws %lld %lld\n", (long long)mcmc.draws(), (long long)st.iterations);
        }
        delete train;
        delete test;
    } catch (const Error &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
