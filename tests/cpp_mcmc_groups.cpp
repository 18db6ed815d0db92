// cpp_mcmc_groups.cpp — include/sparkfm.hpp's HipMCMC with attribute groups on cpp_mcmc.cpp's problem of integer formulas
// (tests/test_gpu_mcmc_groups.py builds the same one): feature i is of group i % 3, three Gibbs sweeps; prints the parameters, the
// state and the groups' counts as hex floats / integers.
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
        DataSet *train = rows(400, 0);
        FMModel fm(n1 - 1, k);
        fm.w0 = 0.1;
        for (int i = 0; i < n1; ++i) {
            fm.w[(size_t)i] = 0.02 * ((i % 7) - 3);
            for (int f = 0; f < k; ++f) fm.v[(size_t)(f + i * k)] = 0.01 * ((f * 7 + i * 3) % 11 - 5);
        }
        {
            HipMCMC mcmc = HipMCMC::run(12);
            std::vector<int32_t> groups((size_t)n1);
            for (int i = 0; i < n1; ++i) groups[(size_t)i] = i % 3;
            mcmc.setGroups(groups);
            for (int it = 0; it < 3; ++it) mcmc.learn(fm, *train);
            const HipMCMC::State st = mcmc.state();
            line("w0", {fm.w0});
            line("w", fm.w);
            line("v", fm.v);
            line("alpha", {st.alpha});
            line("lambda", st.lambda);
            line("mu", st.mu);
            printf("counts");
            for (int64_t c : mcmc.groupCounts()) printf(" %lld", (long long)c);
            printf("\ngroups %d %lld\n", (int)mcmc.numGroups(), (long long)st.iterations);
        }
        delete train;
    } catch (const Error &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
