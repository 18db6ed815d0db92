// cpp_mcmc_relational.cpp — include/sparkfm.hpp's HipMCMC over a RelationalData on a problem of integer formulas
// (tests/test_gpu_mcmc_relational.py builds the same one): 6 users (id + one of 3 history features), 5 items (id + one of 2 genres),
// 2 plain features, 60 train and 20 test rows, a part is a group, three Gibbs sweeps by blocks; prints the parameters, the state, the
// averaged test predictions and the parts' counts as hex floats / integers.
#include <cstdio>
#include <vector>

#include "sparkfm.hpp"

using namespace sparkfm;

static std::vector<SparseVector> users() {
    std::vector<SparseVector> rows;
    for (int u = 0; u < 6; ++u) rows.push_back(SparseVector{{u, 6 + u % 3}, {1.0, 0.5 + 0.25 * (u % 2)}});
    return rows;
}

static std::vector<SparseVector> items() {
    std::vector<SparseVector> rows;
    for (int i = 0; i < 5; ++i) rows.push_back(SparseVector{{9 + i, 14 + i % 2}, {1.0, 0.75}});
    return rows;
}

struct Rows {
    std::vector<int32_t> umap, imap;
    std::vector<double> y;
    DataSet *plain;
};

static Rows rows(int n, int shift) {
    Rows out;
    std::vector<int64_t> rp(1, 0);
    std::vector<int32_t> col;
    std::vector<double> val;
    for (int j = 0; j < n; ++j) {
        const int r = j + shift;
        out.umap.push_back((3 * r + 1) % 6);
        out.imap.push_back((7 * r + 2) % 5);
        col.push_back(16);
        val.push_back(0.25 * ((r % 5) - 2));
        col.push_back(17);
        val.push_back(0.5 * ((r % 3) - 1) + 0.125);
        rp.push_back((int64_t)col.size());
        out.y.push_back(0.5 * ((r * 5) % 9) - 1.0);
    }
    out.plain = new DataSet(rp, col, val, out.y);
    return out;
}

static void line(const char *name, const std::vector<double> &x) {
    printf("%s", name);
    for (double d : x) printf(" %a", d);
    printf("\n");
}

int main() {
    try {
        const int n1 = 19, k = 3;
        Rows tr = rows(60, 0), te = rows(20, 3);
        FMModel fm(n1 - 1, k);
        fm.w0 = 0.1;
        for (int i = 0; i < n1; ++i) {
            fm.w[(size_t)i] = 0.02 * ((i % 7) - 3);
            for (int f = 0; f < k; ++f) fm.v[(size_t)(f + i * k)] = 0.01 * ((f * 7 + i * 3) % 11 - 5);
        }
        {
            Relation ru(users(), tr.umap), ri(items(), tr.imap), tu(users(), te.umap), ti(items(), te.imap);
            RelationalData train(tr.y, {&ru, &ri}, tr.plain), test(te.y, {&tu, &ti}, te.plain);
            HipMCMC mcmc = HipMCMC::run(12);
            mcmc.setPartGroups();
            mcmc.setTest(&test);
            for (int it = 0; it < 3; ++it) mcmc.learn(fm, train);
            const HipMCMC::State st = mcmc.state();
            line("w0", {fm.w0});
            line("w", fm.w);
            line("v", fm.v);
            line("alpha", {st.alpha});
            line("lambda", st.lambda);
            line("mu", st.mu);
            line("mean", mcmc.predictions());
            printf("counts");
            for (int64_t c : mcmc.groupCounts()) printf(" %lld", (long long)c);
            printf("\ngroups %d\n", (int)mcmc.numGroups());
            mcmc.close();
        }
        delete tr.plain;
        delete te.plain;
    } catch (const std::exception &e) {
        fprintf(stderr, "cpp_mcmc_relational: %s\n", e.what());
        return 1;
    }
    return 0;
}
