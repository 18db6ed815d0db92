// cpp_relational.cpp — include/sparkfm.hpp's Relation / RelationalData: a user block, an item block, their mappings, a plain part
// and a model from integer formulas; the RMSE, one HipSGD epoch in batches of 250, the RMSE again.  Prints "before" / "after" <rmse>,
// "predict3" (the first three predictions) and the parameters "w0", "w", "v", every number as a hex float, for
// tests/test_gpu_relational.py, whose Python mirror over the same formulas must give the same bits.  Then the fit loop with
// FM::withRelation, and the refusal of a mapping entry out of range.
#include <cstdio>
#include <vector>

#include "sparkfm.hpp"

using namespace sparkfm;

static void print(const char *key, const std::vector<double> &x) {
    printf("%s", key);
    for (double v : x) printf(" %a", v);
    printf("\n");
}

static std::vector<SparseVector> block(int rows, int base, int span, int mul) {
    std::vector<SparseVector> out;
    for (int j = 0; j < rows; ++j) {
        SparseVector sv;
        for (int t = 0; t < 1 + j % 4; ++t) {
            const int i = base + (j * mul + t * 17 + (j * t) % 5) % span;
            bool dup = false;
            for (int32_t c : sv.index) dup = dup || c == i;
            if (dup) continue;
            sv.index.push_back(i);
            sv.data.push_back(0.5 + (double)((j + t) % 4) / 8.0);
        }
        out.push_back(sv);
    }
    return out;
}

int main() {
    const int n = 600, nu = 23, ni = 41, k = 8, n1 = 200;
    std::vector<int32_t> mu, mi;
    std::vector<double> y;
    std::vector<std::pair<double, SparseVector>> prow;
    for (int r = 0; r < n; ++r) {
        mu.push_back((r * 5 + r / 7) % nu);
        mi.push_back(r % 3 == 0 ? 3 : (r * 11 + r / 5) % ni);
        y.push_back(0.5 + 0.1 * ((r * 7) % 11 - 5));
        SparseVector sv;
        for (int t = 0; t < r % 3; ++t) {
            sv.index.push_back(t == 0 ? 150 + (r * 3 + t * 7) % 30 : 180 + (r + t) % 20);
            sv.data.push_back(t == 0 ? 1.0 : 0.25);
        }
        prow.emplace_back(y.back(), sv);
    }
    try {
        Relation users(block(nu, 0, 60, 7), mu), items(block(ni, 60, 90, 11), mi);
        DataSet plain(prow, 250);
        RelationalData rd(y, {&users, &items}, &plain, 250);
        FMModel fm(n1 - 1, k);
        fm.w0 = 0.1;
        for (int i = 0; i < n1; ++i) {
            fm.w[(size_t)i] = 0.02 * ((i % 7) - 3);
            for (int f = 0; f < k; ++f) fm.v[(size_t)(f + i * k)] = 0.01 * ((f * 7 + i * 3) % 11 - 5);
        }
        if (rd.n_batches() != 3 || rd.dimension() > n1 - 1) return 1;
        print("before", {fm.computeRMSE(rd)});
        HipSGD sgd = HipSGD::run(0.05, 0.0, 1e-4, 1e-4);
        sgd.learn(fm, rd);
        if (sgd.last_stats.rows != n || sgd.last_stats.steps != 3) return 1;
        print("after", {fm.computeRMSE(rd)});
        const std::vector<double> yh = fm.predict(rd);
        print("predict3", {yh[0], yh[1], yh[2]});
        print("w0", {fm.w0});
        print("w", fm.w);
        print("v", fm.v);
        // the fit loop: withRelation returns the FM, the RMSE falls
        FM fit(plain, k, 3);
        if (&fit.withRelation(users) != &fit || &fit.withRelation({&items}) != &fit) return 1;
        HipSGD sgd2 = HipSGD::run(0.05, 0.0, 1e-4, 1e-4);
        FMModel fitted = fit.learnWith(sgd2);
        if (fit.rmse_history.size() != 3 || !(fit.rmse_history[2] < fit.rmse_history[0])) {
            fprintf(stderr, "the fit loop did not lower the RMSE\n");
            return 1;
        }
        // a learner without a relational step says so; a mapping entry out of range is refused by the library
        try {
            HipALS als;
            als.learn(fm, rd);
            fprintf(stderr, "HipALS trained on relational data\n");
            return 1;
        } catch (const Error &e) {
            if (e.code != FMHIP_ERR_UNSUPPORTED) return 1;
        }
        try {
            std::vector<int32_t> bad = mu;
            bad[5] = nu;
            Relation off(block(nu, 0, 60, 7), bad);
            RelationalData r2(y, {&off, &items});
            r2.cache();
            fprintf(stderr, "a mapping entry out of range was accepted\n");
            return 1;
        } catch (const Error &e) {
            if (e.code != FMHIP_ERR_INVALID) return 1;
        }
    } catch (const Error &e) {
        fprintf(stderr, "error %d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}
