// cpp_weights.cpp — include/sparkfm.hpp's weighted DataSet and FMModel::weightedScores: a small dataset, its weights and a model
// from integer formulas, the weighted scores, one HipSGD epoch, the scores again.  Prints "before" / "after" <sum_w rmse mae logloss>
// and the parameters "w0", "w", "v", every number as a hex float, for tests/test_gpu_weights.py, whose Python mirror over the same
// formulas must give the same bits.
#include <cstdio>
#include <vector>

#include "sparkfm.hpp"

using namespace sparkfm;

static void print(const char *key, const std::vector<double> &x) {
    printf("%s", key);
    for (double v : x) printf(" %a", v);
    printf("\n");
}

int main() {
    const int n_rows = 1000, n1 = 301, k = 8;
    const double cycle[5] = {0.0, 0.25, 1.0, 3.5, 1.0};
    std::vector<std::pair<double, SparseVector>> rows;
    std::vector<double> weights;
    for (int r = 0; r < n_rows; ++r) {
        SparseVector sv;
        double y = 0.5;
        for (int j = 0; j < 3 + r % 6; ++j) {
            const int i = (r * 13 + j * 101 + (r * j) % 7) % n1;
            bool dup = false;
            for (int32_t c : sv.index) dup = dup || c == i;
            if (dup) continue;
            const double x = 0.5 + (double)((r + j) % 4) / 8.0;
            sv.index.push_back(i);
            sv.data.push_back(x);
            y += x * ((i % 5) - 2) * 0.2;
        }
        rows.emplace_back(y, sv);
        weights.push_back(cycle[r % 5]);
    }
    try {
        DataSet ds(rows, 250, 0, weights);
        FMModel fm(n1 - 1, k);
        fm.w0 = 0.1;
        for (int i = 0; i < n1; ++i) {
            fm.w[(size_t)i] = 0.02 * ((i % 7) - 3);
            for (int f = 0; f < k; ++f) fm.v[(size_t)(f + i * k)] = 0.01 * ((f * 7 + i * 3) % 11 - 5);
        }
        const fmhip_weighted_result b = fm.weightedScores(ds);
        print("before", {b.sum_w, b.rmse, b.mae, b.logloss});
        HipSGD sgd = HipSGD::run(0.05, 0.0, 1e-4, 1e-4);
        sgd.learn(fm, ds);
        const fmhip_weighted_result a = fm.weightedScores(ds);
        print("after", {a.sum_w, a.rmse, a.mae, a.logloss});
        print("w0", {fm.w0});
        print("w", fm.w);
        print("v", fm.v);
        // an unweighted DataSet is refused by the weighted scores, a wrong number of weights by the constructor
        DataSet plain(rows, 250);
        try {
            (void)fm.weightedScores(plain);
            fprintf(stderr, "an unweighted dataset was scored\n");
            return 1;
        } catch (const Error &e) {
            if (e.code != FMHIP_ERR_INVALID) return 1;
        }
        try {
            DataSet bad(rows, 250, 0, std::vector<double>(3, 1.0));
            fprintf(stderr, "three weights for a thousand rows were accepted\n");
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
