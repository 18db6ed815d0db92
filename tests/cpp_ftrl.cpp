// cpp_ftrl.cpp — include/sparkfm.hpp's HipFTRL: a small click dataset and a model from integer formulas, two HipFTRL epochs (logistic
// loss, L1 and L2 on; the second epoch needs the state of the first, which the model's upload before every call must not reset), the
// model's sparsity counts.  Prints "logloss" <before after>, "nonzeros" <w v all_zero> and the parameters "w0", "w", "v", every number
// as a hex float, for tests/test_gpu_ftrl.py, whose Python mirror over the same formulas must give the same bits.
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
    std::vector<std::pair<double, SparseVector>> rows;
    for (int r = 0; r < n_rows; ++r) {
        SparseVector sv;
        double s = 0.0;
        for (int j = 0; j < 3 + r % 6; ++j) {
            const int i = (r * 13 + j * 101 + (r * j) % 7) % n1;
            bool dup = false;
            for (int32_t c : sv.index) dup = dup || c == i;
            if (dup) continue;
            const double x = 0.5 + (double)((r + j) % 4) / 8.0;
            sv.index.push_back(i);
            sv.data.push_back(x);
            s += x * ((i % 5) - 2) * 0.2;
        }
        rows.emplace_back(s > 0.0 ? 1.0 : 0.0, sv);
    }
    try {
        DataSet ds(rows, 250);
        FMModel fm(n1 - 1, k);
        fm.w0 = 0.1;
        for (int i = 0; i < n1; ++i) {
            fm.w[(size_t)i] = 0.02 * ((i % 7) - 3);
            for (int f = 0; f < k; ++f) fm.v[(size_t)(f + i * k)] = 0.01 * ((f * 7 + i * 3) % 11 - 5);
        }
        const double before = fm.computeLogLoss(ds);
        HipFTRL ftrl = HipFTRL::run(0.1, 0.5, 0.05, 0.002, 0.0, 1e-4, 1e-4, 0.1, FMHIP_LOSS_LOGISTIC);
        ftrl.learn(fm, ds);
        ftrl.learn(fm, ds);
        print("logloss", {before, fm.computeLogLoss(ds)});
        const FMModel::Nonzeros z = fm.nonzeros();
        print("nonzeros", {(double)z.w_nonzero, (double)z.v_nonzero, (double)z.features_all_zero});
        print("w0", {fm.w0});
        print("w", fm.w);
        print("v", fm.v);
        // the rule is no third value of the optimizer switch
        if (fmhip_model_set_optimizer(fm.upload(), FMHIP_OPT_FTRL, 1e-10, 0.1) != FMHIP_ERR_INVALID) {
            fprintf(stderr, "fmhip_model_set_optimizer accepted FMHIP_OPT_FTRL\n");
            return 1;
        }
    } catch (const Error &e) {
        fprintf(stderr, "error %d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}
