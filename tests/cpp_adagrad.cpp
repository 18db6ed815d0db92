// cpp_adagrad.cpp — include/sparkfm.hpp's HipSGD with the AdaGrad option: FM(dataset, k, maxIteration).learnWith(HipSGD::run(...,
// FMHIP_OPT_ADAGRAD)) on a small synthetic regression problem.  Prints "before <rmse>", "adagrad_after <rmse>" and
// "sgd_after <rmse>" (the same fit under plain SGD) for tests/test_gpu_adagrad.py.
#include <cstdio>
#include <vector>

#include "sparkfm.hpp"

using namespace sparkfm;

int main() {
    const int n_rows = 2000, n1 = 301, k = 8;
    std::vector<std::pair<double, SparseVector>> rows;
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
    }
    try {
        DataSet ds(rows, 250);
        FM fit0(ds, k, 0);
        HipSGD none = HipSGD::run(0.05, 0.0, 0.0, 0.0, FMHIP_LOSS_SQUARED, FMHIP_OPT_ADAGRAD);
        FMModel m0 = fit0.learnWith(none);
        const double before = m0.computeRMSE(ds);
        FM fit(ds, k, 5);
        HipSGD ada = HipSGD::run(0.05, 0.0, 1e-4, 1e-4, FMHIP_LOSS_SQUARED, FMHIP_OPT_ADAGRAD, 1e-10, 0.1);
        FMModel ma = fit.learnWith(ada);
        HipSGD sgd = HipSGD::run(0.05, 0.0, 1e-4, 1e-4);
        FM fit2(ds, k, 5);
        FMModel ms = fit2.learnWith(sgd);
        printf("before %.9g\nadagrad_after %.9g\nsgd_after %.9g\n", before, ma.computeRMSE(ds), ms.computeRMSE(ds));
    } catch (const Error &e) {
        fprintf(stderr, "error %d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}
