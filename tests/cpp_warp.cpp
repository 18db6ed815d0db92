// cpp_warp.cpp — include/sparkfm.hpp's HipBPR with sampler = kWarp (include/fmhip_warp.h), 4 candidates and margin 1/64 over the
// integer formulas of cpp_bpr.cpp: two epochs in batches of 100 pairs (n_neg = 2), each epoch's negatives the first violators under
// the model at the epoch's start, then a WARP resample at t = 2 under the trained model.  Prints "candidates", "margin", "neg" /
// "weights" / "trials" (the draw of the last epoch), "pairs" / "violated" / "sum_trials", "neg2" / "weights2" / "trials2" of the
// resample, and the parameters "w0", "w", "v", every number as a hex float, for tests/test_gpu_warp.py, whose Python mirror must give
// the same bits.  Then the refusals of the wrapper.
#include <cstdio>
#include <string>
#include <vector>

#include "sparkfm.hpp"

using namespace sparkfm;

static void print(const char *key, const std::vector<double> &x) {
    printf("%s", key);
    for (double v : x) printf(" %a", v);
    printf("\n");
}

static std::vector<std::pair<double, SparseVector>> block(int rows, int base, int span, int mul) {
    std::vector<std::pair<double, SparseVector>> out;
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
        out.emplace_back(0.0, sv);
    }
    return out;
}

template <typename T>
static std::vector<double> as_doubles(const std::vector<T> &x) { return std::vector<double>(x.begin(), x.end()); }

template <typename F>
static bool refused(F &&call, const char *needle) {
    try {
        call();
    } catch (const Error &e) {
        return e.code == FMHIP_ERR_INVALID && std::string(e.what()).find(needle) != std::string::npos;
    }
    return false;
}

int main() {
    const int nu = 23, ni = 41, k = 8, n1 = 150;
    const double margin = 1.0 / 64.0;
    std::vector<std::vector<int32_t>> positives;
    for (int u = 0; u < nu; ++u) {
        std::vector<int32_t> rows;
        for (int t = 0; t < 3 + u % 5; ++t) rows.push_back((u * 7 + t * 11) % ni);
        positives.push_back(rows);
    }
    try {
        DataSet users(block(nu, 0, 60, 7)), items(block(ni, 60, 90, 11));
        HipBPR bpr(users, items, positives, 2, 100, 5, 0.05, 0.0, 1e-4, 1e-4, FMHIP_LOSS_LOGISTIC, FMHIP_OPT_SGD, 1e-10, 0.1, 4, HipBPR::kWarp, margin);
        FMModel fm(n1 - 1, k);
        fm.w0 = 0.1;
        for (int i = 0; i < n1; ++i) {
            fm.w[(size_t)i] = 0.02 * ((i % 7) - 3);
            for (int f = 0; f < k; ++f) fm.v[(size_t)(f + i * k)] = 0.01 * ((f * 7 + i * 3) % 11 - 5);
        }
        int32_t n_cand = 0;
        int enabled = 0;
        double m = 0.0;
        check(fmhip_bpr_get_candidates(bpr.handle(), &n_cand));
        check(fmhip_warp_get(bpr.handle(), &enabled, &m));
        if (n_cand != 4 || bpr.n_candidates() != 4 || enabled != 1 || m != margin || !bpr.warp() || bpr.margin() != margin) return 1;
        print("candidates", {(double)n_cand});
        print("margin", {m});
        // no WARP draw yet: the weights are refused by the library
        if (!refused([&] { bpr.pairWeights(); }, "fmhip_warp_resample")) return 1;
        bpr.learn(fm);
        bpr.learn(fm);
        if (bpr.last_stats.rows != 2 * bpr.n_pairs() || bpr.last_stats.sum_e != 0.0) return 1;
        print("neg", as_doubles(bpr.negatives()));
        print("weights", as_doubles(bpr.pairWeights()));
        print("trials", as_doubles(bpr.trials()));
        const fmhip_warp_stats st = bpr.resampleWarp(2, fm);
        print("pairs", {(double)st.pairs});
        print("violated", {(double)st.violated});
        print("sum_trials", {(double)st.trials});
        print("neg2", as_doubles(bpr.negatives()));
        print("weights2", as_doubles(bpr.pairWeights()));
        print("trials2", as_doubles(bpr.trials()));
        print("w0", {fm.w0});
        print("w", fm.w);
        print("v", fm.v);
        // the other draws are refused under WARP, by the wrapper ...
        if (!refused([&] { bpr.resample(3); }, "resampleWarp") || !refused([&] { bpr.resample(3, fm); }, "resampleWarp")) return 1;
        // ... and by the library, which leaves the draw as it was
        const std::vector<int32_t> before = bpr.negatives();
        fmhip_bpr_sample_stats su{};
        if (fmhip_bpr_resample(bpr.handle(), 3, &su) != FMHIP_ERR_INVALID || bpr.negatives() != before) return 1;
        // a bad sampler, a bad margin, a loss beside WARP: refused at construction
        if (!refused([&] { HipBPR r(users, items, positives, 1, 0, 0, 0.05, 0.0, 0.0, 0.0, FMHIP_LOSS_LOGISTIC, FMHIP_OPT_SGD, 1e-10, 0.1, 1, 2); }, "sampler")) return 1;
        if (!refused([&] { HipBPR r(users, items, positives, 1, 0, 0, 0.05, 0.0, 0.0, 0.0, FMHIP_LOSS_LOGISTIC, FMHIP_OPT_SGD, 1e-10, 0.1, 1, HipBPR::kWarp, -0.5); },
                     "margin"))
            return 1;
        if (!refused([&] { HipBPR r(users, items, positives, 1, 0, 0, 0.05, 0.0, 0.0, 0.0, FMHIP_LOSS_SQUARED, FMHIP_OPT_SGD, 1e-10, 0.1, 1, HipBPR::kWarp); }, "loss"))
            return 1;
    } catch (const Error &e) {
        fprintf(stderr, "error %d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}
