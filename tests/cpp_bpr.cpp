// cpp_bpr.cpp — include/sparkfm.hpp's HipBPR: a user block, an item block, per-user positives and a model from integer formulas;
// the pair log-loss of the draw at t = 0, two epochs in batches of 100 pairs (n_neg = 2), the pair log-loss of the last draw.
// Prints "before" / "after" <pair log-loss>, "neg" (the last draw), "attempts" / "forced" of a resample at t = 1 and the parameters
// "w0", "w", "v", every number as a hex float, for tests/test_gpu_bpr.py, whose Python mirror over the same formulas must give the
// same bits.  Then the fit loop sized by the learner, and the refusal of a user whose positives are all items.
#include <cstdio>
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

int main() {
    const int nu = 23, ni = 41, k = 8, n1 = 150;
    std::vector<std::vector<int32_t>> positives;
    int n_inter = 0;
    for (int u = 0; u < nu; ++u) {
        std::vector<int32_t> rows;
        for (int t = 0; t < 3 + u % 5; ++t) rows.push_back((u * 7 + t * 11) % ni);      // (unsorted; a repeat now and then)
        positives.push_back(rows);
        std::vector<int32_t> s = rows;
        std::sort(s.begin(), s.end());
        n_inter += (int)(std::unique(s.begin(), s.end()) - s.begin());
    }
    try {
        DataSet users(block(nu, 0, 60, 7)), items(block(ni, 60, 90, 11));
        HipBPR bpr(users, items, positives, 2, 100, 5, 0.05, 0.0, 1e-4, 1e-4);
        FMModel fm(n1 - 1, k);
        fm.w0 = 0.1;
        for (int i = 0; i < n1; ++i) {
            fm.w[(size_t)i] = 0.02 * ((i % 7) - 3);
            for (int f = 0; f < k; ++f) fm.v[(size_t)(f + i * k)] = 0.01 * ((f * 7 + i * 3) % 11 - 5);
        }
        if (bpr.n_pairs() != 2 * n_inter || bpr.dimension() > n1 - 1) return 1;
        print("before", {bpr.computePairLogLoss(fm)});
        bpr.learn(fm);
        bpr.learn(fm);
        if (bpr.last_stats.rows != 2 * bpr.n_pairs() || bpr.last_stats.sum_e != 0.0 || bpr.last_stats.steps != (bpr.n_pairs() + 99) / 100) return 1;
        print("after", {bpr.computePairLogLoss(fm), bpr.computePairAccuracy(fm)});
        std::vector<double> neg;
        for (int32_t c : bpr.negatives()) neg.push_back((double)c);
        print("neg", neg);
        const fmhip_bpr_sample_stats st = bpr.resample(1);
        print("attempts", {(double)st.attempts});
        print("forced", {(double)st.forced});
        print("w0", {fm.w0});
        print("w", fm.w);
        print("v", fm.v);
        // the fit loop: the model is as wide as the learner's blocks, not as the dataset argument (the users alone)
        FM fit(users, k, 2);
        HipBPR bpr2(users, items, positives, 1, 20, 5, 0.5, 0.0, 1e-4, 1e-4);
        FMModel fitted = fit.learnWith(bpr2);
        if (fitted.num_attribute != bpr2.dimension() || fitted.num_attribute <= users.dimension()) {
            fprintf(stderr, "the fit loop sized the model from the users alone\n");
            return 1;
        }
        FMModel fresh(bpr2.dimension(), k);                                 // the model the fit started from (seed 0)
        if (!(bpr2.computePairLogLoss(fitted) < bpr2.computePairLogLoss(fresh))) {      // (the handle is made again over the re-cached users)
            fprintf(stderr, "two epochs did not lower the pair log-loss\n");
            return 1;
        }
        // a user whose positives are all items has no negative: refused by the library, which names the user
        try {
            std::vector<std::vector<int32_t>> all = positives;
            all[4].clear();
            for (int j = 0; j < ni; ++j) all[4].push_back(j);
            HipBPR bad(users, items, all);
            bad.handle();
            fprintf(stderr, "a context without a negative was accepted\n");
            return 1;
        } catch (const Error &e) {
            if (e.code != FMHIP_ERR_INVALID || std::string(e.what()).find("context 4") == std::string::npos) return 1;
        }
    } catch (const Error &e) {
        fprintf(stderr, "error %d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}
