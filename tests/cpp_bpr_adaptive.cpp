// cpp_bpr_adaptive.cpp — include/sparkfm.hpp's HipBPR with n_candidates = 4 (include/fmhip_bpr_adaptive.h) over the integer formulas
// of cpp_bpr.cpp: two epochs in batches of 100 pairs (n_neg = 2), each epoch's negatives the best of 4 candidates under the model at
// the epoch's start, then an adaptive resample at t = 2 under the trained model.  Prints "candidates", "neg" (the draw of the last
// epoch), "attempts" / "forced" / "replaced" and "neg2" of the resample, and the parameters "w0", "w", "v", every number as a hex
// float, for tests/test_gpu_bpr_adaptive.py, whose Python mirror must give the same bits.  Then the refusals of the wrapper.
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

static std::vector<double> as_doubles(const std::vector<int32_t> &x) { return std::vector<double>(x.begin(), x.end()); }

int main() {
    const int nu = 23, ni = 41, k = 8, n1 = 150;
    std::vector<std::vector<int32_t>> positives;
    for (int u = 0; u < nu; ++u) {
        std::vector<int32_t> rows;
        for (int t = 0; t < 3 + u % 5; ++t) rows.push_back((u * 7 + t * 11) % ni);
        positives.push_back(rows);
    }
    try {
        DataSet users(block(nu, 0, 60, 7)), items(block(ni, 60, 90, 11));
        HipBPR bpr(users, items, positives, 2, 100, 5, 0.05, 0.0, 1e-4, 1e-4, FMHIP_LOSS_LOGISTIC, FMHIP_OPT_SGD, 1e-10, 0.1, 4);
        FMModel fm(n1 - 1, k);
        fm.w0 = 0.1;
        for (int i = 0; i < n1; ++i) {
            fm.w[(size_t)i] = 0.02 * ((i % 7) - 3);
            for (int f = 0; f < k; ++f) fm.v[(size_t)(f + i * k)] = 0.01 * ((f * 7 + i * 3) % 11 - 5);
        }
        int32_t n_cand = 0;
        check(fmhip_bpr_get_candidates(bpr.handle(), &n_cand));
        if (n_cand != 4 || bpr.n_candidates() != 4) return 1;
        print("candidates", {(double)n_cand});
        bpr.learn(fm);
        bpr.learn(fm);
        if (bpr.last_stats.rows != 2 * bpr.n_pairs() || bpr.last_stats.sum_e != 0.0) return 1;
        print("neg", as_doubles(bpr.negatives()));
        const fmhip_bpr_adaptive_stats st = bpr.resample(2, fm);
        print("attempts", {(double)st.attempts});
        print("forced", {(double)st.forced});
        print("replaced", {(double)st.replaced});
        print("neg2", as_doubles(bpr.negatives()));
        print("w0", {fm.w0});
        print("w", fm.w);
        print("v", fm.v);
        // several candidates and no model: refused by the wrapper; a count outside [1, 64]: refused at construction
        try {
            bpr.resample(3);
            fprintf(stderr, "a uniform resample was accepted at 4 candidates\n");
            return 1;
        } catch (const Error &e) {
            if (e.code != FMHIP_ERR_INVALID || std::string(e.what()).find("model") == std::string::npos) return 1;
        }
        for (int32_t bad : {0, 65}) {
            try {
                HipBPR refused(users, items, positives, 1, 0, 0, 0.05, 0.0, 0.0, 0.0, FMHIP_LOSS_LOGISTIC, FMHIP_OPT_SGD, 1e-10, 0.1, bad);
                fprintf(stderr, "n_candidates = %d was accepted\n", (int)bad);
                return 1;
            } catch (const Error &e) {
                if (e.code != FMHIP_ERR_INVALID) return 1;
            }
        }
    } catch (const Error &e) {
        fprintf(stderr, "error %d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}
