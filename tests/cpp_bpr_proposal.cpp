// cpp_bpr_proposal.cpp — include/sparkfm.hpp's HipBPR with negatives = kPopularity (include/fmhip_proposal.h) over the integer
// formulas of cpp_bpr.cpp: n_neg = 2, batches of 100 pairs, the keep-the-draw rule.  Prints "weights" (the proposal), "thresh" and
// "alias" (the library's table), "neg" and "stats" (attempts, forced) after resample(2), "neg1" and the parameters "w0", "w", "v" after
// one epoch by learn, and "neg_uniform" after setProposal({}) and resample(2), every number as a hex float, for
// tests/test_gpu_bpr_proposal.py, whose Python mirror must give the same bits.  Then the refusals.
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
    std::vector<std::vector<int32_t>> positives;
    for (int u = 0; u < nu; ++u) {
        std::vector<int32_t> rows;
        for (int t = 0; t < 3 + u % 5; ++t) rows.push_back((u * 7 + t * 11) % ni);
        positives.push_back(rows);
    }
    try {
        DataSet users(block(nu, 0, 60, 7)), items(block(ni, 60, 90, 11));
        HipBPR bpr(users, items, positives, 2, 100, 5, 0.05, 0.0, 1e-4, 1e-4, FMHIP_LOSS_LOGISTIC, FMHIP_OPT_SGD, 1e-10, 0.1, 1, HipBPR::kAuto, 1.0,
                   HipBPR::kEpoch, HipBPR::kPopularity, 0.75, 1.0);
        FMModel fm(n1 - 1, k);
        fm.w0 = 0.1;
        for (int i = 0; i < n1; ++i) {
            fm.w[(size_t)i] = 0.02 * ((i % 7) - 3);
            for (int f = 0; f < k; ++f) fm.v[(size_t)(f + i * k)] = 0.01 * ((f * 7 + i * 3) % 11 - 5);
        }
        int weighted = -1;
        check(fmhip_proposal_get(bpr.handle(), &weighted));
        if (weighted != 1 || (int)bpr.proposal().size() != ni) return 1;
        print("weights", bpr.proposal());
        std::vector<uint32_t> thresh((size_t)ni);
        std::vector<int32_t> alias((size_t)ni);
        check(fmhip_proposal_table(bpr.handle(), thresh.data(), alias.data()));
        print("thresh", as_doubles(thresh));
        print("alias", as_doubles(alias));
        bpr.resample(2);
        print("neg", as_doubles(bpr.negatives()));
        print("stats", {(double)bpr.sample_stats.attempts, (double)bpr.sample_stats.forced});
        bpr.learn(fm);
        print("neg1", as_doubles(bpr.negatives()));
        print("w0", {fm.w0});
        print("w", fm.w);
        print("v", fm.v);
        // refusals leave the proposal; the empty vector is the uniform proposal
        const std::vector<double> before = bpr.proposal();
        std::vector<double> bad = before;
        bad[3] = 0.0;
        if (!refused([&] { bpr.setProposal(bad); }, "finite and > 0") || bpr.proposal() != before) return 1;
        if (!refused([&] { bpr.setProposal(std::vector<double>(5, 1.0)); }, "one weight per candidate row") || bpr.proposal() != before) return 1;
        if (fmhip_proposal_set(bpr.handle(), bad.data()) != FMHIP_ERR_INVALID || std::string(fmhip_last_error()).find("weights[3]") == std::string::npos)
            return 1;
        check(fmhip_proposal_get(bpr.handle(), &weighted));
        if (weighted != 1) return 1;
        bpr.setProposal({});
        check(fmhip_proposal_get(bpr.handle(), &weighted));
        if (weighted != 0 || !bpr.proposal().empty()) return 1;
        if (fmhip_proposal_table(bpr.handle(), thresh.data(), alias.data()) != FMHIP_ERR_INVALID) return 1;
        bpr.resample(2);
        print("neg_uniform", as_doubles(bpr.negatives()));
        if (!refused([&] { HipBPR r(users, items, positives, 1, 0, 0, 0.05, 0.0, 0.0, 0.0, FMHIP_LOSS_LOGISTIC, FMHIP_OPT_SGD, 1e-10, 0.1, 1, HipBPR::kAuto, 1.0,
                                    HipBPR::kEpoch, 2); }, "negatives"))
            return 1;
        if (!refused([&] { HipBPR r(users, items, positives, 1, 0, 0, 0.05, 0.0, 0.0, 0.0, FMHIP_LOSS_LOGISTIC, FMHIP_OPT_SGD, 1e-10, 0.1, 1, HipBPR::kAuto, 1.0,
                                    HipBPR::kEpoch, HipBPR::kPopularity, 0.75, 0.0); }, "smooth"))
            return 1;
    } catch (const Error &e) {
        fprintf(stderr, "error %d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}
