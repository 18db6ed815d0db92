// cpp_softmax.cpp — include/sparkfm.hpp's HipBPR with loss = kSoftmax (include/fmhip_softmax.h) over the integer formulas of
// cpp_bpr.cpp: n_neg = 3, batches of 99 pairs, the popularity proposal with logq.  Prints "weights" (the proposal), "logq" (the
// library's table), "neg" and the parameters "w0", "w", "v" after two epochs by learn, "probs", "loss" and "top1", every number as
// a hex float, for tests/test_gpu_softmax.py, whose Python mirror must give the same bits.  Then the refusals.
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
        HipBPR bpr(users, items, positives, 3, 99, 5, 0.05, 0.0, 1e-4, 1e-4, HipBPR::kSoftmax, FMHIP_OPT_SGD, 1e-10, 0.1, 1, HipBPR::kAuto, 1.0,
                   HipBPR::kEpoch, HipBPR::kPopularity, 0.75, 1.0, true);
        FMModel fm(n1 - 1, k);
        fm.w0 = 0.1;
        for (int i = 0; i < n1; ++i) {
            fm.w[(size_t)i] = 0.02 * ((i % 7) - 3);
            for (int f = 0; f < k; ++f) fm.v[(size_t)(f + i * k)] = 0.01 * ((f * 7 + i * 3) % 11 - 5);
        }
        int enabled = -1, logq = -1;
        check(fmhip_softmax_get(bpr.handle(), &enabled, &logq));
        if (enabled != 1 || logq != 1 || !bpr.softmax() || (int)bpr.logq().size() != ni) return 1;
        print("weights", bpr.proposal());
        print("logq", as_doubles(bpr.logq()));
        if (!refused([&] { bpr.softmaxProbs(); }, "no softmax probabilities stand")) return 1;
        bpr.learn(fm);
        bpr.learn(fm);
        print("neg", as_doubles(bpr.negatives()));
        print("w0", {fm.w0});
        print("w", fm.w);
        print("v", fm.v);
        print("probs", as_doubles(bpr.softmaxProbs()));
        print("loss", {bpr.computeSoftmaxLoss(fm)});
        print("top1", {bpr.computeTop1(fm)});
        print("stats", {(double)bpr.last_stats.rows, bpr.last_stats.sum_e, bpr.last_stats.sse});
        // the refusals: WARP beside the softmax in both orders, a batch that splits an interaction
        if (fmhip_warp_set(bpr.handle(), 1, 1.0) != FMHIP_ERR_INVALID || std::string(fmhip_last_error()).find("softmax switch is on") == std::string::npos)
            return 1;
        if (!refused([&] { HipBPR r(users, items, positives, 3, 99, 5, 0.05, 0.0, 0.0, 0.0, HipBPR::kSoftmax, FMHIP_OPT_SGD, 1e-10, 0.1, 4, HipBPR::kWarp); },
                     "choose one"))
            return 1;
        if (!refused([&] { HipBPR r(users, items, positives, 3, 100, 5, 0.05, 0.0, 0.0, 0.0, HipBPR::kSoftmax); }, "batch_pairs = 100 is no multiple of n_neg = 3"))
            return 1;
        // the uniform proposal: the correction is out of force, the table gone
        bpr.setProposal({});
        if (!bpr.logq().empty()) return 1;
        std::vector<float> lq((size_t)ni);
        if (fmhip_softmax_logq(bpr.handle(), lq.data()) != FMHIP_ERR_INVALID) return 1;
    } catch (const Error &e) {
        fprintf(stderr, "error %d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}
