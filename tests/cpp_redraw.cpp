// cpp_redraw.cpp — include/sparkfm.hpp's HipBPR with redraw = kBatch (include/fmhip_redraw.h) over the integer formulas of
// cpp_bpr.cpp: the best of 4 candidates, batches of 100 pairs (n_neg = 2), one per-batch epoch by learn and a second one batch by
// batch through step(fm, batch, t).  Prints "mode", "neg" and "stats" (pairs, attempts, forced, replaced, violated, trials) after
// the first epoch, "neg2" and the summed "stats2" after the second, and the parameters "w0", "w", "v", every number as a hex float,
// for tests/test_gpu_redraw.py, whose Python mirror must give the same bits.  Then mode set and get, and the refusals.
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

static std::vector<double> six(const fmhip_redraw_stats &s) {
    return {(double)s.pairs, (double)s.attempts, (double)s.forced, (double)s.replaced, (double)s.violated, (double)s.trials};
}

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
        HipBPR bpr(users, items, positives, 2, 100, 5, 0.05, 0.0, 1e-4, 1e-4, FMHIP_LOSS_LOGISTIC, FMHIP_OPT_SGD, 1e-10, 0.1, 4, HipBPR::kAuto, 1.0,
                   HipBPR::kBatch);
        FMModel fm(n1 - 1, k);
        fm.w0 = 0.1;
        for (int i = 0; i < n1; ++i) {
            fm.w[(size_t)i] = 0.02 * ((i % 7) - 3);
            for (int f = 0; f < k; ++f) fm.v[(size_t)(f + i * k)] = 0.01 * ((f * 7 + i * 3) % 11 - 5);
        }
        int mode = -1;
        check(fmhip_redraw_get(bpr.handle(), &mode));
        if (mode != FMHIP_REDRAW_BATCH || bpr.redraw() != HipBPR::kBatch) return 1;
        print("mode", {(double)mode});
        // no per-batch epoch yet: its counters are refused by the library
        fmhip_redraw_stats none{};
        if (fmhip_redraw_epoch_stats(bpr.handle(), &none) != FMHIP_ERR_INVALID) return 1;
        bpr.learn(fm);
        if (bpr.last_stats.rows != 2 * bpr.n_pairs() || bpr.last_stats.sum_e != 0.0 || bpr.redraw_stats.pairs != bpr.n_pairs()) return 1;
        print("neg", as_doubles(bpr.negatives()));
        print("stats", six(bpr.redraw_stats));
        // the second epoch, batch by batch
        int64_t n_batches = 0;
        check(fmhip_bpr_info(bpr.handle(), nullptr, nullptr, nullptr, &n_batches, nullptr));
        fmhip_redraw_stats sum{};
        for (int64_t b = 0; b < n_batches; ++b) {
            bpr.step(fm, b, 1);
            sum.pairs += bpr.redraw_stats.pairs;
            sum.attempts += bpr.redraw_stats.attempts;
            sum.forced += bpr.redraw_stats.forced;
            sum.replaced += bpr.redraw_stats.replaced;
            sum.violated += bpr.redraw_stats.violated;
            sum.trials += bpr.redraw_stats.trials;
        }
        print("neg2", as_doubles(bpr.negatives()));
        print("stats2", six(sum));
        print("w0", {fm.w0});
        print("w", fm.w);
        print("v", fm.v);
        // set and get; a value that is no mode is refused and leaves the mode
        check(fmhip_redraw_set(bpr.handle(), FMHIP_REDRAW_EPOCH));
        check(fmhip_redraw_get(bpr.handle(), &mode));
        if (mode != FMHIP_REDRAW_EPOCH) return 1;
        if (fmhip_redraw_set(bpr.handle(), 2) != FMHIP_ERR_INVALID || fmhip_redraw_set(bpr.handle(), -1) != FMHIP_ERR_INVALID) return 1;
        check(fmhip_redraw_get(bpr.handle(), &mode));
        if (mode != FMHIP_REDRAW_EPOCH) return 1;
        // a bad batch, a bad epoch: refused by the library; a bad redraw: at construction
        if (!refused([&] { bpr.step(fm, n_batches, 1); }, "out of range") || !refused([&] { bpr.step(fm, 0, -1); }, "t = -1")) return 1;
        if (!refused([&] { HipBPR r(users, items, positives, 1, 0, 0, 0.05, 0.0, 0.0, 0.0, FMHIP_LOSS_LOGISTIC, FMHIP_OPT_SGD, 1e-10, 0.1, 1, HipBPR::kAuto, 1.0, 2); },
                     "redraw"))
            return 1;
    } catch (const Error &e) {
        fprintf(stderr, "error %d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}
