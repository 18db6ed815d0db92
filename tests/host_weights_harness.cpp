// host_weights_harness.cpp — the example weights' validation pass (validate_weights, sparkfm_amd/csrc/fmhip_host.cpp) as a stand-alone
// program under AddressSanitizer and UBSan: seeded weight arrays of many lengths, each with no, one or several offending entries
// (NaN, +-inf, beyond FLT_MAX, negative) at seeded rows, over 1 .. 7 threads; the answer must be the FIRST offending row, or -1.
//   host_weights_harness <seed> <cases>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

#include "../sparkfm_amd/csrc/fmhip_host.h"

using fmhip::host::validate_weights;

static int fails = 0;
#define CHECK(cond, ...)                          \
    do {                                          \
        if (!(cond)) {                            \
            ++fails;                              \
            fprintf(stderr, "FAIL %s: ", #cond);  \
            fprintf(stderr, __VA_ARGS__);         \
            fprintf(stderr, "\n");                \
        }                                         \
    } while (0)

int main(int argc, char **argv) {
    const unsigned seed = argc > 1 ? (unsigned)strtoul(argv[1], nullptr, 10) : 1u;
    const int cases = argc > 2 ? atoi(argv[2]) : 200;
    std::mt19937_64 gen(seed);
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double bad_values[] = {nan, inf, -inf, -1.0, -1e-300, -DBL_MIN, 2.0 * (double)FLT_MAX, DBL_MAX};
    const double good_values[] = {0.0, -0.0, 0.25, 1.0, 3.5, 1e-300, DBL_MIN, (double)FLT_MAX, 20.0};
    const int n_bad = (int)(sizeof bad_values / sizeof bad_values[0]), n_good = (int)(sizeof good_values / sizeof good_values[0]);
    // the degenerate shapes first
    CHECK(validate_weights(0, nullptr, 1) == -1, "no rows");
    CHECK(validate_weights(0, nullptr, 5) == -1, "no rows, five threads");
    for (int v = 0; v < n_bad; ++v) {
        const double one = bad_values[v];
        CHECK(validate_weights(1, &one, 1) == 0, "one bad row (value %d)", v);
        CHECK(validate_weights(1, &one, 3) == 0, "one bad row, three threads (value %d)", v);
    }
    for (int v = 0; v < n_good; ++v) {
        const double one = good_values[v];
        CHECK(validate_weights(1, &one, 2) == -1, "one good row (value %d)", v);
    }
    for (int c = 0; c < cases; ++c) {
        const int64_t n = 1 + (int64_t)(gen() % (c % 7 == 0 ? 70000 : 300));
        std::vector<double> w((size_t)n);      // exactly n doubles: a read past the end is the sanitizer's to find
        for (auto &x : w) x = good_values[gen() % n_good];
        int64_t first = -1;
        const int plant = (int)(gen() % 4);    // 0: all good
        for (int p = 0; p < plant; ++p) {
            const int64_t at = (int64_t)(gen() % (uint64_t)n);
            w[(size_t)at] = bad_values[gen() % n_bad];
            if (first < 0 || at < first) first = at;
        }
        for (int threads = 1; threads <= 7; ++threads) {
            const int64_t got = validate_weights(n, w.data(), threads);
            CHECK(got == first, "case %d: n %lld, %d threads: first bad row %lld, expected %lld", c, (long long)n, threads, (long long)got,
                  (long long)first);
        }
    }
    if (fails) {
        fprintf(stderr, "%d checks failed\n", fails);
        return 1;
    }
    printf("checks ok (%d cases)\n", cases);
    return 0;
}
