// host_probit_harness.cpp — the host arithmetic of the MCMC learner's tasks (sparkfm_amd/csrc/fmhip_host.cpp over mcmc_rng.h: the
// truncated-normal draw of the probit link, its expectation, the task and clip validation) as a stand-alone program, built with
// -fsanitize=address,undefined:
//   host_probit_harness trunc <seed> <a> <n>     truncated_normal(seed, row i, t 5, a), i < n: the double's bits in hex and the attempts
//   host_probit_harness mean <a> [<a> ...]       E[z | z > a] of every argument: the doubles' bits in hex
//   host_probit_harness check <seed>             draws over a range of a (the support, the attempt bound, a that is not finite), the
//                                                expectation's range, the validation -> "checks ok"
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "../sparkfm_amd/csrc/fmhip_host.h"
#include "../sparkfm_amd/csrc/mcmc_rng.h"

using namespace fmhip::host;

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

static uint64_t bits(double x) {
    uint64_t b;
    memcpy(&b, &x, sizeof b);
    return b;
}

int main(int argc, char **argv) {
    const char *mode = argc > 1 ? argv[1] : "check";
    if (!strcmp(mode, "trunc") && argc > 4) {
        const uint64_t seed = strtoull(argv[2], nullptr, 10);
        const double a = atof(argv[3]);
        const int n = atoi(argv[4]);
        for (int i = 0; i < n; ++i) {
            int attempts = 0;
            const double z = mcmc_truncated_normal(seed, (uint32_t)i, 5, a, &attempts);
            printf("%016" PRIx64 " %d\n", bits(z), attempts);
        }
        return 0;
    }
    if (!strcmp(mode, "mean") && argc > 2) {
        for (int i = 2; i < argc; ++i) printf("%016" PRIx64 "\n", bits(mcmc_truncated_mean(atof(argv[i]))));
        return 0;
    }
    const uint64_t seed = argc > 2 ? strtoull(argv[2], nullptr, 10) : 1u;
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    // the support and the attempt bound over a range of truncation points; the same counter twice gives the same bits; a nullable out
    int most = 0;
    const double as[] = {-1e300, -40.0, -3.0, -0.5, -0.0, 0.0, 1e-300, 0.5, 3.0, 8.0, 40.0, 1e8, 1e300};
    for (double a : as)
        for (uint32_t r = 0; r < 600; ++r) {
            int attempts = 0;
            const double z = mcmc_truncated_normal(seed, r, 1 + r % 7, a, &attempts);
            CHECK(std::isfinite(z) && (z > a || (a >= 1e8 && z >= a)), "a = %g row %u: z = %g", a, r, z);
            CHECK(attempts >= 1 && attempts <= fmhip::rng::kTruncMaxAttempts, "a = %g row %u: %d attempts", a, r, attempts);
            CHECK(bits(z) == bits(mcmc_truncated_normal(seed, r, 1 + r % 7, a, nullptr)), "a = %g row %u is not a function of its counter", a, r);
            if (attempts > most) most = attempts;
        }
    CHECK(most > 1, "no draw needed a second attempt");
    // a truncation point that is not finite: the loop ends all the same
    const double odd[] = {nan, inf, -inf};
    for (double a : odd) {
        int attempts = 0;
        const double z = mcmc_truncated_normal(seed, 3, 1, a, &attempts);
        CHECK(attempts >= 1 && attempts <= fmhip::rng::kTruncMaxAttempts, "a = %g: %d attempts", a, attempts);
        CHECK(a == -inf ? std::isfinite(z) : true, "a = -inf: z = %g", z);
    }
    // the expectation: finite, above the truncation point and above 0
    for (double a = -1000.0; a <= 1000.0; a += 0.37) {
        const double h = mcmc_truncated_mean(a);
        CHECK(std::isfinite(h) && h >= a && h >= 0.0, "E[z | z > %g] = %g", a, h);
    }
    // the task and the clip
    CHECK(mcmc_bad_task(0, 0, 0.0, 0.0) == nullptr && mcmc_bad_task(1, 0, nan, nan) == nullptr, "a task without clip is refused");
    CHECK(mcmc_bad_task(0, 1, 1.0, 5.0) == nullptr, "a regression clip is refused");
    CHECK(mcmc_bad_task(2, 0, 0.0, 0.0) && strstr(mcmc_bad_task(2, 0, 0.0, 0.0), "unknown task"), "task 2 passes");
    CHECK(mcmc_bad_task(-1, 0, 0.0, 0.0) != nullptr, "task -1 passes");
    CHECK(mcmc_bad_task(1, 1, 1.0, 5.0) && strstr(mcmc_bad_task(1, 1, 1.0, 5.0), "regression task"), "clip with classification passes");
    CHECK(mcmc_bad_task(0, 1, 5.0, 5.0) && strstr(mcmc_bad_task(0, 1, 5.0, 5.0), "clip range"), "an empty clip range passes");
    CHECK(mcmc_bad_task(0, 1, 5.0, 1.0) != nullptr && mcmc_bad_task(0, 1, nan, 1.0) != nullptr && mcmc_bad_task(0, 1, 0.0, inf) != nullptr,
          "a reversed, nan or infinite clip range passes");
    if (fails) {
        fprintf(stderr, "%d checks failed\n", fails);
        return 1;
    }
    printf("checks ok (most attempts of a truncated normal: %d)\n", most);
    return 0;
}
