// host_mcmc_groups_harness.cpp — the host plan of the MCMC learner's grouped hyper-parameter sums (sparkfm_amd/csrc/fmhip_host.cpp:
// mcmc_group_plan, mcmc_bad_group) as a stand-alone program, built with -fsanitize=address,undefined:
//   host_mcmc_groups_harness check <seed>    random shapes and the edge cases -> "checks ok"
//   host_mcmc_groups_harness draw <seed>     the epoch's hyper-parameter draws (fmhip_host.h: mcmc_draw_state) -> "draws ok"
// Every shape is checked for: the chunks cover every trained slot exactly once; they sit in group order; no chunk crosses a group
// or holds more than the chunk size; a group's slots keep their ascending order (the plan is stable); m_a is right; quirk Q1's
// slot (id = num_attribute) is in no chunk whatever group it was given.
// draw: mcmc_draw_state for k + 1 = 3 over the three shapes its callers give it — one group with 4 partials (the flat handle), three
// groups with 0, 1 and 5 partials (the grouped handle; the empty group draws from the prior), and two parts' 4 partials each added
// as one run (the relational handle) — against mcmc_draw_alpha / mcmc_draw_group called one at a time on sums added sequentially in
// that order, stream id g + (a << 16): exact equality.  The probit form leaves alpha as it was.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../sparkfm_amd/csrc/fmhip_host.h"

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

static uint64_t rng_state = 1;
static uint32_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}

// cfeat: ascending feature ids of the compressed columns (the last may be num_attribute: quirk Q1's slot)
static void check_plan(const char *what, const std::vector<int32_t> &cfeat, int64_t num_attribute, const std::vector<int32_t> &group, int32_t G, int chunk) {
    McmcGroupPlan plan;
    mcmc_group_plan(cfeat.data(), (int64_t)cfeat.size(), num_attribute, group.data(), G, chunk, &plan);
    const size_t n_chunks = plan.chunk_group.size();
    CHECK(plan.chunk_ptr.size() == n_chunks + 1 && plan.chunk_ptr[0] == 0, "%s: chunk_ptr has %zu entries for %zu chunks", what, plan.chunk_ptr.size(), n_chunks);
    CHECK(plan.group_chunks.size() == (size_t)G + 1 && plan.counts.size() == (size_t)G, "%s: per-group tables", what);
    CHECK((size_t)plan.chunk_ptr[n_chunks] == plan.order.size(), "%s: the chunks end at %d, order holds %zu", what, plan.chunk_ptr[n_chunks], plan.order.size());
    std::vector<int64_t> want((size_t)G, 0);
    int64_t trained = 0;
    for (int32_t f : cfeat)
        if (f < num_attribute) { ++want[(size_t)group[(size_t)f]]; ++trained; }
    CHECK((int64_t)plan.order.size() == trained, "%s: %zu slots planned, %lld trained", what, plan.order.size(), (long long)trained);
    for (int a = 0; a < G; ++a) CHECK(plan.counts[(size_t)a] == want[(size_t)a], "%s: m_%d = %lld, want %lld", what, a, (long long)plan.counts[(size_t)a], (long long)want[(size_t)a]);
    std::vector<int> seen(cfeat.size(), 0);
    std::vector<int32_t> last((size_t)G, -1);
    for (size_t c = 0; c < n_chunks; ++c) {
        const int lo = plan.chunk_ptr[c], hi = plan.chunk_ptr[c + 1], a = plan.chunk_group[c];
        CHECK(hi > lo && hi - lo <= chunk, "%s: chunk %zu holds %d slots (at most %d)", what, c, hi - lo, chunk);
        CHECK(a >= 0 && a < G, "%s: chunk %zu of group %d", what, c, a);
        if (c) CHECK(plan.chunk_group[c - 1] <= a, "%s: chunk %zu of group %d follows one of group %d", what, c, a, plan.chunk_group[c - 1]);
        CHECK((int)c >= plan.group_chunks[(size_t)a] && (int)c < plan.group_chunks[(size_t)a + 1], "%s: chunk %zu outside its group's range", what, c);
        for (int p = lo; p < hi; ++p) {
            const int32_t s = plan.order[(size_t)p];
            CHECK(s >= 0 && (size_t)s < cfeat.size(), "%s: slot %d", what, s);
            if (s < 0 || (size_t)s >= cfeat.size()) continue;
            ++seen[(size_t)s];
            CHECK(cfeat[(size_t)s] < num_attribute, "%s: the untrained slot %d is planned", what, s);
            if (cfeat[(size_t)s] < num_attribute) CHECK(group[(size_t)cfeat[(size_t)s]] == a, "%s: slot %d of group %d in a chunk of group %d", what, s, group[(size_t)cfeat[(size_t)s]], a);
            CHECK(s > last[(size_t)a], "%s: group %d's slots out of order (%d after %d)", what, a, s, last[(size_t)a]);
            last[(size_t)a] = s;
        }
    }
    for (int a = 0; a < G; ++a) {
        const int nc = plan.group_chunks[(size_t)a + 1] - plan.group_chunks[(size_t)a];
        CHECK(nc == (int)((want[(size_t)a] + chunk - 1) / chunk), "%s: group %d has %d chunks for %lld slots", what, a, nc, (long long)want[(size_t)a]);
    }
    for (size_t s = 0; s < cfeat.size(); ++s) CHECK(seen[s] == (cfeat[s] < num_attribute ? 1 : 0), "%s: slot %zu planned %d times", what, s, seen[s]);
}

static double rnd_double() { return (double)rnd() / 2147483648.0 * 4.0 - 2.0; }

// partials[g][a]: the (sum theta, sum dev^2) pairs of (g, a) in the order they are added
static void check_draw(const char *what, uint64_t seed, uint32_t t, int G, const std::vector<int> &n_partials, const std::vector<int64_t> &counts) {
    const int k1 = 3;
    McmcPriors pri;
    pri.alpha_0 = 1.5; pri.beta_0 = 0.5; pri.alpha_lambda = 2.0; pri.beta_lambda = 0.25; pri.gamma_0 = 3.0; pri.mu_0 = -0.5;
    std::vector<std::vector<double>> partials((size_t)k1 * (size_t)G);
    for (int g = 0; g < k1; ++g)
        for (int a = 0; a < G; ++a)
            for (int c = 0; c < n_partials[(size_t)a]; ++c) {
                partials[(size_t)g * G + a].push_back(rnd_double());
                partials[(size_t)g * G + a].push_back(rnd_double() * rnd_double() + 4.0);      // a sum of squares: positive
            }
    std::vector<double> lambda0((size_t)k1 * (size_t)G), mu0((size_t)k1 * (size_t)G);
    for (size_t i = 0; i < lambda0.size(); ++i) {
        lambda0[i] = 0.5 + (double)(rnd() % 100) / 10.0;
        mu0[i] = rnd_double();
    }
    const int64_t n_rows = 1 + rnd() % 1000;
    const double sse = 0.25 + (double)(rnd() % 1000);
    const auto count_of = [&](int a) { return counts[(size_t)a]; };
    const auto partials_of = [&](int g, int a, auto add) {
        const std::vector<double> &v = partials[(size_t)g * G + a];
        for (size_t c = 0; c < v.size(); c += 2) add(v[c], v[c + 1]);
    };
    for (int probit = 0; probit < 2; ++probit) {
        double alpha = 7.25;
        std::vector<double> lambda = lambda0, mu = mu0;
        mcmc_draw_state(seed, t, pri, probit != 0, n_rows, sse, k1, G, count_of, partials_of, &alpha, lambda.data(), mu.data());
        const double want_alpha = probit ? 7.25 : mcmc_draw_alpha(seed, t, pri, n_rows, sse);
        CHECK(alpha == want_alpha, "%s, probit %d: alpha = %.17g, want %.17g", what, probit, alpha, want_alpha);
        for (int g = 0; g < k1; ++g)
            for (int a = 0; a < G; ++a) {
                const size_t at = (size_t)g * G + a;
                double sum_theta = 0.0, sum_dev2 = 0.0;
                for (size_t c = 0; c < partials[at].size(); c += 2) {
                    sum_theta += partials[at][c];
                    sum_dev2 += partials[at][c + 1];
                }
                double want_lambda = lambda0[at], want_mu = mu0[at];
                mcmc_draw_group(seed, t, (uint32_t)g + ((uint32_t)a << 16), pri, counts[(size_t)a], sum_theta, sum_dev2, mu0[at], &want_lambda, &want_mu);
                CHECK(lambda[at] == want_lambda && mu[at] == want_mu, "%s, probit %d, (g, a) = (%d, %d): lambda %.17g mu %.17g, want %.17g %.17g", what, probit, g,
                      a, lambda[at], mu[at], want_lambda, want_mu);
                CHECK(want_lambda != lambda0[at] && want_mu != mu0[at], "%s: (%d, %d) was not drawn", what, g, a);
            }
    }
}

static int draws(uint64_t seed) {
    for (uint32_t t = 0; t < 3; ++t) {
        check_draw("one group, 4 partials", seed, t, 1, {4}, {11});
        check_draw("three groups, 0 / 1 / 5 partials", seed, t, 3, {0, 1, 5}, {0, 300, 2100});
        check_draw("two parts of 4 partials as one run", seed, t, 1, {2 * 4}, {64});
    }
    if (fails) {
        fprintf(stderr, "%d checks failed\n", fails);
        return 1;
    }
    printf("draws ok\n");
    return 0;
}

int main(int argc, char **argv) {
    rng_state = argc > 2 ? strtoull(argv[2], nullptr, 10) : 1u;
    if (argc > 1 && !strcmp(argv[1], "draw")) return draws(rng_state);
    // ---- the edge cases
    {
        const int64_t n = 10;
        std::vector<int32_t> all(n + 1), g(n, 0);
        for (int i = 0; i <= n; ++i) all[(size_t)i] = i;                 // every feature present, and quirk Q1's slot
        check_plan("G = 1", all, n, g, 1, 4);
        check_plan("G = 1, one chunk", all, n, g, 1, 512);
        check_plan("a group with no slot", all, n, g, 3, 4);             // groups 1 and 2 are empty
        std::vector<int32_t> lastg(n, 4);
        check_plan("all features in the last group", all, n, lastg, 5, 3);
        std::vector<int32_t> alt(n);
        for (int i = 0; i < n; ++i) alt[(size_t)i] = i % 3;
        check_plan("interleaved", all, n, alt, 3, 2);
        check_plan("chunk of one", all, n, alt, 4, 1);
        check_plan("no columns", std::vector<int32_t>(), n, alt, 3, 4);
        check_plan("only the untrained slot", std::vector<int32_t>(1, (int32_t)n), n, alt, 3, 4);
        // equal ids: stable — group 1's slots are exactly the odd positions, ascending
        McmcGroupPlan plan;
        std::vector<int32_t> two(n);
        for (int i = 0; i < n; ++i) two[(size_t)i] = i & 1;
        mcmc_group_plan(all.data(), n + 1, n, two.data(), 2, 512, &plan);
        const int32_t want[] = {0, 2, 4, 6, 8, 1, 3, 5, 7, 9};
        CHECK(plan.order.size() == 10 && !memcmp(plan.order.data(), want, sizeof want), "the plan is not stable");
        CHECK(plan.counts[0] == 5 && plan.counts[1] == 5, "m = %lld, %lld", (long long)plan.counts[0], (long long)plan.counts[1]);
        // the table's validation
        CHECK(mcmc_bad_group(alt.data(), n, 3) == -1, "a valid table is refused");
        CHECK(mcmc_bad_group(alt.data(), n, 2) == 2, "id 2 passes with two groups");
        alt[7] = -1;
        CHECK(mcmc_bad_group(alt.data(), n, 3) == 7, "a negative id passes");
        CHECK(mcmc_bad_group(alt.data(), 0, 1) == -1, "an empty table is refused");
    }
    // ---- random shapes: sparse column sets, with and without the untrained slot, every chunk size around the group sizes
    for (int round = 0; round < 300; ++round) {
        const int64_t n = 1 + rnd() % 700;
        const int32_t G = 1 + (int32_t)(rnd() % (round % 3 == 0 ? 40 : 5));
        std::vector<int32_t> group((size_t)n), cfeat;
        const uint32_t mode = rnd() % 3;
        for (int64_t i = 0; i < n; ++i) group[(size_t)i] = mode == 0 ? (int32_t)(rnd() % (uint32_t)G) : mode == 1 ? (int32_t)(i * G / n) : G - 1;
        const uint32_t keep = 1 + rnd() % 4;
        for (int64_t i = 0; i < n; ++i)
            if (rnd() % 4 < keep) cfeat.push_back((int32_t)i);
        if (rnd() & 1) cfeat.push_back((int32_t)n);
        const int chunk = 1 + (int)(rnd() % (round % 2 ? 7 : 600));
        check_plan("random", cfeat, n, group, G, chunk);
    }
    if (fails) {
        fprintf(stderr, "%d checks failed\n", fails);
        return 1;
    }
    printf("checks ok\n");
    return 0;
}
