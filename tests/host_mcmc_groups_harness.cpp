// host_mcmc_groups_harness.cpp — the host plan of the MCMC learner's grouped hyper-parameter sums (sparkfm_amd/csrc/fmhip_host.cpp:
// mcmc_group_plan, mcmc_bad_group) as a stand-alone program, built with -fsanitize=address,undefined:
//   host_mcmc_groups_harness check <seed>    random shapes and the edge cases -> "checks ok"
// Every shape is checked for: the chunks cover every trained slot exactly once; they sit in group order; no chunk crosses a group
// or holds more than the chunk size; a group's slots keep their ascending order (the plan is stable); m_a is right; quirk Q1's
// slot (id = num_attribute) is in no chunk whatever group it was given.
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

int main(int argc, char **argv) {
    rng_state = argc > 2 ? strtoull(argv[2], nullptr, 10) : 1u;
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
