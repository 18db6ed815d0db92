// host_sgda_harness.cpp — the host plan of the SGDA learner's grouped sums (sparkfm_amd/csrc/fmhip_host.cpp: sgda_group_plan) as a
// stand-alone program, built with -fsanitize=address,undefined:
//   host_sgda_harness check <seed>    the named cases and random shapes -> "checks ok"
// Every shape is checked for: every feature id appears in exactly one chunk; the chunks sit in group order; no chunk straddles a group
// or holds more than the chunk length; ids ascend inside a group (the plan is stable); an empty group has no chunk; counts[a] is the
// group's size; a group of m features has ceil(m / chunk) chunks.
// Named cases: G = 1; G = 3 with interleaved ids (i % 3); a group of exactly the chunk length; one of chunk length + 1; a group with
// no feature; no feature at all.
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

static void check_plan(const char *what, const std::vector<int32_t> &group, int32_t G, int chunk) {
    const int64_t n = (int64_t)group.size();
    CHECK(mcmc_bad_group(group.data(), n, G) < 0, "%s: the case's own table is out of range", what);
    McmcGroupPlan plan;
    sgda_group_plan(group.data(), n, G, chunk, &plan);
    const size_t n_chunks = plan.chunk_group.size();
    CHECK(plan.chunk_ptr.size() == n_chunks + 1 && plan.chunk_ptr[0] == 0, "%s: chunk_ptr has %zu entries for %zu chunks", what, plan.chunk_ptr.size(), n_chunks);
    CHECK(plan.group_chunks.size() == (size_t)G + 1 && plan.counts.size() == (size_t)G, "%s: per-group tables", what);
    CHECK(plan.group_chunks[0] == 0 && (size_t)plan.group_chunks[(size_t)G] == n_chunks, "%s: group_chunks does not span the chunks", what);
    CHECK((int64_t)plan.order.size() == n && (int64_t)plan.chunk_ptr[n_chunks] == n, "%s: %zu ids planned for %lld features", what, plan.order.size(), (long long)n);
    std::vector<int64_t> want((size_t)G, 0);
    for (int32_t a : group) ++want[(size_t)a];
    std::vector<int> seen((size_t)n, 0);
    std::vector<int32_t> last((size_t)G, -1);
    for (size_t c = 0; c < n_chunks; ++c) {
        const int lo = plan.chunk_ptr[c], hi = plan.chunk_ptr[c + 1], a = plan.chunk_group[c];
        CHECK(hi > lo && hi - lo <= chunk, "%s: chunk %zu holds %d ids (1 .. %d)", what, c, hi - lo, chunk);
        CHECK(a >= 0 && a < G, "%s: chunk %zu of group %d", what, c, a);
        if (a < 0 || a >= G) continue;
        if (c) CHECK(plan.chunk_group[c - 1] <= a, "%s: chunk %zu of group %d follows one of group %d", what, c, a, plan.chunk_group[c - 1]);
        CHECK((int)c >= plan.group_chunks[(size_t)a] && (int)c < plan.group_chunks[(size_t)a + 1], "%s: chunk %zu outside its group's range", what, c);
        for (int p = lo; p < hi && (size_t)p < plan.order.size(); ++p) {
            const int32_t i = plan.order[(size_t)p];
            CHECK(i >= 0 && i < n, "%s: id %d", what, i);
            if (i < 0 || i >= n) continue;
            ++seen[(size_t)i];
            CHECK(group[(size_t)i] == a, "%s: feature %d of group %d in a chunk of group %d", what, i, group[(size_t)i], a);      // no straddling
            CHECK(i > last[(size_t)a], "%s: group %d's ids out of order (%d after %d)", what, a, i, last[(size_t)a]);
            last[(size_t)a] = i;
        }
    }
    for (int a = 0; a < G; ++a) {
        const int nc = plan.group_chunks[(size_t)a + 1] - plan.group_chunks[(size_t)a];
        CHECK(plan.counts[(size_t)a] == want[(size_t)a], "%s: counts[%d] = %lld, want %lld", what, a, (long long)plan.counts[(size_t)a], (long long)want[(size_t)a]);
        CHECK(nc == (int)((want[(size_t)a] + chunk - 1) / chunk), "%s: group %d has %d chunks for %lld ids", what, a, nc, (long long)want[(size_t)a]);
    }
    for (int64_t i = 0; i < n; ++i) CHECK(seen[(size_t)i] == 1, "%s: feature %lld planned %d times", what, (long long)i, seen[(size_t)i]);
}

int main(int argc, char **argv) {
    if (argc != 3 || strcmp(argv[1], "check") != 0) {
        fprintf(stderr, "usage: host_sgda_harness check <seed>\n");
        return 2;
    }
    rng_state = strtoull(argv[2], nullptr, 10) | 1;
    const int chunk = kSgdaChunk;
    check_plan("G = 1", std::vector<int32_t>(37, 0), 1, chunk);
    check_plan("G = 1, three chunks", std::vector<int32_t>((size_t)2 * chunk + 5, 0), 1, chunk);
    {
        std::vector<int32_t> g(203);
        for (size_t i = 0; i < g.size(); ++i) g[i] = (int32_t)(i % 3);
        check_plan("G = 3 interleaved", g, 3, chunk);
        check_plan("G = 3 interleaved, chunk 7", g, 3, 7);
    }
    {
        std::vector<int32_t> g((size_t)chunk, 1);       // group 1: exactly a chunk; group 0: a chunk + 1; group 2: empty; group 3: one id
        g.insert(g.end(), (size_t)chunk + 1, 0);
        g.push_back(3);
        check_plan("chunk, chunk + 1, empty, one", g, 4, chunk);
        McmcGroupPlan plan;
        sgda_group_plan(g.data(), (int64_t)g.size(), 4, chunk, &plan);
        CHECK(plan.group_chunks == (std::vector<int32_t>{0, 2, 3, 3, 4}), "the named case's chunks per group");
        CHECK(plan.chunk_ptr == (std::vector<int32_t>{0, chunk, chunk + 1, 2 * chunk + 1, 2 * chunk + 2}), "the named case's chunk bounds");
        CHECK(plan.order[0] == chunk && plan.order[(size_t)chunk] == 2 * chunk && plan.order[(size_t)chunk + 1] == 0, "the named case's order");
    }
    check_plan("an empty leading and trailing group", std::vector<int32_t>(9, 1), 3, chunk);
    check_plan("no feature", std::vector<int32_t>(), 2, chunk);
    for (int it = 0; it < 300; ++it) {
        const int32_t G = 1 + (int32_t)(rnd() % 9);
        const int c = 1 + (int)(rnd() % 40);
        std::vector<int32_t> g(rnd() % 400);
        const bool skewed = rnd() % 2;
        for (auto &a : g) a = skewed ? (int32_t)((rnd() % 8 < 6) ? 0 : rnd() % G) : (int32_t)(rnd() % G);
        check_plan("random", g, G, c);
    }
    // a bad id is found, the first one
    {
        std::vector<int32_t> g{0, 1, 2, -1, 5};
        CHECK(mcmc_bad_group(g.data(), 5, 3) == 3 && mcmc_bad_group(g.data(), 3, 3) < 0 && mcmc_bad_group(g.data(), 3, 2) == 2, "mcmc_bad_group");
    }
    if (fails) {
        fprintf(stderr, "%d checks failed\n", fails);
        return 1;
    }
    printf("checks ok\n");
    return 0;
}
