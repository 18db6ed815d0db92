// host_mcmc_relational_harness.cpp — the host passes of the MCMC learner's block-structure sweep (sparkfm_amd/csrc/fmhip_host.cpp:
// mcmc_part_order, mcmc_block_counts, mcmc_block_trained) as a stand-alone program, built with -fsanitize=address,undefined:
//   host_mcmc_relational_harness check <seed>    random shapes and the edge cases -> "checks ok"
// Checked: the order is a permutation by ascending range start with the parts without features last and in place; disjoint ranges in
// any given order are accepted, interleaved ones are named (a's range starts lower, the feature is b's lowest and lies inside a's
// range); n_p sums to the rows and counts every block row's references; a column is trained exactly when its id is below
// num_attribute and one of its entries sits in a referenced block row (the flag bit of the row words ignored), and |T| is their count.
#include <algorithm>
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

static McmcPartOrder order_of(const std::vector<std::vector<int32_t>> &feat) {
    std::vector<const int32_t *> fp;
    std::vector<int64_t> fn;
    for (const auto &f : feat) {
        fp.push_back(f.data());
        fn.push_back((int64_t)f.size());
    }
    return mcmc_part_order((int)feat.size(), fp.data(), fn.data());
}

static void check_order(const char *what, const std::vector<std::vector<int32_t>> &feat, bool want_ok) {
    const McmcPartOrder po = order_of(feat);
    const int P = (int)feat.size();
    CHECK((int)po.order.size() == P, "%s: the order holds %zu parts of %d", what, po.order.size(), P);
    std::vector<int> seen((size_t)P, 0);
    for (int p : po.order)
        if (p >= 0 && p < P) ++seen[(size_t)p];
    for (int p = 0; p < P; ++p) CHECK(seen[(size_t)p] == 1, "%s: part %d occurs %d times", what, p, seen[(size_t)p]);
    auto lo = [&](int p) { return feat[(size_t)p].empty() ? INT32_MAX : *std::min_element(feat[(size_t)p].begin(), feat[(size_t)p].end()); };
    auto hi = [&](int p) { return feat[(size_t)p].empty() ? -1 : *std::max_element(feat[(size_t)p].begin(), feat[(size_t)p].end()); };
    for (int x = 0; x + 1 < P; ++x) {
        const int a = po.order[(size_t)x], b = po.order[(size_t)x + 1];
        CHECK(lo(a) <= lo(b), "%s: part %d (from %d) walks before part %d (from %d)", what, a, lo(a), b, lo(b));
        if (lo(a) == lo(b)) CHECK(a < b, "%s: parts %d and %d start alike and swapped places", what, a, b);
    }
    CHECK((po.a < 0) == want_ok, "%s: %s, a = %d b = %d feature = %d", what, want_ok ? "refused" : "accepted", po.a, po.b, (int)po.feature);
    if (po.a >= 0 && !want_ok) {
        CHECK(po.b >= 0 && po.b < P && po.a < P && po.a != po.b, "%s: parts %d, %d", what, po.a, po.b);
        CHECK(lo(po.a) <= lo(po.b), "%s: a does not start lower", what);
        CHECK(po.feature == lo(po.b) && po.feature <= hi(po.a), "%s: feature %d is not b's lowest inside a's range [%d, %d]", what, (int)po.feature, lo(po.a),
              hi(po.a));
    }
}

static void check_block(const char *what, int64_t n_rows, int64_t J, int64_t n_cols, int64_t num_attribute, bool plain) {
    std::vector<int32_t> map((size_t)n_rows);
    for (auto &m : map) m = (int32_t)(rnd() % (uint32_t)J);
    if (J > 2)
        for (auto &m : map)
            if (m == J - 1) m = 0;                                  // the last block row is referenced by nobody
    std::vector<double> n;
    mcmc_block_counts(map.data(), n_rows, J, n);
    CHECK((int64_t)n.size() == J, "%s: n holds %zu entries", what, n.size());
    double total = 0.0;
    for (double c : n) total += c;
    CHECK(total == (double)n_rows, "%s: n sums to %g of %lld rows", what, total, (long long)n_rows);
    std::vector<double> want_n((size_t)J, 0.0);
    for (int32_t m : map) want_n[(size_t)m] += 1.0;
    CHECK(want_n == n, "%s: n differs", what);
    // columns: ascending ids with gaps, the last one possibly num_attribute (quirk Q1's slot); random rows, flag bits set at random
    std::vector<int32_t> cfeat, cptr(1, 0);
    std::vector<uint32_t> crow;
    int32_t id = 0;
    for (int64_t s = 0; s < n_cols; ++s) {
        id += 1 + (int32_t)(rnd() % 3);
        cfeat.push_back(s == n_cols - 1 && rnd() % 2 ? (int32_t)num_attribute : std::min<int32_t>(id, (int32_t)num_attribute - 1));
        const int len = (int)(rnd() % 4);                           // (an empty column: never trained)
        for (int x = 0; x < len; ++x) crow.push_back((rnd() % 3 == 0 ? (uint32_t)(J - 1) : rnd() % (uint32_t)J) | (rnd() % 2 ? 0x80000000u : 0u));
        cptr.push_back((int32_t)crow.size());
    }
    std::vector<int32_t> trained;
    const int64_t count = mcmc_block_trained(cfeat.data(), cptr.data(), crow.data(), n_cols, num_attribute, plain ? nullptr : n.data(), trained);
    CHECK((int64_t)trained.size() == n_cols, "%s: trained holds %zu entries", what, trained.size());
    int64_t want_count = 0;
    for (int64_t s = 0; s < n_cols && (int64_t)trained.size() == n_cols; ++s) {
        bool used = false;
        for (int32_t p = cptr[(size_t)s]; p < cptr[(size_t)s + 1]; ++p) used = used || plain || n[crow[(size_t)p] & 0x7fffffffu] > 0.0;
        const int want = cfeat[(size_t)s] < num_attribute && used ? 1 : 0;
        CHECK(trained[(size_t)s] == want, "%s: column %lld (feature %d) trained = %d, want %d", what, (long long)s, (int)cfeat[(size_t)s], (int)trained[(size_t)s], want);
        want_count += want;
    }
    CHECK(count == want_count, "%s: |T| = %lld, want %lld", what, (long long)count, (long long)want_count);
}

int main(int argc, char **argv) {
    if (argc < 3 || strcmp(argv[1], "check") != 0) {
        fprintf(stderr, "usage: %s check <seed>\n", argv[0]);
        return 2;
    }
    rng_state = strtoull(argv[2], nullptr, 10) * 2654435761ull + 1;
    // the order: edge cases
    check_order("one part", {{3, 1, 2}}, true);
    check_order("given in range order", {{0, 1, 2}, {3, 4}, {5}}, true);
    check_order("given in another order", {{7, 9}, {0, 3}, {4, 6}}, true);
    check_order("a part without features", {{5, 6}, {}, {0, 1}}, true);
    check_order("no features at all", {{}, {}}, true);
    check_order("interleaved", {{0, 5}, {3, 9}}, false);
    check_order("nested", {{4, 5}, {0, 9}}, false);
    check_order("touching ends", {{0, 4}, {4, 8}}, false);
    check_order("the third part interleaves", {{0, 1}, {10, 20}, {15, 30}}, false);
    {
        const McmcPartOrder po = order_of({{10, 20}, {0, 15}});
        CHECK(po.a == 1 && po.b == 0 && po.feature == 10, "named parts: a = %d b = %d feature = %d", po.a, po.b, (int)po.feature);
    }
    for (int it = 0; it < 200; ++it) {
        // disjoint ranges handed out in a random order are accepted; moving one feature into another part's range is refused
        const int P = 1 + (int)(rnd() % 6);
        std::vector<std::vector<int32_t>> feat((size_t)P);
        std::vector<int> place((size_t)P);
        for (int p = 0; p < P; ++p) place[(size_t)p] = p;
        for (int p = P - 1; p > 0; --p) std::swap(place[(size_t)p], place[(size_t)(rnd() % (uint32_t)(p + 1))]);
        int32_t next = (int32_t)(rnd() % 5);
        for (int x = 0; x < P; ++x) {
            const int len = 2 + (int)(rnd() % 5);
            const bool down = rnd() % 2;                            // (the ids in either order: the range is what counts)
            for (int y = 0; y < len; ++y) feat[(size_t)place[(size_t)x]].push_back(next + (int32_t)(down ? len - 1 - y : y));
            next += len + (int32_t)(rnd() % 3);
        }
        check_order("random disjoint", feat, true);
        if (P > 1) {
            const int a = place[0], b = place[(size_t)P - 1];
            feat[(size_t)b].push_back(*std::min_element(feat[(size_t)a].begin(), feat[(size_t)a].end()) + 1);       // (a repeat across parts is the
            check_order("random interleaved", feat, false);                                                            // relational dataset's to refuse)
        }
    }
    // n_p and the trained columns
    check_block("one row", 1, 1, 1, 5, false);
    check_block("no columns", 10, 4, 0, 5, false);
    check_block("plain", 20, 20, 6, 12, true);
    for (int it = 0; it < 200; ++it) {
        const int64_t J = 1 + rnd() % 40, n_rows = 1 + rnd() % 300, n_cols = rnd() % 30;
        check_block("random block", n_rows, J, n_cols, 2 + (int64_t)(rnd() % 60), rnd() % 4 == 0);
    }
    if (fails) {
        fprintf(stderr, "%d checks failed\n", fails);
        return 1;
    }
    printf("checks ok\n");
    return 0;
}
