// host_bpr_proposal_harness.cpp — the weighted proposal's host arithmetic (fmhip_host.cpp: bpr_alias_table, bpr_proposal_candidate;
// include/fmhip_proposal.h) as a stand-alone program, built with g++ -fsanitize=address,undefined by tests/test_host_bpr_proposal.py.
//   host_bpr_proposal_harness <seed> <n_ctx> <M> <n_inter> <n_pairs> <t>
// host_bpr_harness.cpp's seeded problem: n_inter interactions drawn with repeats, the last context given M - 1 positives (every
// row but row M / 2: the forced path).  The weights are small integers from the same generator, one row in eight 1000 times
// heavier.  The table is built into an array of exactly M entries (a write past it is a sanitizer error) and checked — every
// alias in [0, M), the buckets' masses adding up to every row's share — the refusals are checked to leave the table alone, and
// n_pairs draws at epoch t, candidate p % 5 of pair p, are checked (never a positive, inside [0, M)) and printed:
//   P <ptr entries ...>
//   R <rows ...>
//   W <weights ...>
//   T <row> <thresh> <alias>
//   D <p> <context> <candidate> <row> <attempts> <forced>
// The test compares the printed table and draws with the Python twin bit for bit.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <memory>
#include <set>
#include <vector>

#include "../sparkfm_amd/csrc/fmhip_host.h"

using namespace fmhip::host;
using fmhip::rng::AliasEntry;

static uint64_t lcg(uint64_t &s) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return s >> 33;
}

#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                     \
        }                                                                 \
    } while (0)

int main(int argc, char **argv) {
    if (argc != 7) {
        fprintf(stderr, "usage: %s seed n_ctx M n_inter n_pairs t\n", argv[0]);
        return 2;
    }
    const uint64_t seed = strtoull(argv[1], nullptr, 10);
    const int64_t n_ctx = atoll(argv[2]), M = atoll(argv[3]), n_rand = atoll(argv[4]), n_pairs = atoll(argv[5]);
    const uint32_t t = (uint32_t)strtoul(argv[6], nullptr, 10);
    CHECK(n_ctx >= 2 && M >= 2 && n_rand >= 0 && n_pairs >= 1);
    uint64_t s = seed * 2 + 1;
    const int64_t n_inter = n_rand + (M - 1);
    std::unique_ptr<int32_t[]> ictx(new int32_t[(size_t)n_inter]), icand(new int32_t[(size_t)n_inter]);
    std::vector<std::set<int32_t>> brute((size_t)n_ctx);
    for (int64_t i = 0; i < n_rand; ++i) {
        ictx[i] = (int32_t)(lcg(s) % (uint64_t)(n_ctx - 1));
        icand[i] = (int32_t)(lcg(s) % (uint64_t)M);
        if ((int64_t)brute[(size_t)ictx[i]].size() == M - 1 && !brute[(size_t)ictx[i]].count(icand[i])) icand[i] = *brute[(size_t)ictx[i]].begin();
        brute[(size_t)ictx[i]].insert(icand[i]);
    }
    for (int64_t j = 0, i = n_rand; j < M; ++j) {
        if (j == M / 2) continue;
        ictx[i] = (int32_t)(n_ctx - 1);
        icand[i] = (int32_t)j;
        brute[(size_t)n_ctx - 1].insert((int32_t)j);
        ++i;
    }
    std::vector<int64_t> ptr;
    std::vector<int32_t> rows;
    bpr_positive_lists(n_ctx, n_inter, ictx.get(), icand.get(), ptr, rows);
    printf("P");
    for (int64_t v : ptr) printf(" %lld", (long long)v);
    printf("\nR");
    for (int32_t v : rows) printf(" %d", (int)v);
    printf("\n");

    // ---- the table, in arrays of exactly M entries
    std::unique_ptr<double[]> w(new double[(size_t)M]);
    for (int64_t i = 0; i < M; ++i) w[i] = (double)(1 + lcg(s) % 50) * (lcg(s) % 8 == 0 ? 1000.0 : 1.0);
    std::unique_ptr<AliasEntry[]> tab(new AliasEntry[(size_t)M]);
    CHECK(bpr_alias_table(M, w.get(), tab.get()) == -1);
    printf("W");
    for (int64_t i = 0; i < M; ++i) printf(" %.17g", w[i]);
    printf("\n");
    double sum = 0.0;
    for (int64_t i = 0; i < M; ++i) sum += w[i];
    std::vector<double> mass((size_t)M, 0.0);      // in units of 2^-32 of a bucket: exact in a double
    for (int64_t j = 0; j < M; ++j) {
        CHECK(tab[j].alias >= 0 && tab[j].alias < M);
        if (tab[j].alias == j) {
            mass[(size_t)j] += 4294967296.0;
        } else {
            mass[(size_t)j] += (double)tab[j].thresh;
            mass[(size_t)tab[j].alias] += 4294967296.0 - (double)tab[j].thresh;
        }
        printf("T %lld %u %d\n", (long long)j, (unsigned)tab[j].thresh, (int)tab[j].alias);
    }
    for (int64_t i = 0; i < M; ++i) CHECK(fabs(mass[(size_t)i] / (4294967296.0 * (double)M) - w[i] / sum) <= 0x1p-30);

    // ---- the refusals: the first bad row named, the table not written
    {
        const double bads[] = {0.0, -1.0, std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity(), -0.0};
        std::unique_ptr<AliasEntry[]> keep(new AliasEntry[(size_t)M]);
        for (int64_t j = 0; j < M; ++j) keep[j] = tab[j];
        for (double bad : bads) {
            const int64_t at = (int64_t)(lcg(s) % (uint64_t)M);
            std::unique_ptr<double[]> wb(new double[(size_t)M]);
            for (int64_t i = 0; i < M; ++i) wb[i] = w[i];
            wb[at] = bad;
            wb[M - 1] = at == M - 1 ? bad : -2.0;       // (a second bad row behind it: the first is named)
            CHECK(bpr_alias_table(M, wb.get(), tab.get()) == at);
            for (int64_t j = 0; j < M; ++j) CHECK(tab[j].thresh == keep[j].thresh && tab[j].alias == keep[j].alias);
        }
        std::unique_ptr<double[]> huge(new double[(size_t)M]);
        for (int64_t i = 0; i < M; ++i) huge[i] = std::numeric_limits<double>::max();
        CHECK(bpr_alias_table(M, huge.get(), tab.get()) == -2);
        for (int64_t j = 0; j < M; ++j) CHECK(tab[j].thresh == keep[j].thresh && tab[j].alias == keep[j].alias);
    }

    // ---- the draws
    for (int64_t p = 0; p < n_pairs; ++p) {
        // every fourth pair draws for the last context (one row left: mostly forced), the others for a random one
        const int64_t u = p % 4 == 3 ? n_ctx - 1 : (int64_t)(lcg(s) % (uint64_t)n_ctx);
        const uint32_t c = (uint32_t)(p % 5 == 4 ? 63 : p % 5);
        const int32_t len = (int32_t)(ptr[(size_t)u + 1] - ptr[(size_t)u]);
        std::unique_ptr<int32_t[]> list(new int32_t[(size_t)len]);      // the list in an array of exactly its length
        for (int32_t j = 0; j < len; ++j) list[j] = rows[(size_t)ptr[(size_t)u] + (size_t)j];
        int attempts = -1, forced = -1;
        const int32_t row = bpr_proposal_candidate(seed, (uint32_t)p, c, t, (int32_t)M, tab.get(), list.get(), len, &attempts, &forced);
        CHECK(row >= 0 && row < M && !brute[(size_t)u].count(row));
        CHECK(attempts >= 1 && attempts <= 32 && (forced == 0 || (forced == 1 && attempts == 32)));
        CHECK(bpr_proposal_candidate(seed, (uint32_t)p, c, t, (int32_t)M, tab.get(), list.get(), len, nullptr) == row);
        if (u == n_ctx - 1) CHECK(row == M / 2);
        printf("D %lld %lld %u %d %d %d\n", (long long)p, (long long)u, (unsigned)c, (int)row, attempts, forced);
    }
    printf("checks ok\n");
    return 0;
}
