// host_bpr_harness.cpp — the BPR trainer's host arithmetic (fmhip_host.cpp: bpr_positive_lists, bpr_negative) as a stand-alone
// program, built with g++ -fsanitize=address,undefined by tests/test_host_bpr.py.
//   host_bpr_harness <seed> <n_ctx> <M> <n_inter> <n_pairs> <t>
// A seeded problem: n_inter interactions (context, row) drawn with repeats, the last context given M - 1 positives (every row but
// row M / 2: the forced path) — then the lists are checked against a brute-force build (exactly sized arrays, so a read past a
// list's end is a sanitizer error), and n_pairs draws at epoch t are checked (never a positive, inside [0, M)) and printed:
//   P <ptr entries ...>
//   R <rows ...>
//   D <p> <context> <row> <attempts> <forced>
// The test compares the printed lists and draws with the Python twin bit for bit.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <set>
#include <vector>

#include "../sparkfm_amd/csrc/fmhip_host.h"

using namespace fmhip::host;

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
    // exactly sized heap arrays
    std::unique_ptr<int32_t[]> ictx(new int32_t[(size_t)n_inter]), icand(new int32_t[(size_t)n_inter]);
    std::vector<std::set<int32_t>> brute((size_t)n_ctx);
    for (int64_t i = 0; i < n_rand; ++i) {
        ictx[i] = (int32_t)(lcg(s) % (uint64_t)(n_ctx - 1));        // (the last context's list is made below)
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
    CHECK((int64_t)ptr.size() == n_ctx + 1 && ptr[0] == 0 && ptr.back() == (int64_t)rows.size());
    for (int64_t u = 0; u < n_ctx; ++u) {
        const std::vector<int32_t> want(brute[(size_t)u].begin(), brute[(size_t)u].end());
        CHECK(ptr[(size_t)u + 1] - ptr[(size_t)u] == (int64_t)want.size());
        for (size_t j = 0; j < want.size(); ++j) CHECK(rows[(size_t)ptr[(size_t)u] + j] == want[j]);
    }
    printf("P");
    for (int64_t v : ptr) printf(" %lld", (long long)v);
    printf("\nR");
    for (int32_t v : rows) printf(" %d", (int)v);
    printf("\n");
    for (int64_t p = 0; p < n_pairs; ++p) {
        // every fourth pair draws for the last context (one row left: mostly forced), the others for a random one
        const int64_t u = p % 4 == 3 ? n_ctx - 1 : (int64_t)(lcg(s) % (uint64_t)n_ctx);
        const int32_t len = (int32_t)(ptr[(size_t)u + 1] - ptr[(size_t)u]);
        // the list in an array of exactly its length
        std::unique_ptr<int32_t[]> list(new int32_t[(size_t)len]);
        for (int32_t j = 0; j < len; ++j) list[j] = rows[(size_t)ptr[(size_t)u] + (size_t)j];
        int attempts = -1, forced = -1;
        const int32_t c = bpr_negative(seed, (uint32_t)p, t, (int32_t)M, list.get(), len, &attempts, &forced);
        CHECK(c >= 0 && c < M && !brute[(size_t)u].count(c));
        CHECK(attempts >= 1 && attempts <= 64 && (forced == 0 || (forced == 1 && attempts == 64)));
        CHECK(bpr_negative(seed, (uint32_t)p, t, (int32_t)M, list.get(), len, nullptr) == c);
        if (u == n_ctx - 1) CHECK(c == M / 2);
        printf("D %lld %lld %d %d %d\n", (long long)p, (long long)u, (int)c, attempts, forced);
    }
    printf("checks ok\n");
    return 0;
}
