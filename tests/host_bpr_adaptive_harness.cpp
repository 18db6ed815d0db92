// host_bpr_adaptive_harness.cpp — the adaptive sampler's host twin (fmhip_host.cpp: bpr_candidate) as a stand-alone program, built
// with g++ -fsanitize=address,undefined by tests/test_host_bpr_adaptive.py.
//   host_bpr_adaptive_harness <vectors file>
// The file holds what the Python twin (tests/bpr_adaptive_ref.py) recorded, one record per line:
//   L <seed> <t> <M> <len> <the context's positives, ascending ...>       a context: every V line up to the next L draws for it
//   V <p> <c> <row> <attempts> <forced>                                   candidate c of pair p
// Every V line is recomputed with bpr_candidate — the list in an array of exactly its length, so a read past its end is a sanitizer
// error — and must agree bit for bit; candidate 0 must be bpr_negative's draw; a row is never a positive.  Prints "checks ok <n>".
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "../sparkfm_amd/csrc/fmhip_host.h"

using namespace fmhip::host;

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            fprintf(stderr, "%s:%d: check failed: %s (record %ld)\n", __FILE__, __LINE__, #cond, n_read); \
            return 1;                                                                \
        }                                                                            \
    } while (0)

int main(int argc, char **argv) {
    long n_read = 0, n_checked = 0;
    if (argc != 2) {
        fprintf(stderr, "usage: %s vectors\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "r");
    CHECK(f != nullptr);
    uint64_t seed = 0;
    uint32_t t = 0;
    int32_t M = 0, len = -1;
    std::unique_ptr<int32_t[]> list;
    char tag = 0;
    while (fscanf(f, " %c", &tag) == 1) {
        ++n_read;
        if (tag == 'L') {
            CHECK(fscanf(f, "%" SCNu64 " %" SCNu32 " %" SCNd32 " %" SCNd32, &seed, &t, &M, &len) == 4);
            CHECK(M >= 2 && len >= 0 && len < M);
            list.reset(new int32_t[(size_t)len]);
            for (int32_t j = 0; j < len; ++j) {
                CHECK(fscanf(f, "%" SCNd32, &list[(size_t)j]) == 1);
                CHECK(list[(size_t)j] >= 0 && list[(size_t)j] < M && (j == 0 || list[(size_t)j] > list[(size_t)j - 1]));
            }
        } else {
            CHECK(tag == 'V' && len >= 0);
            uint32_t p = 0, c = 0;
            int32_t row = 0;
            int attempts = 0, forced = 0;
            CHECK(fscanf(f, "%" SCNu32 " %" SCNu32 " %" SCNd32 " %d %d", &p, &c, &row, &attempts, &forced) == 5);
            CHECK(c < 64);
            int a = -1, fo = -1;
            const int32_t got = bpr_candidate(seed, p, c, t, M, list.get(), len, &a, &fo);
            CHECK(got == row && a == attempts && fo == forced);
            CHECK(got >= 0 && got < M);
            for (int32_t j = 0; j < len; ++j) CHECK(list[(size_t)j] != got);
            CHECK(bpr_candidate(seed, p, c, t, M, list.get(), len, nullptr) == row);        // attempts / forced are nullable
            if (c == 0) {
                int a0 = -1, f0 = -1;
                CHECK(bpr_negative(seed, p, t, M, list.get(), len, &a0, &f0) == row && a0 == attempts && f0 == forced);
            }
            ++n_checked;
        }
    }
    fclose(f);
    CHECK(n_checked > 0);
    printf("checks ok %ld\n", n_checked);
    return 0;
}
