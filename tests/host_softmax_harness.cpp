// host_softmax_harness.cpp — the sampled softmax's host arithmetic (fmhip_host.cpp: bpr_log_proposal) as a stand-alone program,
// built with g++ -fsanitize=address,undefined by tests/test_host_softmax.py.
//   host_softmax_harness <vectors file>
// The file holds what the Python side recorded, one record per line, numbers as the hex of their bits:
//   L <M> <w_0> ... <w_{M-1}> <lq_0> ... <lq_{M-1}>       M fp64 weights and the M fp32 entries of their log-Q table
// Every record is recomputed into arrays of exactly its length — a read or write past their end is a sanitizer error — and must
// agree bit for bit; the weights must pass bpr_alias_table's check first, as in fmhip_proposal_set.  Prints "checks ok <n>".
#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
    char tag = 0;
    while (fscanf(f, " %c", &tag) == 1) {
        ++n_read;
        CHECK(tag == 'L');
        int64_t M = 0;
        CHECK(fscanf(f, "%" SCNd64, &M) == 1 && M >= 1 && M <= (1 << 20));
        std::unique_ptr<double[]> w(new double[(size_t)M]);
        for (int64_t i = 0; i < M; ++i) {
            uint64_t bits = 0;
            CHECK(fscanf(f, "%" SCNx64, &bits) == 1);
            memcpy(&w[(size_t)i], &bits, sizeof bits);
        }
        std::unique_ptr<fmhip::rng::AliasEntry[]> tab(new fmhip::rng::AliasEntry[(size_t)M]);
        CHECK(bpr_alias_table(M, w.get(), tab.get()) == -1);
        std::unique_ptr<float[]> got(new float[(size_t)M]);
        bpr_log_proposal(M, w.get(), got.get());
        for (int64_t i = 0; i < M; ++i) {
            uint32_t want = 0, have = 0;
            CHECK(fscanf(f, "%" SCNx32, &want) == 1);
            memcpy(&have, &got[(size_t)i], sizeof have);
            CHECK(have == want);
            CHECK(std::isfinite(got[(size_t)i]) && got[(size_t)i] <= 0.f);
        }
        ++n_checked;
    }
    fclose(f);
    CHECK(n_checked > 0);
    printf("checks ok %ld\n", n_checked);
    return 0;
}
