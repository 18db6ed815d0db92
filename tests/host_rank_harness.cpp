// host_rank_harness.cpp — the ranking metrics' host arithmetic (rank_metrics, sparkfm_amd/csrc/fmhip_host.cpp) under
// AddressSanitizer and UBSan, in the style of host_arith_harness.cpp: tests/test_host_ranking.py compiles this file together
// with fmhip_host.cpp with `g++ -fsanitize=address,undefined` (no HIP, no GPU), writes its cases to a file and compares what
// this program prints with the numpy restatement (tests/rank_ref.py).  The arrays are sized exactly, so a read past a context's
// ranks is the sanitizer's to report.
//
//   host_rank_harness <cases file>
// a case: "k n_contexts", then n_contexts + 1 offsets starting at 0, then offsets[n_contexts] ranks.
// Per case one line: the status (-1, or the context refused), contexts, skipped, relevant and the six metrics as %a.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../sparkfm_amd/csrc/fmhip_host.h"

using namespace fmhip::host;

int main(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: host_rank_harness <cases file>\n");
        return 2;
    }
    FILE *f = fopen(argv[1], "r");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    long long k = 0, n = 0;
    int cases = 0;
    while (fscanf(f, "%lld %lld", &k, &n) == 2) {
        std::vector<int64_t> ptr((size_t)n + 1);
        for (auto &p : ptr) {
            long long v = 0;
            if (fscanf(f, "%lld", &v) != 1) return 2;
            p = v;
        }
        if (ptr[0] != 0) return 2;
        std::vector<int32_t> rank((size_t)ptr[(size_t)n]);
        for (auto &r : rank) {
            long long v = 0;
            if (fscanf(f, "%lld", &v) != 1) return 2;
            r = (int32_t)v;
        }
        RankMetricSums s;
        const int64_t rc = rank_metrics(n, ptr.data(), rank.data(), (int32_t)k, &s);
        printf("%lld %lld %lld %lld %a %a %a %a %a %a\n", (long long)rc, (long long)s.contexts, (long long)s.skipped, (long long)s.relevant,
               s.hit_rate, s.recall, s.precision, s.ndcg, s.mrr, s.map);
        ++cases;
    }
    fclose(f);
    fprintf(stderr, "host_rank_harness: %d cases\n", cases);
    return 0;
}
