// cpp_ranking.cpp — include/sparkfm.hpp's FMModel::rankOf and computeRankingMetrics on a small problem built from an integer
// recipe that tests/test_gpu_ranking.py repeats in Python (the rows of tests/cpp_topk.cpp).  Prints one "<rank> <score as %a>"
// line per (context, relevant row), then one line of the metrics at k = 9: contexts, skipped, relevant and the six ratios as %a.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "sparkfm.hpp"

using namespace sparkfm;

static std::vector<std::pair<double, SparseVector>> make_rows(int n, int lo, int salt) {
    std::vector<std::pair<double, SparseVector>> rows;
    for (int r = 0; r < n; ++r) {
        SparseVector sv;
        if (r % 10 != 3)
            for (int j = 0; j < 1 + r % 3; ++j) {
                sv.index.push_back(lo + (r * 5 + j * 17 + salt) % 16 + 16 * j);
                sv.data.push_back((r + j) % 2 ? 1.0 : 0.5);
            }
        rows.emplace_back(0.0, sv);
    }
    return rows;
}

int main() {
    const int B = 50, M = 777, K = 9, n1 = 128, k = 12;
    try {
        FMModel fm(n1 - 1, k);
        fm.w0 = 0.125;
        for (int i = 0; i < n1; ++i) {
            fm.w[(size_t)i] = ((i * 7) % 11 - 5) / 32.0;
            for (int f = 0; f < k; ++f) fm.v[(size_t)(f + i * k)] = ((f * 5 + i * 3) % 13 - 6) / 40.0;
        }
        DataSet ctx(make_rows(B, 0, 1), 16), cand(make_rows(M, 64, 2));
        // context c holds out the rows 7c mod M and 7c + 300 mod M (every sixth context: none); every fifth of the other rows is excluded
        std::vector<std::vector<int32_t>> rel((size_t)B), ex((size_t)B);
        for (int c = 0; c < B; ++c) {
            if (c % 6 != 0) rel[(size_t)c] = {(c * 7) % M, (c * 7 + 300) % M};
            std::sort(rel[(size_t)c].begin(), rel[(size_t)c].end());
            for (int d = 0; d < M; ++d)
                if ((d + c) % 5 == 0 && !std::binary_search(rel[(size_t)c].begin(), rel[(size_t)c].end(), d)) ex[(size_t)c].push_back(d);
        }
        std::vector<std::vector<double>> score;
        const std::vector<std::vector<int32_t>> ranks = fm.rankOf(ctx, cand, rel, &ex, &score);
        for (size_t c = 0; c < ranks.size(); ++c)
            for (size_t j = 0; j < ranks[c].size(); ++j) printf("%d %a\n", (int)ranks[c][j], score[c][j]);
        const fmhip_rank_metrics_t r = fm.computeRankingMetrics(ctx, cand, rel, K, &ex);
        printf("%lld %lld %lld %a %a %a %a %a %a\n", (long long)r.contexts, (long long)r.skipped, (long long)r.relevant, r.hit_rate, r.recall,
               r.precision, r.ndcg, r.mrr, r.map);
        // the refusals arrive as sparkfm::Error
        bool threw = false;
        try {
            ex[1].push_back(rel[1][0]);      // relevant and excluded
            std::sort(ex[1].begin(), ex[1].end());
            (void)fm.rankOf(ctx, cand, rel, &ex);
        } catch (const Error &e) {
            threw = e.code == FMHIP_ERR_INVALID;
        }
        if (!threw) {
            fprintf(stderr, "a relevant and excluded row was not refused\n");
            return 1;
        }
    } catch (const Error &e) {
        fprintf(stderr, "error %d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}
