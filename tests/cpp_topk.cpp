// cpp_topk.cpp — include/sparkfm.hpp's FMModel::recommend on a small problem built from an integer recipe that
// tests/test_gpu_topk.py repeats in Python.  Prints one "<candidate row> <score as %a>" line per (context, rank).
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
        DataSet ctx(make_rows(B, 0, 1)), cand(make_rows(M, 64, 2));
        std::vector<std::vector<int32_t>> ex((size_t)B);
        for (int c = 0; c < B; ++c)
            for (int d = 0; d < M; ++d)
                if ((d + c) % 5 == 0) ex[(size_t)c].push_back(d);
        std::vector<double> score;
        const std::vector<int32_t> idx = fm.recommend(ctx, cand, K, &score, &ex);
        for (size_t i = 0; i < idx.size(); ++i) printf("%d %a\n", (int)idx[i], score[i]);
        // the refusals arrive as sparkfm::Error
        bool threw = false;
        try {
            (void)fm.recommend(ctx, cand, 0);
        } catch (const Error &e) {
            threw = e.code == FMHIP_ERR_INVALID;
        }
        if (!threw) {
            fprintf(stderr, "k = 0 was not refused\n");
            return 1;
        }
    } catch (const Error &e) {
        fprintf(stderr, "error %d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}
