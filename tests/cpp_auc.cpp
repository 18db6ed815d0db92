// cpp_auc.cpp — include/sparkfm.hpp's FMModel::computeAUC / computeGroupAUC / aucDetails on a small problem built from an
// integer recipe that tests/test_gpu_auc.py repeats in Python.  Prints "<u2> <pairs> <positives> <negatives> <groups>
// <groups_scored> <auc as %a> <gauc as %a>", ungrouped and then grouped.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "sparkfm.hpp"

using namespace sparkfm;

static void print(const fmhip_auc_result &r) {
    printf("%" PRIu64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %a %a\n", r.u2, r.pairs, r.positives, r.negatives,
           r.groups, r.groups_scored, r.auc, r.gauc);
}

int main() {
    const int N = 600, n1 = 96, k = 6;
    try {
        FMModel fm(n1 - 1, k);
        fm.w0 = -0.0625;
        for (int i = 0; i < n1; ++i) {
            fm.w[(size_t)i] = ((i * 7) % 11 - 5) / 32.0;
            for (int f = 0; f < k; ++f) fm.v[(size_t)(f + i * k)] = ((f * 5 + i * 3) % 13 - 6) / 40.0;
        }
        std::vector<std::pair<double, SparseVector>> rows;
        std::vector<int32_t> groups;
        for (int r = 0; r < N; ++r) {
            SparseVector sv;
            if (r % 10 != 3)                                     // (every tenth row is empty: those predictions tie at w0)
                for (int j = 0; j < 1 + r % 3; ++j) {
                    sv.index.push_back((r * 5 + j * 17) % 32 + 32 * j);
                    sv.data.push_back((r + j) % 2 ? 1.0 : 0.5);
                }
            rows.emplace_back((r * 7) % 5 < 2 ? 1.0 : -1.0, sv);
            groups.push_back((r * 13) % 41 == 0 ? 2147483647 : (r * 13) % 41);
        }
        DataSet ds(rows, 250);
        print(fm.aucDetails(ds));
        print(fm.aucDetails(ds, &groups));
        if (fm.computeAUC(ds) != fm.aucDetails(ds).auc || fm.computeGroupAUC(ds, groups) != fm.aucDetails(ds, &groups).gauc) {
            fprintf(stderr, "computeAUC / computeGroupAUC disagree with aucDetails\n");
            return 1;
        }
        // the refusals arrive as sparkfm::Error
        bool threw = false;
        groups[17] = -1;
        try {
            (void)fm.computeGroupAUC(ds, groups);
        } catch (const Error &e) {
            threw = e.code == FMHIP_ERR_INVALID;
        }
        if (!threw) {
            fprintf(stderr, "a negative group id was not refused\n");
            return 1;
        }
    } catch (const Error &e) {
        fprintf(stderr, "error %d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}
