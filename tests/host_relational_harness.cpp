// host_relational_harness.cpp — the relational dataset's host arithmetic (relational_bad_mapping, first_shared_feature,
// RelationInverse::append_batch; sparkfm_amd/csrc/fmhip_host.cpp) as a stand-alone program under AddressSanitizer and UBSan:
// seeded mappings — uniform, skewed, one list holding every row, block rows nobody references, a block of one row — cut into
// batches; every batch's inverse map is checked against a brute-force one, its work list against the cut, and every index the
// device would read against the bounds of the array it indexes.
//   host_relational_harness <seed> <cases>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
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

static void check_inverse(const std::vector<int32_t> &map, int64_t J, int64_t batch_rows, int32_t cut, int c) {
    const int64_t n = (int64_t)map.size();
    RelationInverse inv;
    std::vector<int32_t> count;
    size_t nb = 0;
    for (int64_t r0 = 0; r0 < n; r0 += batch_rows, ++nb) inv.append_batch(map.data() + r0, std::min(batch_rows, n - r0), J, cut, count);
    CHECK(inv.batches.size() == nb, "case %d: %zu batches", c, inv.batches.size());
    CHECK((int64_t)inv.trow.size() == n, "case %d: trow holds %zu rows of %lld", c, inv.trow.size(), (long long)n);
    for (int32_t x : count) CHECK(x == 0, "case %d: the scratch is not left zeroed", c);
    int64_t touched_all = 0;
    for (size_t b = 0; b < nb; ++b) {
        const RelationInverse::Batch &B = inv.batches[b];
        const int64_t r0 = (int64_t)b * batch_rows, rows = std::min(batch_rows, n - r0);
        CHECK(B.row_off == r0, "case %d batch %zu: row_off", c, b);
        // brute force: the lists
        std::vector<std::vector<int32_t>> lists((size_t)J);
        for (int64_t r = 0; r < rows; ++r) lists[(size_t)map[(size_t)(r0 + r)]].push_back((int32_t)r);
        int32_t touched = 0, work = 0, longs = 0, parts = 0;
        for (int64_t j = 0; j < J; ++j) {
            if (lists[(size_t)j].empty()) continue;
            const int32_t t = touched++;
            CHECK(t < B.n_touched && inv.tj[(size_t)(B.t_off + t)] == (int32_t)j, "case %d batch %zu: touched row %d is not block row %lld", c, b, t, (long long)j);
            if (t >= B.n_touched) continue;
            const int32_t beg = inv.tptr[(size_t)(B.tptr_off + t)], end = inv.tptr[(size_t)(B.tptr_off + t + 1)];
            CHECK(end - beg == (int32_t)lists[(size_t)j].size() && beg >= 0 && end <= rows, "case %d batch %zu: list of block row %lld is [%d, %d)", c, b,
                  (long long)j, beg, end);
            for (int32_t i = beg; i < end && i - beg < (int32_t)lists[(size_t)j].size(); ++i)
                CHECK(inv.trow[(size_t)(B.row_off + i)] == lists[(size_t)j][(size_t)(i - beg)], "case %d batch %zu: list of block row %lld is not ascending", c, b,
                      (long long)j);
            // the work items of this list, in order
            const int32_t len = end - beg;
            if (len <= cut) {
                CHECK(work < B.n_work && inv.wt[(size_t)(B.w_off + work)] == t && inv.wbeg[(size_t)(B.w_off + work)] == beg &&
                          inv.wdst[(size_t)(B.w_off + work)] == (int32_t)j, "case %d batch %zu: the item of the short list %lld", c, b, (long long)j);
                ++work;
            } else {
                CHECK(longs < B.n_long && inv.lt[(size_t)(B.l_off + longs)] == t && inv.lfirst[(size_t)(B.l_off + longs)] == parts &&
                          inv.lcount[(size_t)(B.l_off + longs)] == (len + cut - 1) / cut, "case %d batch %zu: the second-pass entry of the long list %lld", c, b,
                      (long long)j);
                ++longs;
                for (int32_t o = 0; o < len; o += cut, ++work, ++parts)
                    CHECK(work < B.n_work && inv.wt[(size_t)(B.w_off + work)] == t && inv.wbeg[(size_t)(B.w_off + work)] == beg + o &&
                              inv.wdst[(size_t)(B.w_off + work)] == -1 - parts, "case %d batch %zu: chunk %d of the long list %lld", c, b, o / cut, (long long)j);
            }
        }
        CHECK(touched == B.n_touched && work == B.n_work && longs == B.n_long && parts == B.n_part, "case %d batch %zu: %d touched, %d items, %d long, %d partial rows", c, b,
              B.n_touched, B.n_work, B.n_long, B.n_part);
        CHECK(B.n_part <= inv.max_part, "case %d batch %zu: max_part", c, b);
        touched_all += touched;
    }
    // nothing is sized by batches x block rows
    CHECK((int64_t)inv.tj.size() == touched_all && (int64_t)inv.tptr.size() == touched_all + (int64_t)nb, "case %d: tj / tptr sizes", c);
    CHECK((int64_t)inv.wt.size() <= touched_all + n / cut + (int64_t)nb, "case %d: %zu work items", c, inv.wt.size());
}

int main(int argc, char **argv) {
    const unsigned seed = argc > 1 ? (unsigned)strtoul(argv[1], nullptr, 10) : 1u;
    const int cases = argc > 2 ? atoi(argv[2]) : 100;
    std::mt19937_64 gen(seed);
    // the mapping check
    {
        const int32_t ok[5] = {0, 3, 1, 3, 2}, neg[5] = {0, 3, -1, 9, 2}, high[5] = {0, 3, 1, 3, 4};
        CHECK(relational_bad_mapping(5, ok, 4) == -1, "a good mapping");
        CHECK(relational_bad_mapping(5, neg, 4) == 2, "the first bad entry is named");
        CHECK(relational_bad_mapping(5, high, 4) == 4, "an entry equal to the block's row count");
        CHECK(relational_bad_mapping(0, nullptr, 4) == -1, "no rows");
    }
    // disjoint feature sets
    {
        const int32_t a[] = {1, 5, 5, 9}, b[] = {7, 3, -1}, c3[] = {9, 3, 12, 40};
        const int32_t *f[3] = {a, b, c3};
        const int64_t n2[3] = {4, 3, 0}, n3[3] = {4, 3, 4};
        SharedFeature s = first_shared_feature(3, f, n2, 12);
        CHECK(s.feature == -1, "disjoint parts (a repeat inside a part, an id of -1)");
        s = first_shared_feature(3, f, n3, 12);       // 3 is shared by parts 1 and 2, 9 by 0 and 2; 40 lies beyond the dimension
        CHECK(s.feature == 3 && s.a == 1 && s.b == 2, "the lowest shared feature: got %d (%d, %d)", s.feature, s.a, s.b);
        s = first_shared_feature(0, nullptr, nullptr, 0);
        CHECK(s.feature == -1, "no parts");
    }
    // the degenerate shapes first: one block row, one list holding every row, lengths around the cut
    check_inverse(std::vector<int32_t>(1, 0), 1, 1, 4, -1);
    check_inverse(std::vector<int32_t>(37, 0), 1, 10, 4, -2);
    check_inverse(std::vector<int32_t>(600, 2), 5, 600, 256, -3);
    for (int32_t len : {255, 256, 257, 512, 513}) {
        std::vector<int32_t> m((size_t)len, 1);
        m.push_back(0);
        check_inverse(m, 3, len + 1, 256, -4);
    }
    for (int c = 0; c < cases; ++c) {
        const int64_t J = 1 + (int64_t)(gen() % (c % 5 == 0 ? 3 : 200));
        const int64_t n = 1 + (int64_t)(gen() % 3000);
        const int64_t batch_rows = 1 + (int64_t)(gen() % (uint64_t)n);
        const int32_t cut = (int32_t)(1 + gen() % (c % 3 == 0 ? 8 : 300));
        std::vector<int32_t> map((size_t)n);     // exactly n entries: a read past the end is the sanitizer's to find
        const int kind = (int)(gen() % 3);
        for (auto &x : map) {
            const uint64_t u = gen();
            x = kind == 0 ? (int32_t)(u % (uint64_t)J)                               // uniform
              : kind == 1 ? (int32_t)((u % (uint64_t)J) * (gen() % (uint64_t)J) / (uint64_t)J)      // skewed to the low rows
                          : (int32_t)((u & 3) ? 0 : u % (uint64_t)((J + 1) / 2));    // one popular row; the upper half referenced by nobody
        }
        check_inverse(map, J, batch_rows, cut, c);
    }
    if (fails) {
        fprintf(stderr, "%d checks failed\n", fails);
        return 1;
    }
    printf("checks ok (%d cases)\n", cases);
    return 0;
}
