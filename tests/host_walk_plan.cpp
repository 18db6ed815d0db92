// host_walk_plan.cpp — the cost-ordered, cost-balanced form of the backward's band plan (plan_bands with an order,
// sparkfm_amd/csrc/fmhip_host.cpp) under AddressSanitizer and UBSan, in the style of host_arith_harness.cpp:
// tests/test_host_walk_plan.py compiles this file together with fmhip_host.cpp with `g++ -fsanitize=address,undefined`
// (no HIP, no GPU) and runs it over seeded random transposes.  What the device code relies on:
//   * every range appears exactly once across the eight lists, in the interval form AND in the walk form, and both
//     forms of a list hold the same ranges (a range missing from the walk form is a gradient row never written);
//   * every run of the interval form ascends (a feature-interval launch clips the runs with lower_bound);
//   * the lists' accumulated costs lie within one block's cost of each other: a list that was dealt a free block is,
//     less the most expensive block's cost, no heavier than the lightest list;
//   * the free part of the walk form is whole blocks in non-increasing cost.
//
//   host_walk_plan <seed> [cases]
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <numeric>
#include <random>
#include <vector>

#include "../sparkfm_amd/csrc/fmhip_host.h"

using namespace fmhip;
using namespace fmhip::host;

static uint64_t g_seed = 0;
static int g_case = 0;

#define CHECK(cond)                                                                                         \
    do {                                                                                                    \
        if (!(cond)) { fprintf(stderr, "FAILED %s:%d: %s  (seed %llu case %d)\n", __FILE__, __LINE__, #cond, (unsigned long long)g_seed, g_case); exit(1); } \
    } while (0)

typedef std::mt19937_64 Rng;
static int64_t uni(Rng &r, int64_t lo, int64_t hi) { return lo + (int64_t)(r() % (uint64_t)(hi - lo + 1)); }

// a random feature-sorted transpose: power-law column lengths (a few long hot columns in front when `hot`, then ever
// colder ones), every column's rows ascending and distinct
static void make_transpose(Rng &r, int64_t rows, int32_t n_cols, bool hot, HostBatch &hb, std::vector<uint32_t> &crow) {
    hb = HostBatch();
    crow.clear();
    hb.cptr.assign(1, 0);
    for (int32_t c = 0; c < n_cols; ++c) {
        const double u = (double)(r() >> 11) / 9007199254740992.0;
        int64_t len = 1 + (int64_t)((hot ? 2.0 : 0.05) * (double)rows * u * u * u / (1.0 + c));
        len = std::min(len, rows);
        const int64_t stride = std::max<int64_t>(rows / len, 1);
        int64_t row = uni(r, 0, stride - 1);
        const size_t at = crow.size();
        for (int64_t j = 0; j < len && row < rows; ++j) {
            crow.push_back((uint32_t)row | (j == 0 ? 0x80000000u : 0u));
            row += uni(r, 1, stride);
        }
        if (crow.size() == at) continue;
        hb.cfeat.push_back(c);
        hb.cptr.push_back((int32_t)crow.size());
    }
}

static void check_plan(Rng &r) {
    const int64_t rows = uni(r, 1, 80000);
    const int32_t dim = (int32_t)uni(r, 1, 6000);
    HostBatch hb;
    std::vector<uint32_t> crow;
    make_transpose(r, rows, dim, uni(r, 0, 2) != 0, hb, crow);
    const int32_t nnz = (int32_t)crow.size();
    std::vector<int32_t> cnt((size_t)dim + 1, 0), base((size_t)dim + 1, 0);
    finish_batch_meta(hb, nnz, cnt, base);
    const int32_t n_ranges = (nnz + kRangeLen - 1) / kRangeLen;
    CHECK((int32_t)hb.range_seg.size() == n_ranges);
    std::vector<int32_t> first((size_t)n_ranges), last((size_t)n_ranges);
    for (int32_t rho = 0; rho < n_ranges; ++rho) {
        first[(size_t)rho] = (int32_t)(crow[(size_t)rho * kRangeLen] & 0x7fffffffu);
        last[(size_t)rho] = (int32_t)(crow[(size_t)std::min<int32_t>((rho + 1) * kRangeLen, nnz) - 1] & 0x7fffffffu);
    }
    // the cost of a range, recounted from the stream's column flags: a close = an entry after which a new column starts
    // (or the stream ends)
    std::vector<int64_t> cost((size_t)n_ranges, 0);
    for (int32_t rho = 0; rho < n_ranges; ++rho) {
        const int32_t beg = rho * kRangeLen, end = std::min(beg + kRangeLen, nnz);
        int64_t closes = 0;
        for (int32_t p = beg; p < end; ++p) closes += (p + 1 == nnz || (crow[(size_t)p + 1] >> 31)) ? 1 : 0;
        cost[(size_t)rho] = (int64_t)(end - beg) * kCostUnit + closes * kCloseCost;
        CHECK(range_cost(hb, nnz, rho) == cost[(size_t)rho]);
    }
    std::vector<int32_t> ref_lists[kXcds];
    int32_t ref_seg[kXcds][kXSegs + 1];
    const int32_t ref_affine = plan_bands(hb, nnz, rows, first, last, ref_lists, ref_seg);      // the stream-order plan
    // the free ranges (no band run of the stream-order plan holds them) in stream order, cut into blocks of 32
    std::vector<int32_t> block_of((size_t)n_ranges, 0), block_len;
    std::vector<int64_t> block_cost;
    for (int x = 0; x < kXcds; ++x)
        for (int32_t i = 0; i < ref_seg[x][kXSegs - 1]; ++i) block_of[(size_t)ref_lists[x][(size_t)i]] = -1;
    {
        int32_t n_free_all = 0;
        for (int32_t rho = 0; rho < n_ranges; ++rho) {
            if (block_of[(size_t)rho] < 0) continue;
            const int32_t blk = n_free_all++ / 32;
            block_of[(size_t)rho] = blk;
            if ((size_t)blk == block_len.size()) { block_len.push_back(0); block_cost.push_back(0); }
            ++block_len[(size_t)blk];
            block_cost[(size_t)blk] += cost[(size_t)rho];
        }
    }
    const int64_t max_block = block_cost.empty() ? 0 : *std::max_element(block_cost.begin(), block_cost.end());
    for (int order : {(int)kWalkOrderStream, (int)kWalkOrderColdFirst}) {
        std::vector<int32_t> lists[kXcds], walk[kXcds];
        int32_t seg[kXcds][kXSegs + 1];
        const int32_t affine = plan_bands(hb, nnz, rows, first, last, lists, seg, order, &walk);
        CHECK(affine == ref_affine);
        std::vector<int> seen((size_t)n_ranges, 0), seen_w((size_t)n_ranges, 0);
        int64_t acc[kXcds];
        bool has_free[kXcds];
        for (int x = 0; x < kXcds; ++x) {
            CHECK(seg[x][0] == 0 && seg[x][kXSegs] == (int32_t)lists[x].size());
            // the band runs are those of the stream-order plan: the order only touches the free part
            for (int sg = 0; sg < kXSegs; ++sg) CHECK(seg[x][sg] == ref_seg[x][sg]);
            CHECK(std::equal(lists[x].begin(), lists[x].begin() + seg[x][kXSegs - 1], ref_lists[x].begin()));
            for (int sg = 0; sg < kXSegs; ++sg) {
                CHECK(seg[x][sg] <= seg[x][sg + 1]);
                for (int32_t i = seg[x][sg]; i < seg[x][sg + 1]; ++i) {
                    const int32_t rho = lists[x][(size_t)i];
                    CHECK(rho >= 0 && rho < n_ranges && !seen[(size_t)rho]);
                    seen[(size_t)rho] = 1;
                    if (i > seg[x][sg]) CHECK(lists[x][(size_t)i - 1] < rho);      // the interval form ascends inside every run
                }
            }
            // the walk form: the same ranges
            CHECK(walk[x].size() == lists[x].size());
            for (int32_t rho : walk[x]) {
                CHECK(rho >= 0 && rho < n_ranges && !seen_w[(size_t)rho]);
                seen_w[(size_t)rho] = 1;
            }
            std::vector<int32_t> a(lists[x]), b(walk[x]);
            std::sort(a.begin(), a.end());
            std::sort(b.begin(), b.end());
            CHECK(a == b);
            const size_t n_band = (size_t)seg[x][kXSegs - 1], n_free = lists[x].size() - n_band;
            has_free[x] = n_free > 0;
            acc[x] = 0;
            // (a band-affine range is charged its entries: it lies inside one column)
            for (int32_t rho : walk[x]) acc[x] += block_of[(size_t)rho] < 0 ? (int64_t)kRangeLen * kCostUnit : cost[(size_t)rho];
            if (order == kWalkOrderStream) {
                CHECK(walk[x] == lists[x]);
                continue;
            }
            // the free part comes first: whole blocks (32 consecutive free ranges of the stream) in non-increasing cost; the
            // band runs follow as they stand
            const size_t f0 = 0, b0 = n_free;
            CHECK(std::equal(walk[x].begin() + (std::ptrdiff_t)b0, walk[x].begin() + (std::ptrdiff_t)(b0 + n_band), lists[x].begin()));
            int64_t prev = INT64_MAX;
            for (size_t i = 0; i < n_free;) {
                const int32_t blk = block_of[(size_t)walk[x][f0 + i]];
                CHECK(blk >= 0);
                size_t j = i;
                int64_t c = 0;
                for (; j < n_free && block_of[(size_t)walk[x][f0 + j]] == blk; ++j) {
                    if (j > i) CHECK(walk[x][f0 + j - 1] < walk[x][f0 + j]);
                    c += cost[(size_t)walk[x][f0 + j]];
                }
                CHECK((int32_t)(j - i) == block_len[(size_t)blk] && c == block_cost[(size_t)blk] && c <= prev);
                prev = c;
                i = j;
            }
        }
        CHECK(std::all_of(seen.begin(), seen.end(), [](int v) { return v == 1; }));
        CHECK(std::all_of(seen_w.begin(), seen_w.end(), [](int v) { return v == 1; }));
        if (order != kWalkOrderStream) {
            // balanced by cost: when a list was dealt a block it was the lightest, so without one block's cost it is no
            // heavier than any other list at the end
            const int64_t lightest = *std::min_element(acc, acc + kXcds);
            for (int x = 0; x < kXcds; ++x)
                if (has_free[x]) CHECK(acc[x] - max_block <= lightest);
        }
    }
}

int main(int argc, char **argv) {
    g_seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    const int cases = argc > 2 ? atoi(argv[2]) : 20;
    Rng r(g_seed);
    for (g_case = 0; g_case < cases; ++g_case) check_plan(r);
    printf("host_walk_plan: seed %llu, %d cases: checks ok\n", (unsigned long long)g_seed, cases);
    return 0;
}
