// host_arith_harness.cpp — the library's pure host arithmetic (sparkfm_amd/csrc/fmhip_host.cpp) under AddressSanitizer and
// UBSan: tests/test_host_cpu.py compiles this file together with fmhip_host.cpp with `g++ -fsanitize=address,undefined` (no
// HIP, no GPU) and runs it over seeded random shapes.  Every function is checked against its own contract — what the device
// code and the other host code RELY on (a band plan whose runs are not ascending makes step_backward's lower_bound clip the
// wrong ranges; a level schedule that puts two columns sharing a row side by side races in k_als_level) — while the sanitizers
// watch the index arithmetic.  VERDICT r4 next #6; the sanitizers cannot run on the GPU pool.
//
// Covered: shard_bounds; feature_counts / rank_from_counts / relabel_columns; finish_batch_meta, plan_bands, als_levels; choose_cuts,
// interval_edges, shard_share, compact_edges, apply_groups; bw_window_step (`host_arith_harness window`: exhaustive); and the host passes of the dataset build — validate_rows,
// choose_hot_block, split_hot_rows, forward_row_order, sort_rows_by_feature (each for float and double values, with 1 and with
// 4 threads, which must agree) and own_bitmaps.
//
//   host_arith_harness <seed> [cases]
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <numeric>
#include <random>
#include <vector>

#include "../sparkfm_amd/csrc/fmhip_host.h"

using namespace fmhip;
using namespace fmhip::host;

#define CHECK(cond)                                                                                         \
    do {                                                                                                    \
        if (!(cond)) { fprintf(stderr, "FAILED %s:%d: %s  (seed %llu case %d)\n", __FILE__, __LINE__, #cond, (unsigned long long)g_seed, g_case); exit(1); } \
    } while (0)

static uint64_t g_seed = 0;
static int g_case = 0;
typedef std::mt19937_64 Rng;

static int64_t uni(Rng &r, int64_t lo, int64_t hi) { return lo + (int64_t)(r() % (uint64_t)(hi - lo + 1)); }

// ---- fmhip_shard_rows ------------------------------------------------------------------------------------------
static void check_shards(Rng &r) {
    const int64_t n_rows = uni(r, 0, 3000);
    std::vector<int64_t> rp((size_t)n_rows + 1, 0);
    const int kind = (int)uni(r, 0, 3);
    for (int64_t i = 0; i < n_rows; ++i) {
        int64_t len = kind == 0 ? 0 : uni(r, 0, 20);
        if (kind == 2 && uni(r, 0, 99) == 0) len = uni(r, 1000, 100000);          // giant rows
        if (kind == 3 && i == n_rows / 2) len = (int64_t)1 << 40;                  // one row that dwarfs everything (64-bit products)
        rp[(size_t)i + 1] = rp[(size_t)i] + len;
    }
    for (int world = 1; world <= 9; ++world) {
        int64_t covered = 0;
        for (int rank = 0; rank < world; ++rank) {
            int64_t lo = -1, hi = -1;
            shard_bounds(n_rows, rp.data(), world, rank, &lo, &hi);
            CHECK(lo == covered && hi >= lo && hi <= n_rows);
            covered = hi;
            if (rank + 1 < world && rp[(size_t)n_rows] > 0) {
                // the boundary is a row offset nearest to (rank + 1) / world of the nonzeros
                const int64_t target = (int64_t)((__int128)rp[(size_t)n_rows] * (rank + 1) / world);
                const int64_t d = llabs(rp[(size_t)hi] - target);
                if (hi > lo) {      // (a boundary clamped to the previous one need not be nearest)
                    if (hi > 0) CHECK(d <= llabs(rp[(size_t)hi - 1] - target) || hi - 1 < lo);
                    if (hi < n_rows) CHECK(d <= llabs(rp[(size_t)hi + 1] - target));
                }
            }
        }
        CHECK(covered == n_rows);
    }
}

// ---- feature relabelling ---------------------------------------------------------------------------------------
static void check_relabel(Rng &r, bool big) {
    const int64_t n1 = big ? ((int64_t)1 << 23) + uni(r, 1, 1000) : uni(r, 1, 5000);
    const int64_t nnz = big ? 400000 : uni(r, 0, 300000);
    std::vector<int32_t> col((size_t)nnz);
    for (auto &c : col) {
        const double u = (double)(r() >> 11) / 9007199254740992.0;
        c = (int32_t)std::min<int64_t>((int64_t)((double)n1 * u * u * u), n1 - 1);          // skewed towards small ids
    }
    std::vector<int64_t> counts((size_t)n1, 0), ref((size_t)n1, 0);
    for (int32_t c : col) ++ref[(size_t)c];
    // two partitions accumulate
    const int64_t half = nnz / 2;
    CHECK(feature_counts(half, col.data(), n1, counts.data()) == -1);
    CHECK(feature_counts(nnz - half, col.data() + half, n1, counts.data()) == -1);
    CHECK(counts == ref);
    std::vector<int32_t> rank((size_t)n1), by_rank((size_t)n1), out((size_t)nnz);
    rank_from_counts(n1, counts.data(), rank.data(), by_rank.data());
    for (int64_t i = 0; i < n1; ++i) {
        CHECK(rank[(size_t)by_rank[(size_t)i]] == (int32_t)i);
        if (i > 0) {
            const int32_t a = by_rank[(size_t)i - 1], b = by_rank[(size_t)i];
            CHECK(counts[(size_t)a] > counts[(size_t)b] || (counts[(size_t)a] == counts[(size_t)b] && a < b));
        }
    }
    CHECK(relabel_columns(nnz, col.data(), n1, rank.data(), out.data()) == -1);
    for (int64_t i = 0; i < nnz; ++i) CHECK(by_rank[(size_t)out[(size_t)i]] == col[(size_t)i]);
    if (nnz > 0) {
        // an id outside [0, n1): found and named, nothing written past the arrays
        const int64_t at = uni(r, 0, nnz - 1);
        const int32_t keep = col[(size_t)at];
        col[(size_t)at] = uni(r, 0, 1) ? (int32_t)n1 : -1;
        std::vector<int64_t> c2((size_t)n1, 0);
        const int64_t bad = feature_counts(nnz, col.data(), n1, c2.data());
        CHECK(bad >= 0 && (col[(size_t)bad] < 0 || col[(size_t)bad] >= n1));
        CHECK(relabel_columns(nnz, col.data(), n1, rank.data(), out.data()) >= 0);
        col[(size_t)at] = keep;
    }
}

// ---- a batch's metadata, the band plan, the ALS levels ---------------------------------------------------------------
struct Transpose {
    HostBatch hb;
    std::vector<uint32_t> crow;
    int64_t rows = 0;
    int32_t nnz = 0;
};

// a random feature-sorted transpose: power-law column lengths, every column's rows ascending and distinct
static Transpose make_transpose(Rng &r, int64_t rows, int32_t n_cols, int32_t dim, bool long_cols) {
    Transpose t;
    t.rows = rows;
    std::vector<int32_t> feats;
    {
        std::vector<int32_t> all((size_t)dim);
        std::iota(all.begin(), all.end(), 0);
        std::shuffle(all.begin(), all.end(), r);
        feats.assign(all.begin(), all.begin() + std::min<int32_t>(n_cols, dim));
        std::sort(feats.begin(), feats.end());
    }
    t.hb.cfeat = feats;
    t.hb.cptr.assign(1, 0);
    for (size_t c = 0; c < feats.size(); ++c) {
        const double u = (double)(r() >> 11) / 9007199254740992.0;
        int64_t len = 1 + (int64_t)((long_cols ? 0.6 : 0.02) * (double)rows * u * u * u * u);
        if (c == 0 && long_cols) len = rows;                                       // one column with every row
        len = std::min(len, rows);
        // `len` distinct ascending rows: a random start and stride pattern
        const int64_t stride = std::max<int64_t>(rows / len, 1);
        int64_t row = uni(r, 0, stride - 1);
        for (int64_t j = 0; j < len && row < rows; ++j) {
            t.crow.push_back((uint32_t)row | (j == 0 ? 0x80000000u : 0u));           // bit 31 = first entry of its column
            row += uni(r, 1, stride);
        }
        t.hb.cptr.push_back((int32_t)t.crow.size());
    }
    t.nnz = (int32_t)t.crow.size();
    return t;
}

static void check_batch_meta_and_bands(Rng &r) {
    const int64_t rows = uni(r, 1, 60000);
    const int32_t dim = (int32_t)uni(r, 1, 4000);
    Transpose t = make_transpose(r, rows, (int32_t)uni(r, 1, dim), dim, uni(r, 0, 1) != 0);
    HostBatch &hb = t.hb;
    std::vector<int32_t> cnt((size_t)dim + 1, 0), base((size_t)dim + 1, 0);
    finish_batch_meta(hb, t.nnz, cnt, base);
    CHECK(std::all_of(cnt.begin(), cnt.end(), [](int32_t v) { return v == 0; }) && std::all_of(base.begin(), base.end(), [](int32_t v) { return v == 0; }));
    const size_t nc = hb.cfeat.size();
    const int32_t n_ranges = (t.nnz + kRangeLen - 1) / kRangeLen;
    CHECK((int32_t)hb.range_seg.size() == n_ranges && hb.n_feats == (int32_t)nc && hb.n_pieces == 0 && hb.mp_feat.empty());
    for (int32_t rho = 0; rho < n_ranges; ++rho) {
        const int32_t s = hb.range_seg[(size_t)rho], pos = rho * kRangeLen;
        CHECK(s >= 0 && (size_t)s < nc && hb.cptr[(size_t)s] <= pos && pos < hb.cptr[(size_t)s + 1]);
    }
    for (size_t c = 0; c < nc; ++c) CHECK(hb.cdst[c] == hb.cfeat[c]);
    // the fixup lists: exactly the columns the backward's predicate leaves cut, short ones and long ones apart, ascending
    std::vector<int32_t> want_short, want_long;
    for (size_t c = 0; c < nc; ++c) {
        const int32_t ra = hb.cptr[c] / kRangeLen, rb = (hb.cptr[c + 1] - 1) / kRangeLen;
        if (rb > ra && !(rb == ra + 1 && hb.cptr[c + 1] - rb * kRangeLen <= kExtend)) (rb - ra + 1 <= 8 ? want_short : want_long).push_back((int32_t)c);
    }
    CHECK(hb.split_short == want_short && hb.split_seg == want_long);
    // the band plan: every range in exactly one list, every run ascending (step_backward clips runs with lower_bound)
    std::vector<int32_t> first((size_t)n_ranges), last((size_t)n_ranges);
    for (int32_t rho = 0; rho < n_ranges; ++rho) {
        first[(size_t)rho] = (int32_t)(t.crow[(size_t)rho * kRangeLen] & 0x7fffffffu);
        last[(size_t)rho] = (int32_t)(t.crow[(size_t)std::min<int32_t>((rho + 1) * kRangeLen, t.nnz) - 1] & 0x7fffffffu);
    }
    std::vector<int32_t> lists[kXcds];
    int32_t seg[kXcds][kXSegs + 1];
    const int32_t affine = plan_bands(hb, t.nnz, rows, first, last, lists, seg);
    std::vector<int> seen((size_t)n_ranges, 0);
    int32_t in_bands = 0;
    size_t longest = 0, shortest = (size_t)-1;
    for (int x = 0; x < kXcds; ++x) {
        CHECK(seg[x][0] == 0 && seg[x][kXSegs] == (int32_t)lists[x].size());
        for (int sg = 0; sg < kXSegs; ++sg) {
            CHECK(seg[x][sg] <= seg[x][sg + 1]);
            for (int32_t i = seg[x][sg]; i < seg[x][sg + 1]; ++i) {
                const int32_t rho = lists[x][(size_t)i];
                CHECK(rho >= 0 && rho < n_ranges && !seen[(size_t)rho]);
                seen[(size_t)rho] = 1;
                if (i > seg[x][sg]) CHECK(lists[x][(size_t)i - 1] < rho);
                if (sg < kXSegs - 1) {
                    ++in_bands;
                    // placed by its band: inside one column, a full range
                    const int32_t s = hb.range_seg[(size_t)rho];
                    CHECK(hb.cptr[(size_t)s] <= rho * kRangeLen && hb.cptr[(size_t)s + 1] >= (rho + 1) * kRangeLen);
                }
            }
        }
        longest = std::max(longest, lists[x].size());
        shortest = std::min(shortest, lists[x].size());
    }
    CHECK(in_bands == affine && std::all_of(seen.begin(), seen.end(), [](int v) { return v == 1; }));
    (void)longest; (void)shortest;
    // the ALS level schedule of the same transpose
    std::vector<int32_t> lev_ptr, cols;
    const int32_t n_levels = als_levels(hb.cptr, t.crow.data(), rows, lev_ptr, cols);
    CHECK((int32_t)lev_ptr.size() == n_levels + 1 && lev_ptr[0] == 0 && lev_ptr.back() == (int32_t)nc && cols.size() == nc);
    std::vector<int32_t> level_of(nc, 0);
    {
        std::vector<int> hit(nc, 0);
        for (int32_t l = 0; l < n_levels; ++l) {
            CHECK(lev_ptr[(size_t)l] < lev_ptr[(size_t)l + 1]);                      // no empty level
            for (int32_t i = lev_ptr[(size_t)l]; i < lev_ptr[(size_t)l + 1]; ++i) {
                const int32_t c = cols[(size_t)i];
                CHECK(c >= 0 && (size_t)c < nc && !hit[(size_t)c]);
                hit[(size_t)c] = 1;
                level_of[(size_t)c] = l + 1;
                if (i > lev_ptr[(size_t)l]) CHECK(cols[(size_t)i - 1] < c);         // ascending id inside a level
            }
        }
    }
    // validity and minimality: walking the columns in id order, a column's level is 1 + the largest level among the EARLIER
    // columns that share a row with it (so no two columns of one level share a row, and the sweep order is respected)
    std::vector<int32_t> row_level((size_t)rows, 0);
    for (size_t c = 0; c < nc; ++c) {
        int32_t lv = 0;
        for (int32_t p = hb.cptr[c]; p < hb.cptr[c + 1]; ++p) lv = std::max(lv, row_level[t.crow[(size_t)p] & 0x7fffffffu]);
        CHECK(level_of[c] == lv + 1);
        for (int32_t p = hb.cptr[c]; p < hb.cptr[c + 1]; ++p) row_level[t.crow[(size_t)p] & 0x7fffffffu] = lv + 1;
    }
}

// row-blocked streams: a feature may come in several pieces; finish_batch_meta hands out piece rows
static void check_pieces(Rng &r) {
    const int32_t dim = (int32_t)uni(r, 2, 300);
    HostBatch hb;
    const int blocks = (int)uni(r, 1, 5);
    hb.cptr.assign(1, 0);
    std::vector<int32_t> per_feat((size_t)dim + 1, 0);
    for (int b = 0; b < blocks; ++b)
        for (int32_t f = 0; f <= dim; ++f)
            if (uni(r, 0, 2) == 0) {
                hb.cfeat.push_back(f);
                hb.cptr.push_back(hb.cptr.back() + (int32_t)uni(r, 1, 200));
                ++per_feat[(size_t)f];
            }
    std::vector<int32_t> cnt((size_t)dim + 1, 0), base((size_t)dim + 1, 0);
    finish_batch_meta(hb, hb.cptr.back(), cnt, base);
    int32_t feats = 0, pieces = 0;
    std::vector<int32_t> multi;
    for (int32_t f = 0; f <= dim; ++f) {
        feats += per_feat[(size_t)f] > 0;
        if (per_feat[(size_t)f] > 1) { multi.push_back(f); pieces += per_feat[(size_t)f]; }
    }
    CHECK(hb.n_feats == feats && hb.n_pieces == pieces && hb.mp_feat == multi && hb.mp_ptr.size() == multi.size() + 1);
    std::vector<int> piece_used((size_t)pieces, 0);
    for (size_t s = 0; s < hb.cfeat.size(); ++s) {
        const int32_t f = hb.cfeat[s];
        if (per_feat[(size_t)f] == 1) { CHECK(hb.cdst[s] == f); continue; }
        const int32_t piece = -1 - hb.cdst[s];
        const size_t m = (size_t)(std::lower_bound(multi.begin(), multi.end(), f) - multi.begin());
        CHECK(piece >= hb.mp_ptr[m] && piece < hb.mp_ptr[m + 1] && !piece_used[(size_t)piece]);
        piece_used[(size_t)piece] = 1;
    }
}

// ---- the data-parallel plan ------------------------------------------------------------------------------------
static void check_plan(Rng &r) {
    const int64_t n1 = uni(r, 1, 20000);
    std::vector<int32_t> cnt((size_t)n1);
    for (int64_t f = 0; f < n1; ++f) cnt[(size_t)f] = uni(r, 0, 3) == 0 ? 0 : (int32_t)(1 + 100000 / (f + 1) * uni(r, 0, 2));
    int64_t total = 0;
    for (int32_t c : cnt) total += c;
    const int nf = (int)uni(r, 0, 7);
    std::vector<double> fr((size_t)nf);
    for (auto &x : fr) x = (double)uni(r, -5, 105) / 100.0;        // out-of-range fractions are clamped
    std::sort(fr.begin(), fr.end());
    int64_t cuts[8] = {-7, -7, -7, -7, -7, -7, -7, -7};
    choose_cuts(cnt.data(), n1, nf, fr.data(), cuts);
    for (int i = 0; i < nf; ++i) {
        CHECK(cuts[i] >= 0 && cuts[i] < n1);
        if (i > 0 && cuts[i] > 0) CHECK(cuts[i] <= cuts[i - 1] || cuts[i - 1] == 0);     // larger shares reach further down
        if (cuts[i] > 0) {
            int64_t above = 0;
            for (int64_t f = cuts[i]; f < n1; ++f) above += cnt[(size_t)f];
            const double want = std::min(std::max(fr[(size_t)i], 0.0), 1.0) * (double)total;
            CHECK((double)above >= want || cuts[i] == 1);             // the share at or above the cut covers the fraction ...
            CHECK((double)(above - cnt[(size_t)cuts[i]]) < want || want <= 0.0 || i > 0);      // ... and no higher cut would (first cut: exactly)
        }
    }
    CHECK(cuts[7] == -7 || nf == 8);
    std::vector<int64_t> cv;
    for (int i = 0; i < nf; ++i)
        if (cuts[i] > 0 && cuts[i] < n1) cv.push_back(cuts[i]);
    std::sort(cv.begin(), cv.end());
    cv.erase(std::unique(cv.begin(), cv.end()), cv.end());
    for (int W : {0, 1, 2, 3, 8, 64}) {
        const std::vector<int64_t> e = interval_edges(cv, n1, W);
        CHECK(e.size() >= 2 && e.front() == 0 && e.back() == n1);
        for (size_t i = 1; i < e.size(); ++i) {
            CHECK(e[i - 1] < e[i]);
            if (W > 0 && i + 1 < e.size()) CHECK(e[i] % W == 0);
        }
        if (W == 0) CHECK(e.size() == cv.size() + 2);
        if (W <= 0) continue;
        // equal shares: the ranks' shares of every interval tile it exactly (the top one up to shard_top, into the slack rows)
        const int64_t top = shard_top(n1, W);
        CHECK(top >= n1 && top - n1 < W && top % W == 0);
        for (size_t i = 0; i + 1 < e.size(); ++i) {
            const bool is_top = i + 2 == e.size();
            int64_t at = e[i];
            for (int R = 0; R < W; ++R) {
                const Share s = shard_share(e[i], e[i + 1], is_top, n1, W, R);
                CHECK(s.hi_r == (is_top ? top : e[i + 1]) && s.chunk * W == s.hi_r - e[i]);
                CHECK(s.vlo == at && s.vhi == at + s.chunk);
                at = s.vhi;
            }
            CHECK(at == (is_top ? top : e[i + 1]));
        }
    }
}

// ---- the data-parallel step's update groups and the touched-rows exchange's compact intervals -----------------------
// the step's own loops as they were written inline in fmhip_comm.hip before apply_groups / compact_edges (dense, pipelined
// and touched): each launch as {interval waited for, lo, hi}
static std::vector<ApplyGroup> groups_dense(const std::vector<int64_t> &edge, int64_t n1) {
    std::vector<ApplyGroup> out;
    const int n_int = (int)edge.size() - 1;
    int64_t pend_hi = -1;
    for (int i = n_int - 1; i >= 0; --i) {
        const int64_t lo = edge[(size_t)i], hi = edge[(size_t)i + 1];
        if (pend_hi < 0) pend_hi = hi;
        const bool last = i == 0;
        if (!last && (pend_hi - lo) * 8 < n1) continue;
        out.push_back({i, lo, pend_hi});
        pend_hi = -1;
    }
    return out;
}
static std::vector<ApplyGroup> groups_pipelined(const std::vector<int64_t> &edge, int64_t n1) {
    std::vector<ApplyGroup> out;
    const int n_int = (int)edge.size() - 1, T = n_int - 1;
    int64_t pend_hi = -1;
    for (int i = T - 1; i >= 0; --i) {
        const int64_t lo = edge[(size_t)i], hi = edge[(size_t)i + 1];
        if (pend_hi < 0) pend_hi = hi;
        if (i > 0 && (pend_hi - lo) * 8 < n1) continue;
        out.push_back({i, lo, pend_hi});
        pend_hi = -1;
    }
    return out;
}
static void edges_touched(const std::vector<int64_t> &cuts, int64_t n1, const int32_t *cut_pos, int32_t n_u, std::vector<int64_t> &edge,
                          std::vector<int64_t> &pe) {
    edge.assign(1, 0);
    pe.assign(1, 0);
    for (size_t i = 0; i < cuts.size(); ++i) {
        const int64_t x = cuts[i];
        if (x > edge.back() && x < n1) {
            edge.push_back(x);
            pe.push_back(cut_pos[i]);
        }
    }
    edge.push_back(n1);
    pe.push_back(n_u);
}
static std::vector<ApplyGroup> groups_touched(const std::vector<int64_t> &pe, int32_t n_u) {
    std::vector<ApplyGroup> out;
    const int n_int = (int)pe.size() - 1;
    int64_t pend_hi = -1;
    for (int i = n_int - 1; i >= 0; --i) {
        const int64_t plo = pe[(size_t)i], phi = pe[(size_t)i + 1];
        if (pend_hi < 0) pend_hi = phi;
        const bool last = i == 0;
        if (!last && (pend_hi - plo) * 8 < n_u) continue;
        out.push_back({i, plo, pend_hi});
        pend_hi = -1;
    }
    return out;
}
static bool same_groups(const std::vector<ApplyGroup> &a, const std::vector<ApplyGroup> &b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if (a[i].at != b[i].at || a[i].lo != b[i].lo || a[i].hi != b[i].hi) return false;
    return true;
}
// the groups tile the rows [edges[0], edges[first + 1]) from the top down and the last one waits for interval 0
static void check_tiling(const std::vector<ApplyGroup> &g, const std::vector<int64_t> &edges, int first) {
    if (first < 0) { CHECK(g.empty()); return; }
    CHECK(!g.empty() && g.back().at == 0 && g.back().lo == edges[0]);
    int64_t top = edges[(size_t)first + 1];
    int prev = first + 1;
    for (const ApplyGroup &x : g) {
        CHECK(x.at < prev && x.hi == top && x.lo == edges[(size_t)x.at] && x.lo <= x.hi);
        top = x.lo;
        prev = x.at;
    }
}

static void check_groups(Rng &r) {
    const int64_t n1 = uni(r, 1, uni(r, 0, 1) ? 64 : 200000);
    // up to FMHIP_DP_MAX_CUTS cuts, ascending; some collapsed (0), some at or past n1, some equal, some clustered near the top
    const int nc = (int)uni(r, 0, 7);
    std::vector<int64_t> cuts((size_t)nc);
    for (auto &x : cuts) {
        const int64_t k = uni(r, 0, 5);
        x = k == 0 ? 0 : k == 1 ? n1 + uni(r, 0, 2) : k == 2 ? std::max<int64_t>(n1 - uni(r, 1, 40), 0) : uni(r, 0, n1);
    }
    std::sort(cuts.begin(), cuts.end());
    if (nc > 1 && uni(r, 0, 3) == 0) cuts[1] = cuts[0];
    const std::vector<int64_t> edge = interval_edges(cuts, n1, 0);
    const int n_int = (int)edge.size() - 1;
    const std::vector<ApplyGroup> gd = apply_groups(edge, n1, n_int - 1);
    CHECK(same_groups(gd, groups_dense(edge, n1)));
    check_tiling(gd, edge, n_int - 1);
    if (n_int >= 2) {
        const std::vector<ApplyGroup> gp = apply_groups(edge, n1, n_int - 2);
        CHECK(same_groups(gp, groups_pipelined(edge, n1)));
        check_tiling(gp, edge, n_int - 2);
    }
    // the touched mode: the cuts' positions in a union of n_u rows (lower bounds: ascending, within [0, n_u])
    const int32_t n_u = (int32_t)uni(r, 0, uni(r, 0, 1) ? 50 : 100000);
    int32_t cut_pos[8] = {};
    for (int i = 0; i < nc; ++i) cut_pos[i] = (int32_t)uni(r, 0, n_u);
    std::sort(cut_pos, cut_pos + nc);
    std::vector<int64_t> e_ref, pe_ref;
    edges_touched(cuts, n1, cut_pos, n_u, e_ref, pe_ref);
    const CompactEdges ce = compact_edges(cuts, n1, cut_pos, n_u);
    CHECK(ce.edge == e_ref && ce.pe == pe_ref && ce.edge == edge);
    const std::vector<ApplyGroup> gt = apply_groups(ce.pe, n_u, (int)ce.pe.size() - 2);
    CHECK(same_groups(gt, groups_touched(ce.pe, n_u)));
    check_tiling(gt, ce.pe, (int)ce.pe.size() - 2);
}

// ---- the dataset build: validation, the dense hot block's choice and split, forward row order, ALS row sort, own bitmaps ----
template <typename FT>
struct Rows {
    int64_t n_rows = 0;
    std::vector<int64_t> rp;
    std::vector<int32_t> col;
    std::vector<FT> val;
};

// Rows over n_feat ids of which n_cand (scattered over the id range) are frequent: the first n_page0 of them in 12-90 % of the
// rows, the others in 3-6 %; every other id is rare.  Some rows are empty, the entries of a row are shuffled.  refuse_a (a
// page-0 feature) / refuse_b (a later one), when >= 0: stored twice in some rows, or with a value that is 0 as fp32
template <typename FT>
static Rows<FT> make_rows(Rng &r, int64_t n_rows, int32_t n_feat, int n_cand, int n_page0, int refuse_a, int refuse_b) {
    Rows<FT> d;
    d.n_rows = n_rows;
    d.rp.assign((size_t)n_rows + 1, 0);
    std::vector<int32_t> ids((size_t)n_feat);
    std::iota(ids.begin(), ids.end(), 0);
    std::shuffle(ids.begin(), ids.end(), r);
    n_cand = std::min<int>(n_cand, n_feat);
    std::vector<int> freq((size_t)n_cand);                                     // in 1/1000 of the rows
    for (int j = 0; j < n_cand; ++j) freq[(size_t)j] = j < n_page0 ? (int)uni(r, 120, 900) : (int)uni(r, 30, 60);
    const bool dup_a = uni(r, 0, 1) != 0, dup_b = uni(r, 0, 1) != 0;
    const FT zero = sizeof(FT) == 8 && uni(r, 0, 1) ? (FT)1e-60 : (FT)0;       // a double that is 0 only as fp32, or 0
    std::vector<std::pair<int32_t, FT>> row;
    for (int64_t i = 0; i < n_rows; ++i) {
        row.clear();
        if (n_feat > 0 && uni(r, 0, 19) != 0) {
            for (int j = 0; j < n_cand; ++j) {
                if (uni(r, 0, 999) >= freq[(size_t)j]) continue;
                FT x = (FT)((double)uni(r, 1, 1000) / 500.0 - 1.001);
                const bool refused = j == refuse_a || j == refuse_b, dup = j == refuse_a ? dup_a : dup_b;
                if (refused && !dup && uni(r, 0, 3) == 0) x = zero;
                row.push_back({ids[(size_t)j], x});
                if (refused && dup && uni(r, 0, 3) == 0) row.push_back({ids[(size_t)j], (FT)0.5});
            }
            if (n_feat > n_cand)
                for (int64_t e = uni(r, 0, 4); e > 0; --e) row.push_back({ids[(size_t)uni(r, n_cand, n_feat - 1)], (FT)((double)uni(r, 1, 100) / 50.0)});
            std::shuffle(row.begin(), row.end(), r);
        }
        for (const auto &e : row) { d.col.push_back(e.first); d.val.push_back(e.second); }
        d.rp[(size_t)i + 1] = (int64_t)d.col.size();
    }
    return d;
}

template <typename T>
static bool same_array(const T *a, const T *b, size_t n) { return n == 0 || memcmp(a, b, n * sizeof(T)) == 0; }

// one dataset through the host passes as fmhip_dataset_create chains them, each with 1 and with 4 threads (equal outputs), each
// against what the device code relies on.  shape: the corner the case is built around (see the table in the body)
template <typename FT>
static void check_dataset_build(Rng &r, int shape) {
    int64_t n_rows = uni(r, 2, 3000);
    int32_t n_feat = (int32_t)uni(r, 2, 600);
    int n_cand = (int)uni(r, 0, 40), n_page0 = (int)uni(r, 0, 20), max_pages = (int)uni(r, 1, kHotPages);
    bool row_blocked = false;
    int sample_stride = 0;                                                   // > 0: counts from every so-manieth row or so
    switch (shape) {
        case 0: n_rows = 0; break;
        case 1: n_rows = 1; break;
        case 2: n_feat = 0; n_cand = 0; break;                                 // zero nonzeros
        case 3: n_feat = 1; n_cand = 1; n_page0 = 1; break;                    // dimension 0
        case 4: n_rows = 2000; n_cand = 5; n_page0 = 1; break;                 // one feature at the 10 % mark: no block
        case 5: n_cand = n_page0 = kHotT; break;
        case 6: n_cand = n_page0 = kHotT + 1; max_pages = (int)uni(r, 1, 2); break;
        case 7: n_rows = uni(r, 1000, 2000); n_cand = (int)uni(r, 128, 140); n_page0 = (int)uni(r, 2, 20); max_pages = kHotPages; break;
        case 8: row_blocked = true; n_cand = 40; n_page0 = 10; max_pages = 4; break;
        case 9: n_rows = uni(r, 2000, 4000); n_cand = 30; n_page0 = 12; sample_stride = (int)uni(r, 2, 16); break;
        case 10: n_rows = uni(r, 17000, 20000); n_cand = 20; n_page0 = 6; sample_stride = (g_case / 12 & 1) * 2; break;   // a histogram per thread, of all rows / of every other row
        default: break;
    }
    n_feat = std::max<int32_t>(n_feat, std::min<int32_t>(n_cand, 1));
    n_page0 = std::min(n_page0, n_cand);
    const int refuse_a = n_page0 > 2 && uni(r, 0, 2) ? (int)uni(r, 0, n_page0 - 1) : -1;
    const int refuse_b = n_cand > n_page0 && uni(r, 0, 2) ? (int)uni(r, n_page0, n_cand - 1) : -1;
    Rows<FT> d = make_rows<FT>(r, n_rows, n_feat, n_cand, n_page0, refuse_a, refuse_b);
    const int64_t nnz = d.rp[(size_t)n_rows];
    // the exact / sampled threshold as an argument: the stride is nnz / (threshold / 2)
    const int64_t exact_nnz = sample_stride > 0 ? std::max<int64_t>(nnz * 2 / sample_stride - 1, 2) : kHotExactNnz;
    const int64_t *rp = d.rp.data();
    // (an empty vector's data() may be NULL: the library is handed NULL arrays for datasets without entries too)
    const int32_t *col = d.col.data();
    const FT *val = d.val.data();
    const int kThreads[2] = {1, 4};

    // ---- validate_rows: clean rows; the FIRST negative entry; the FIRST row where row_ptr decreases
    int32_t dim = 0;
    for (int32_t c : d.col) dim = std::max(dim, c);
    for (int T : kThreads) {
        const RowCheck ok = validate_rows(n_rows, rp, col, T);
        CHECK(ok.bad_row == -1 && ok.bad_entry == -1 && ok.dim == dim);
        if (nnz > 0) {
            const int64_t a = uni(r, 0, nnz - 1), b = uni(r, 0, nnz - 1);
            const int32_t ka = d.col[(size_t)a], kb = d.col[(size_t)b];
            d.col[(size_t)a] = -1;
            d.col[(size_t)b] = INT32_MIN;
            const RowCheck bad = validate_rows(n_rows, rp, col, T);
            CHECK(bad.bad_row == -1 && bad.bad_entry == std::min(a, b));
            d.col[(size_t)a] = ka;
            d.col[(size_t)b] = kb;
        }
        std::vector<int64_t> rp2 = d.rp;
        int64_t first = -1;
        for (int j = 0; j < 2 && n_rows > 0; ++j) {
            const int64_t i = uni(r, 0, n_rows - 1);
            if (rp2[(size_t)i] < 1 || rp2[(size_t)i + 1] < rp2[(size_t)i]) continue;
            rp2[(size_t)i + 1] = rp2[(size_t)i] - 1;                               // (row i + 1 then starts lower too: still not a decrease)
            first = first < 0 ? i : std::min(first, i);
        }
        if (first >= 0)
            for (int64_t i = 0; i < n_rows; ++i)
                if (rp2[(size_t)i + 1] < rp2[(size_t)i]) { first = i; break; }
        CHECK(validate_rows(n_rows, rp2.data(), nullptr, T).bad_row == first);
    }

    // ---- choose_hot_block
    HotBlock hb[2];
    for (int t = 0; t < 2; ++t) hb[t] = choose_hot_block<FT>(n_rows, rp, col, val, dim, max_pages, row_blocked, kThreads[t], exact_nnz);
    CHECK(hb[0].pages == hb[1].pages && hb[0].p0 == hb[1].p0 && hb[0].hot_ids == hb[1].hot_ids && hb[0].slot == hb[1].slot && hb[0].kept == hb[1].kept);
    const HotBlock &h = hb[0];
    // what the rows say: entries per feature, and the features that may not be dense (twice in a row, or a stored zero)
    std::vector<int64_t> cnt((size_t)dim + 1, 0);
    std::vector<char> refusable((size_t)dim + 1, 0);
    {
        std::vector<int64_t> last_row((size_t)dim + 1, -1);
        for (int64_t i = 0; i < n_rows; ++i)
            for (int64_t p = rp[i]; p < rp[i + 1]; ++p) {
                const size_t f = (size_t)col[p];
                ++cnt[f];
                if (last_row[f] == i || (float)val[p] == 0.f) refusable[f] = 1;
                last_row[f] = i;
            }
    }
    CHECK(h.slot.size() == (size_t)dim + 1 || h.pages == 0);
    if (h.pages == 0) {
        CHECK(h.hot_ids.empty() && h.p0 == 0);
    } else {
        CHECK(h.pages >= 1 && h.pages <= (row_blocked ? 1 : max_pages) && h.pages <= kHotPages && h.hot_ids.size() == (size_t)h.pages * kHotT);
        CHECK(h.p0 >= 2 && h.p0 <= (size_t)kHotT);
        std::vector<int> slot_ref((size_t)dim + 1, -1);
        for (int pg = 0; pg < h.pages; ++pg) {
            int live = 0;
            while (live < kHotT && h.hot_ids[(size_t)(pg * kHotT + live)] >= 0) ++live;
            for (int s2 = 0; s2 < kHotT; ++s2) {
                const int32_t f = h.hot_ids[(size_t)(pg * kHotT + s2)];
                CHECK(s2 < live ? (f >= 0 && f <= dim) : f == -1);                 // live slots first
                if (s2 > 0 && s2 < live) CHECK(h.hot_ids[(size_t)(pg * kHotT + s2 - 1)] < f);   // ascending (k_fill_hot_pages searches them)
                if (s2 < live) { CHECK(!refusable[(size_t)f] && slot_ref[(size_t)f] == -1); slot_ref[(size_t)f] = pg * kHotT + s2; }
            }
            CHECK(pg == 0 ? (size_t)live == h.p0 : (live >= 1 && (live == kHotT || pg == h.pages - 1)));   // no empty page, only the last one partly filled
        }
        for (int32_t f = 0; f <= dim; ++f) CHECK((int)h.slot[(size_t)f] == slot_ref[(size_t)f]);
        for (int64_t i = 0; i < n_rows; ++i) {
            int64_t keep = 0;
            for (int64_t p = rp[i]; p < rp[i + 1]; ++p) keep += h.slot[(size_t)col[p]] < 0 || h.slot[(size_t)col[p]] >= kHotT;
            CHECK(h.kept[(size_t)i + 1] == keep);
        }
    }
    if (nnz <= exact_nnz && nnz > 0) {
        // exact counts: the candidates (>= 2.5 % of the rows) by descending count, ties by ascending id, WITHOUT the refusable
        // ones — page 0 is the leading ones at >= 10 % (at most kHotT, at least 2 or there is no block), the other pages take
        // the next ones while there is room: a refused feature's place goes to the next candidate, none is skipped
        std::vector<int32_t> surv;
        for (int32_t f = 0; f <= dim; ++f)
            if (cnt[(size_t)f] * 40 >= n_rows && !refusable[(size_t)f]) surv.push_back(f);
        std::sort(surv.begin(), surv.end(), [&](int32_t x, int32_t y) { return cnt[(size_t)x] != cnt[(size_t)y] ? cnt[(size_t)x] > cnt[(size_t)y] : x < y; });
        size_t p0 = 0;
        while (p0 < surv.size() && p0 < (size_t)kHotT && cnt[(size_t)surv[p0]] * 10 >= n_rows) ++p0;
        const size_t rest = p0 < 2 ? 0 : std::min(surv.size() - p0, (size_t)kHotT * (size_t)((row_blocked ? 1 : max_pages) - 1));
        if (p0 < 2) {
            CHECK(h.pages == 0);
        } else {
            CHECK(h.p0 == p0 && h.pages == 1 + (int)((rest + kHotT - 1) / kHotT));
            for (size_t j = 0; j < p0 + rest; ++j) {
                const int sl = h.slot[(size_t)surv[j]];
                CHECK(j < p0 ? (sl >= 0 && sl < kHotT) : (sl >= kHotT + (int)((j - p0) / kHotT * kHotT) && sl < kHotT + (int)(((j - p0) / kHotT + 1) * kHotT)));
            }
            size_t live = 0;
            for (int32_t f : h.hot_ids) live += f >= 0;
            CHECK(live == p0 + rest);
        }
    } else if (nnz == 0) {
        CHECK(h.pages == 0);
    }

    // ---- split_hot_rows (only a chosen block is split); the stream the device will hold either way
    const int64_t batch_rows = std::max<int64_t>(std::min(uni(r, 1, n_rows + 3), n_rows), 1);      // as the caller clamps it
    const int64_t nb = n_rows > 0 ? (n_rows + batch_rows - 1) / batch_rows : 0;
    const int64_t *walk_ptr = rp;
    HotSplit sp[2];
    if (h.pages > 0) {
        for (int t = 0; t < 2; ++t) sp[t] = split_hot_rows<FT>(n_rows, rp, col, val, dim, batch_rows, hb[t], kThreads[t]);
        const HotSplit &s = sp[0];
        const int64_t kept = s.sp_ptr[(size_t)n_rows];
        CHECK(s.sp_ptr == sp[1].sp_ptr && s.bwd_out == sp[1].bwd_out && s.drop_bits == sp[1].drop_bits && s.hot_masks.size() == sp[1].hot_masks.size());
        CHECK(same_array(s.hot_masks.data(), sp[1].hot_masks.data(), s.hot_masks.size()));
        CHECK(same_array(s.sp_col.get(), sp[1].sp_col.get(), (size_t)kept) && same_array(s.sp_val.get(), sp[1].sp_val.get(), (size_t)kept));
        CHECK(same_array(s.xhot0.get(), sp[1].xhot0.get(), (size_t)n_rows * kHotT));
        CHECK(s.sp_ptr.size() == (size_t)n_rows + 1 && s.sp_ptr[0] == 0 && s.hot_masks.size() == (size_t)nb && s.bwd_out.size() == (size_t)nb);
        std::vector<slotmask_t> masks((size_t)nb, 0);
        std::vector<int64_t> outb((size_t)nb, 0);
        for (int64_t i = 0; i < n_rows; ++i) {
            // the kept entries in stored order + the non-zero slots of page 0 = the row
            int64_t o = s.sp_ptr[(size_t)i];
            float x0[kHotT] = {};
            for (int64_t p = rp[i]; p < rp[i + 1]; ++p) {
                const int sl = h.slot[(size_t)col[p]];
                if (sl >= 0) masks[(size_t)(i / batch_rows)] |= (slotmask_t)1 << sl;
                if (sl >= 0 && sl < kHotT) { x0[sl] = (float)val[p]; continue; }
                CHECK(o < s.sp_ptr[(size_t)i + 1] && s.sp_col[(size_t)o] == col[p] && s.sp_val[(size_t)o] == (float)val[p]);
                ++o;
                outb[(size_t)(i / batch_rows)] += sl >= kHotT;                    // pages 1..: stays in the CSR, leaves the transposes
            }
            CHECK(o == s.sp_ptr[(size_t)i + 1]);
            CHECK(same_array(x0, s.xhot0.get() + (size_t)i * kHotT, (size_t)kHotT));
        }
        CHECK(same_array(masks.data(), s.hot_masks.data(), (size_t)nb) && outb == s.bwd_out);
        CHECK(s.drop_bits.empty() == (h.pages == 1));
        if (h.pages > 1) {
            CHECK(s.drop_bits.size() >= (size_t)dim / 32 + 1);
            for (size_t w = 0; w < s.drop_bits.size(); ++w)
                for (int b = 0; b < 32; ++b) {
                    const size_t f = w * 32 + (size_t)b;
                    CHECK((s.drop_bits[w] >> b & 1u) == (f <= (size_t)dim && h.slot[f] >= kHotT ? 1u : 0u));
                }
        }
        walk_ptr = s.sp_ptr.data();
    }

    // ---- forward_row_order over that stream: whole batches, and windows (odd ones reversed)
    for (int64_t window : {(int64_t)0, uni(r, 1, 3), (int64_t)64}) {
        const std::vector<int32_t> order = forward_row_order(n_rows, batch_rows, walk_ptr, window, 1);
        CHECK(order == forward_row_order(n_rows, batch_rows, walk_ptr, window, 4) && order.size() == (size_t)n_rows);
        std::vector<char> seen;
        for (int64_t b = 0; b < nb; ++b) {
            const int64_t row0 = b * batch_rows, rows = std::min(batch_rows, n_rows - row0), win = window > 0 ? window : rows;
            seen.assign((size_t)rows, 0);
            for (int64_t w0 = 0; w0 < rows; w0 += win) {
                const int64_t w1 = std::min(rows, w0 + win);
                const bool reversed = window > 0 && ((w0 / win) & 1);
                for (int64_t i = w0; i < w1; ++i) {
                    const int64_t lr = order[(size_t)(row0 + i)];
                    CHECK(lr >= w0 && lr < w1 && !seen[(size_t)lr]);                    // a permutation of the window's local row ids
                    seen[(size_t)lr] = 1;
                    if (i == w0) continue;
                    // longest first, ties in row order (a reversed window: the mirror image)
                    const int64_t a = order[(size_t)(row0 + (reversed ? i : i - 1))], c = order[(size_t)(row0 + (reversed ? i - 1 : i))];
                    const int64_t la = walk_ptr[row0 + a + 1] - walk_ptr[row0 + a], lc = walk_ptr[row0 + c + 1] - walk_ptr[row0 + c];
                    CHECK(la > lc || (la == lc && a < c));
                }
            }
        }
    }

    // ---- sort_rows_by_feature (the caller's rows): per row, by id, equal ids in stored order
    const SortedRows sr = sort_rows_by_feature<FT>(n_rows, rp, col, val, 1), sr4 = sort_rows_by_feature<FT>(n_rows, rp, col, val, 4);
    CHECK(sr.scol == sr4.scol && same_array(sr.sval.data(), sr4.sval.data(), sr.sval.size()) && sr.dup == sr4.dup);
    CHECK(sr.scol.size() == (size_t)nnz && sr.sval.size() == (size_t)nnz);
    bool dup = false;
    std::vector<char> taken;
    for (int64_t i = 0; i < n_rows; ++i) {
        taken.assign((size_t)(rp[i + 1] - rp[i]), 0);
        for (int64_t p = rp[i]; p < rp[i + 1]; ++p) {
            if (p > rp[i]) CHECK(sr.scol[(size_t)p - 1] <= sr.scol[(size_t)p]);
            dup = dup || (p > rp[i] && sr.scol[(size_t)p - 1] == sr.scol[(size_t)p]);
            // stable: the entry is the FIRST stored one of its id not handed out yet
            int64_t q = rp[i];
            while (q < rp[i + 1] && (taken[(size_t)(q - rp[i])] || col[q] != sr.scol[(size_t)p])) ++q;
            CHECK(q < rp[i + 1] && sr.sval[(size_t)p] == (double)val[q]);
            taken[(size_t)(q - rp[i])] = 1;
        }
    }
    CHECK(sr.dup == dup);
}

// The histogram rule's other branch: per-thread tables of dim + 1 counters would pass 256 MB in all (4 threads: ids beyond 2^24),
// so ONE table is filled by one thread.  The same rows with and without a single entry of such an id choose the same block.
static void check_hot_block_one_table(Rng &r) {
    Rows<float> d = make_rows<float>(r, 9000, 300, 24, 8, 1, 20);
    int32_t dim = 0;
    for (int32_t c : d.col) dim = std::max(dim, c);
    const HotBlock small = choose_hot_block<float>(d.n_rows, d.rp.data(), d.col.data(), d.val.data(), dim, 3, false, 4);
    size_t at = (size_t)uni(r, 0, (int64_t)d.col.size() - 1);
    while (small.slot[(size_t)d.col[at]] >= 0) at = (at + 1) % d.col.size();        // (not an entry of a chosen feature)
    const int32_t big = (int32_t)(((int64_t)1 << 24) + uni(r, 0, 1000));
    d.col[at] = big;
    HotBlock hb[2];
    for (int t = 0; t < 2; ++t) hb[t] = choose_hot_block<float>(d.n_rows, d.rp.data(), d.col.data(), d.val.data(), big, 3, false, t ? 4 : 1);
    CHECK(small.pages >= 2 && hb[0].pages == small.pages && hb[0].p0 == small.p0 && hb[0].hot_ids == small.hot_ids && hb[0].kept == small.kept);
    CHECK(hb[1].pages == small.pages && hb[1].p0 == small.p0 && hb[1].hot_ids == small.hot_ids && hb[1].kept == small.kept && hb[1].slot == hb[0].slot);
    CHECK(hb[0].slot.size() == (size_t)big + 1 && hb[0].slot[(size_t)big] == -1);
}

// sort_rows_by_feature at its edges: equal ids at the very start of a row, in neighbouring rows (no duplicate), apart in a row
static void check_row_sort_edges() {
    const int64_t rp[] = {0, 2, 3, 4, 7};
    const int32_t col[] = {3, 3, 3, 3, 2, 1, 2};
    const double val[] = {1, 2, 3, 4, 5, 6, 7};
    for (int T : {1, 4}) {
        CHECK(sort_rows_by_feature<double>(1, rp, col, val, T).dup);                                   // {3, 3}
        CHECK(!sort_rows_by_feature<double>(2, rp + 1, col, val, T).dup);                               // {3}, {3}
        const SortedRows s = sort_rows_by_feature<double>(1, rp + 3, col, val, T);                      // {2, 1, 2}
        CHECK(s.dup && s.scol[4] == 1 && s.scol[5] == 2 && s.scol[6] == 2 && s.sval[4] == 6 && s.sval[5] == 5 && s.sval[6] == 7);
    }
}

// own_bitmaps: a batch's bits = the features of its cut columns (both fixup lists) + the live slots of the hot block
static void check_own_bitmaps(Rng &r) {
    const int32_t dim = (int32_t)uni(r, 0, 700);
    std::vector<HostBatch> hbs((size_t)uni(r, 0, 4));
    std::vector<int32_t> hot_ids((size_t)(uni(r, 0, 3) * kHotT), -1);
    for (auto &f : hot_ids)
        if (uni(r, 0, 2) == 0) f = (int32_t)uni(r, 0, dim);
    std::vector<std::vector<char>> want(hbs.size(), std::vector<char>((size_t)dim + 1, 0));
    for (size_t b = 0; b < hbs.size(); ++b) {
        HostBatch &hb = hbs[b];
        for (int32_t f = 0; f <= dim; ++f)
            if (uni(r, 0, 3) == 0) hb.cfeat.push_back(f);
        for (size_t c = 0; c < hb.cfeat.size(); ++c) {
            const int64_t k = uni(r, 0, 5);
            if (k == 0) hb.split_seg.push_back((int32_t)c);
            if (k == 1) hb.split_short.push_back((int32_t)c);
            if (k <= 1) want[b][(size_t)hb.cfeat[c]] = 1;
        }
        for (int32_t f : hot_ids)
            if (f >= 0) want[b][(size_t)f] = 1;
    }
    const std::vector<uint32_t> own = own_bitmaps(hbs, hot_ids, dim);
    const size_t words = (size_t)dim / 32 + 1;
    CHECK(own.size() == hbs.size() * words);
    for (size_t b = 0; b < hbs.size(); ++b)
        for (size_t f = 0; f < words * 32; ++f) CHECK((own[b * words + f / 32] >> (f & 31) & 1u) == (f <= (size_t)dim && want[b][f] ? 1u : 0u));
}

// ---- the split step's backward window (bw_window_step: fmhip_step_backward's tiling rule) -------------------------------
// The intervals [e[j], e[j+1]) of one cut of [0, n1), walked in EVERY order: `used` marks the calls accepted so far (depth of
// them), which by the rule are the top `depth` intervals (descending) or the bottom ones (ascending, up).  Every interval still
// unused is offered as the next call: only the one that continues the order may be accepted, with its own flags; any other is
// refused with the window as it was.  After the last interval the window is closed and refuses everything.
struct WindowWalk {
    int64_t n1;
    std::vector<int64_t> e;
    int k() const { return (int)e.size() - 1; }
    int64_t calls = 0;

    BwVerdict call(BwWindow w, int j, bool finish, bool open_top) {
        ++calls;
        return bw_window_step(w, n1, e[(size_t)j], open_top ? INT64_MAX : e[(size_t)j + 1], finish);
    }
    void walk(BwWindow w, int depth, bool up, unsigned used) {
        if (depth == k()) {
            CHECK(w.closed());
            for (int j = 0; j < k(); ++j)
                for (int finish = 0; finish < 2; ++finish) {
                    const BwVerdict v = call(w, j, finish != 0, false);
                    CHECK(v.refusal == BwRefusal::kClosed && v.next == w);
                }
            CHECK(bw_refusal_text(call(w, 0, false, false)) == "fmhip_step_backward without fmhip_step_forward");
            return;
        }
        CHECK(!w.closed());
        for (int j = 0; j < k(); ++j) {
            if (used >> j & 1u) continue;
            // the first call says which way: the top interval descends (a single interval is both, and descends), the bottom one ascends
            const bool down_ok = (depth == 0 || !up) && j == k() - 1 - depth, up_ok = (depth == 0 ? k() > 1 : up) && j == depth;
            for (int open_top = 0; open_top < (j == k() - 1 ? 2 : 1); ++open_top) {      // hi beyond n1 is n1
                const BwVerdict v = call(w, j, false, open_top != 0);
                if (down_ok || up_ok) {
                    CHECK(v.refusal == BwRefusal::kNone && v.own == (down_ok ? kOwnLower : kOwnUpper));
                    CHECK(v.next.closed() == (depth + 1 == k()));
                    if (!open_top) walk(v.next, depth + 1, up_ok, used | 1u << j);
                } else {
                    CHECK(v.refusal == (depth > 0 && up ? BwRefusal::kNotAscending : BwRefusal::kNotDescending) && v.next == w);
                    CHECK(v.got == (depth > 0 && up ? e[(size_t)j] : open_top ? INT64_MAX : e[(size_t)j + 1]));
                    CHECK(v.want == (depth == 0 ? n1 : up ? e[(size_t)depth] : e[(size_t)(k() - depth)]));
                }
                // finish belongs to the interval that starts at feature 0, and changes nothing else
                const BwVerdict f = call(w, j, true, open_top != 0);
                if (j > 0) CHECK(f.refusal == BwRefusal::kFinishAboveZero && f.next == w);
                else CHECK(f.refusal == v.refusal && f.own == v.own && f.next == v.next);
            }
        }
    }
};

static void check_backward_window() {
    int64_t calls = 0;
    for (int64_t n1 : {1, 2, 7, 300})
        for (int64_t a = 1; a <= n1; ++a)              // cuts 0 < a < b < c < n1 (a cut at n1: none, and none above it)
            for (int64_t b = a < n1 ? a + 1 : n1; b <= n1; ++b)
                for (int64_t c = b < n1 ? b + 1 : n1; c <= n1; ++c) {
                    WindowWalk ww{n1, {0}};
                    for (int64_t x : {a, b, c})
                        if (x < n1) ww.e.push_back(x);
                    ww.e.push_back(n1);
                    ww.walk(BwWindow::opened(), 0, false, 0u);
                    // no forward, no window
                    CHECK(ww.call(BwWindow{}, ww.k() - 1, false, false).refusal == BwRefusal::kClosed);
                    calls += ww.calls;
                }
    // the refusals' texts, byte for byte
    BwVerdict v = bw_window_step(BwWindow::opened(), 300, 90, 180, false);
    CHECK(bw_refusal_text(v) == "feature intervals must tile [0, n+1) in descending order (expected hi = 300, got 180), or start at feature 0 and ascend");
    v = bw_window_step(BwWindow{180, false}, 300, 0, 90, true);
    CHECK(bw_refusal_text(v) == "feature intervals must tile [0, n+1) in descending order (expected hi = 180, got 90), or start at feature 0 and ascend");
    v = bw_window_step(BwWindow{90, true}, 300, 180, 300, false);
    CHECK(bw_refusal_text(v) == "feature intervals must tile [0, n+1) in ascending order (expected lo = 90, got 180)");
    v = bw_window_step(BwWindow::opened(), 300, 180, 300, true);
    CHECK(bw_refusal_text(v) == "finish = 1 belongs to the interval that starts at feature 0");
    CHECK(bw_refusal_text(bw_window_step(BwWindow::opened(), 300, 0, 300, true)).empty());
    printf("host_arith_harness: backward window: %lld calls: checks ok\n", (long long)calls);
}

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "window")) {      // exhaustive and unseeded: a run of its own
        check_backward_window();
        return 0;
    }
    g_seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    const int cases = argc > 2 ? atoi(argv[2]) : 40;
    Rng r(g_seed);
    for (g_case = 0; g_case < cases; ++g_case) {
        check_shards(r);
        check_relabel(r, false);
        check_batch_meta_and_bands(r);
        check_pieces(r);
        check_plan(r);
        for (int j = 0; j < 20; ++j) check_groups(r);
        check_dataset_build<float>(r, g_case % 12);
        check_dataset_build<double>(r, (g_case + 6) % 12);
        check_own_bitmaps(r);
    }
    g_case = -1;
    // the multi-threaded paths: private tables per thread, and (tables too large for that) one table with atomic adds
    setenv("FMHIP_HOST_THREADS", "4", 1);
    check_relabel(r, false);
    check_relabel(r, true);
    unsetenv("FMHIP_HOST_THREADS");
    check_hot_block_one_table(r);
    check_row_sort_edges();
    printf("host_arith_harness: seed %llu, %d cases: checks ok\n", (unsigned long long)g_seed, cases);
    return 0;
}
