// host_arith_harness.cpp — the library's pure host arithmetic (sparkfm_amd/csrc/fmhip_host.cpp) under AddressSanitizer and
// UBSan: tests/test_host_cpu.py compiles this file together with fmhip_host.cpp with `g++ -fsanitize=address,undefined` (no
// HIP, no GPU) and runs it over seeded random shapes.  Every function is checked against its own contract — what the device
// code and the other host code RELY on (a band plan whose runs are not ascending makes step_backward's lower_bound clip the
// wrong ranges; a level schedule that puts two columns sharing a row side by side races in k_als_level) — while the sanitizers
// watch the index arithmetic.  VERDICT r4 next #6; the sanitizers cannot run on the GPU pool.
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

int main(int argc, char **argv) {
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
    }
    g_case = -1;
    // the multi-threaded paths: private tables per thread, and (tables too large for that) one table with atomic adds
    setenv("FMHIP_HOST_THREADS", "4", 1);
    check_relabel(r, false);
    check_relabel(r, true);
    unsetenv("FMHIP_HOST_THREADS");
    printf("host_arith_harness: seed %llu, %d cases: checks ok\n", (unsigned long long)g_seed, cases);
    return 0;
}
