// fmhip_host.cpp — the library's pure host arithmetic (fmhip_host.h): no HIP, no GPU.  Part of libfmhip.so, and compiled on
// its own with g++ -fsanitize=address,undefined by the CPU suite (tests/host_arith_harness.cpp).
#include "fmhip_host.h"
#include "mcmc_rng.h"

#include <stdio.h>
#include <stdlib.h>

#include <math.h>

#include <algorithm>
#include <atomic>
#include <cfloat>
#include <cmath>
#include <numeric>

namespace fmhip {
namespace host {

// Host-side passes of the dataset build (validation, dense-hot-block split, forward row order, fp32
// re-pack) run over row chunks on all host cores: they are what `DataSet.cache()` costs before the
// device takes over (single-threaded they took 3.9 s for C4's 10 M rows).
int host_threads(int64_t work_items) {
    unsigned hc = std::thread::hardware_concurrency();
    int64_t t = hc ? (int64_t)hc : 4;
    if (const char *e = getenv("FMHIP_HOST_THREADS")) t = atoi(e);
    t = std::min<int64_t>({t, 32, work_items / 65536 + 1});
    return (int)std::max<int64_t>(t, 1);
}

void shard_bounds(int64_t n_rows, const int64_t *row_ptr, int world, int rank, int64_t *lo, int64_t *hi) {
    const int64_t nnz = row_ptr[n_rows];
    // boundary of rank i: the row offset NEAREST to i/world of the stored nonzeros (so one giant row does
    // not drag every row before it into the same shard); datasets without nonzeros fall back to row counts
    auto bound = [&](int i) -> int64_t {
        if (i <= 0) return 0;
        if (i >= world) return n_rows;
        if (nnz == 0) return n_rows * i / world;
        const int64_t target = (int64_t)((__int128)nnz * i / world);
        int64_t r = std::lower_bound(row_ptr, row_ptr + n_rows + 1, target) - row_ptr;
        if (r > 0 && (r > n_rows || target - row_ptr[r - 1] < row_ptr[r] - target)) --r;
        return r;
    };
    *lo = std::min(bound(rank), n_rows);
    *hi = std::min(std::max(bound(rank + 1), *lo), n_rows);
}

int64_t feature_counts(int64_t nnz, const int32_t *col, int64_t n1, int64_t *counts) {
    const int T = host_threads(nnz);
    std::atomic<int64_t> bad{-1};
    // a private table per thread while that stays small (<= 64 MiB each), one shared table with atomic adds beyond
    const bool private_tables = T > 1 && n1 <= (int64_t)1 << 23;
    std::vector<std::vector<int64_t>> part(private_tables ? (size_t)T : 0);
    parallel_chunks(nnz, T, [&](int t, int64_t lo, int64_t hi) {
        int64_t *dst = counts;
        if (private_tables) {
            part[(size_t)t].assign((size_t)n1, 0);
            dst = part[(size_t)t].data();
        }
        for (int64_t i = lo; i < hi; ++i) {
            const int64_t c = col[i];
            if (c < 0 || c >= n1) { bad.store(i); return; }
            if (private_tables || T == 1) ++dst[c];
            else __atomic_fetch_add(&dst[c], (int64_t)1, __ATOMIC_RELAXED);
        }
    });
    if (bad.load() >= 0) return bad.load();
    if (private_tables)
        parallel_chunks(n1, T, [&](int, int64_t lo, int64_t hi) {
            for (int t = 0; t < T; ++t) {
                if (part[(size_t)t].empty()) continue;          // (a thread whose chunk was empty never made its table)
                const int64_t *src = part[(size_t)t].data();
                for (int64_t f = lo; f < hi; ++f) counts[f] += src[f];
            }
        });
    return -1;
}

void rank_from_counts(int64_t n1, const int64_t *counts, int32_t *rank, int32_t *by_rank) {
    std::vector<int32_t> order((size_t)n1);
    std::iota(order.begin(), order.end(), 0);
    // descending count, ties by ascending id: every rank of a job derives the same order from the same counts
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return counts[a] > counts[b]; });
    for (int64_t r = 0; r < n1; ++r) {
        rank[order[(size_t)r]] = (int32_t)r;
        if (by_rank) by_rank[r] = order[(size_t)r];
    }
}

int64_t relabel_columns(int64_t nnz, const int32_t *col, int64_t n1, const int32_t *rank, int32_t *out) {
    std::atomic<int64_t> bad{-1};
    parallel_chunks(nnz, host_threads(nnz), [&](int, int64_t lo, int64_t hi) {
        for (int64_t i = lo; i < hi; ++i) {
            const int64_t c = col[i];
            if (c < 0 || c >= n1) { bad.store(i); return; }
            out[i] = rank[c];
        }
    });
    return bad.load();
}

// ---- dataset build ------------------------------------------------------------------------------------------------

RowCheck validate_rows(int64_t n_rows, const int64_t *row_ptr, const int32_t *col, int threads) {
    RowCheck rc;
    std::vector<int64_t> bad((size_t)threads, -1);          // every thread's first finding: the first of them is the first of all
    std::vector<int32_t> mx((size_t)threads, 0);
    auto first_bad = [&]() {
        for (int64_t i : bad)
            if (i >= 0) return i;
        return (int64_t)-1;
    };
    parallel_chunks(n_rows, threads, [&](int t, int64_t lo, int64_t hi) {
        for (int64_t r = lo; r < hi; ++r)
            if (row_ptr[r + 1] < row_ptr[r]) { bad[(size_t)t] = r; break; }
    });
    if ((rc.bad_row = first_bad()) >= 0 || !col) return rc;
    parallel_chunks(row_ptr[n_rows], threads, [&](int t, int64_t lo, int64_t hi) {
        int32_t m = 0;
        for (int64_t p = lo; p < hi; ++p) {
            if (col[p] < 0) { bad[(size_t)t] = p; break; }
            m = std::max(m, col[p]);
        }
        mx[(size_t)t] = m;
    });
    rc.bad_entry = first_bad();
    rc.dim = *std::max_element(mx.begin(), mx.end());
    return rc;
}

int64_t validate_weights(int64_t n_rows, const double *weight, int threads) {
    if (threads < 1) threads = 1;
    std::vector<int64_t> bad((size_t)threads, -1);          // every thread's first finding: the first of them is the first of all
    parallel_chunks(n_rows, threads, [&](int t, int64_t lo, int64_t hi) {
        for (int64_t r = lo; r < hi; ++r)
            if (!(weight[r] >= 0.0 && weight[r] <= (double)FLT_MAX)) { bad[(size_t)t] = r; break; }      // (a NaN fails both)
    });
    for (int64_t r : bad)
        if (r >= 0) return r;
    return -1;
}

template <typename FT>
HotBlock choose_hot_block(int64_t n_rows, const int64_t *row_ptr, const int32_t *col, const FT *val, int32_t dim, int max_pages, bool row_blocked,
                          int threads, int64_t exact_nnz) {
    const int T = threads;
    const int64_t nnz = row_ptr[n_rows];
    // Frequencies: exact for datasets of up to exact_nnz (8 M) nonzeros; beyond that from every s-th row (the
    // choice of hot features is a layout decision — any set that passes the checks below is valid —
    // and a feature in >= 10 % of the rows cannot hide from a sample of millions of entries).
    const int64_t stride = nnz > exact_nnz ? std::max<int64_t>(1, nnz / std::max<int64_t>(exact_nnz / 2, 1)) : 1;
    const int64_t sampled_rows = (n_rows + stride - 1) / stride;
    std::vector<int32_t> cnt((size_t)dim + 1, 0);
    {
        // per-thread histograms while they stay small (<= 256 MB in all), merged in thread order; else one table, one thread
        const int Ts = ((int64_t)(dim + 1) * T * 4 <= ((int64_t)256 << 20)) ? std::min<int>(T, (int)std::max<int64_t>(sampled_rows / 4096, 1)) : 1;
        std::vector<std::vector<int32_t>> part((size_t)(Ts > 1 ? Ts : 0));
        parallel_chunks(sampled_rows, Ts, [&](int t, int64_t lo, int64_t hi) {
            int32_t *c = cnt.data();
            if (Ts > 1) { part[(size_t)t].assign((size_t)dim + 1, 0); c = part[(size_t)t].data(); }
            for (int64_t i = lo; i < hi; ++i) {
                const int64_t r = i * stride;
                for (int64_t p = row_ptr[r]; p < row_ptr[r + 1]; ++p) ++c[(size_t)col[p]];
            }
        });
        if (Ts > 1)
            parallel_chunks((int64_t)dim + 1, Ts, [&](int, int64_t lo, int64_t hi) {
                for (const auto &pc : part)
                    for (int64_t f = lo; f < hi; ++f) cnt[(size_t)f] += pc[(size_t)f];
            });
    }
    // candidates in descending order of frequency (ties: ascending id).  Page 0 is dense for the forward too, where a
    // slot costs every row a multiply-add chain: it takes features present in >= 10 % of the rows.  A gradient-side slot
    // costs a row 4 streamed bytes and saves, per entry, an 8-byte stream read, a P-row gather and an e gather (~2 line
    // requests of the texture path, which is what bounds the column walk): those pages take features down to 2.5 %.
    std::vector<int32_t> cand;
    for (int32_t f = 0; f <= dim; ++f)
        if ((int64_t)cnt[(size_t)f] * 40 >= sampled_rows) cand.push_back(f);
    std::sort(cand.begin(), cand.end(), [&](int32_t x, int32_t y) { return cnt[(size_t)x] != cnt[(size_t)y] ? cnt[(size_t)x] > cnt[(size_t)y] : x < y; });
    const size_t max_rest = (size_t)kHotT * (size_t)((row_blocked ? 1 : max_pages) - 1);
    HotBlock hb;
    hb.slot.assign((size_t)dim + 1, -1);
    hb.kept.assign((size_t)n_rows + 1, 0);
    std::vector<int8_t> &slot = hb.slot;
    // one sweep: the CSR length of every row if page 0 leaves the streams, and which candidates may not be
    // dense — one that occurs twice in a row, or is stored with an explicit zero (its G row must have exactly one
    // writer); if any is refused the sweep runs again without it (the ranking moves up)
    size_t used = 0, p0 = 0;   // candidates being tried: the first p0 in page 0 (slots 0..), the next ones in slots kHotT..
    auto slot_of = [&](size_t j) { return (int8_t)(j < p0 ? j : kHotT + (j - p0)); };
    for (;;) {
        p0 = 0;
        while (p0 < cand.size() && p0 < (size_t)kHotT && (int64_t)cnt[(size_t)cand[p0]] * 10 >= sampled_rows) ++p0;
        used = p0 < 2 ? 0 : p0 + std::min(cand.size() - p0, max_rest);
        if (!used) break;
        for (size_t j = 0; j < used; ++j) slot[(size_t)cand[j]] = slot_of(j);
        std::vector<slotmask_t> badv((size_t)T, 0u);
        parallel_chunks(n_rows, T, [&](int t, int64_t lo, int64_t hi) {
            slotmask_t bad = 0;
            for (int64_t r = lo; r < hi; ++r) {
                slotmask_t seen = 0;
                int64_t keep = 0;
                for (int64_t p = row_ptr[r]; p < row_ptr[r + 1]; ++p) {
                    const int8_t h = slot[(size_t)col[p]];
                    if (h < 0 || h >= kHotT) ++keep;
                    if (h < 0) continue;
                    if ((seen >> h & 1u) || (float)val[p] == 0.f) bad |= (slotmask_t)1 << h;
                    seen |= (slotmask_t)1 << h;
                }
                hb.kept[(size_t)r + 1] = keep;
            }
            badv[(size_t)t] = bad;
        });
        slotmask_t bad = 0;
        for (slotmask_t x : badv) bad |= x;
        if (!bad) break;
        std::vector<int32_t> ok;
        for (size_t j = 0; j < cand.size(); ++j) {
            if (j < used) slot[(size_t)cand[j]] = -1;
            if (j >= used || !(bad >> slot_of(j) & 1u)) ok.push_back(cand[j]);
        }
        cand.swap(ok);
    }
    if (!used) return hb;
    // slots in ascending feature order inside every page (the sweep above does not depend on the numbering)
    hb.p0 = p0;
    hb.pages = 1 + (int)((used - p0 + kHotT - 1) / kHotT);
    hb.hot_ids.assign((size_t)(hb.pages * kHotT), -1);
    std::sort(cand.begin(), cand.begin() + (std::ptrdiff_t)p0);
    for (size_t lo = p0; lo < used; lo += kHotT) std::sort(cand.begin() + (std::ptrdiff_t)lo, cand.begin() + (std::ptrdiff_t)std::min(used, lo + kHotT));
    for (size_t j = 0; j < used; ++j) {
        hb.hot_ids[(size_t)slot_of(j)] = cand[j];
        slot[(size_t)cand[j]] = slot_of(j);
    }
    return hb;
}
template HotBlock choose_hot_block<float>(int64_t, const int64_t *, const int32_t *, const float *, int32_t, int, bool, int, int64_t);
template HotBlock choose_hot_block<double>(int64_t, const int64_t *, const int32_t *, const double *, int32_t, int, bool, int, int64_t);

template <typename FT>
HotSplit split_hot_rows(int64_t n_rows, const int64_t *row_ptr, const int32_t *col, const FT *val, int32_t dim, int64_t batch_rows, HotBlock &hb,
                        int threads) {
    const int T = threads;
    const int64_t nb = n_rows > 0 ? (n_rows + batch_rows - 1) / batch_rows : 0;
    HotSplit s;
    if (hb.pages > 1) {
        s.drop_bits.assign((size_t)(dim + 1) / 32 + 2, 0u);
        for (size_t h = kHotT; h < hb.hot_ids.size(); ++h)
            if (hb.hot_ids[h] >= 0) s.drop_bits[(size_t)hb.hot_ids[h] >> 5] |= 1u << (hb.hot_ids[h] & 31);
    }
    s.hot_masks.assign((size_t)nb, 0u);
    s.bwd_out.assign((size_t)nb, 0);
    s.sp_ptr.swap(hb.kept);
    for (int64_t r = 0; r < n_rows; ++r) s.sp_ptr[(size_t)r + 1] += s.sp_ptr[(size_t)r];
    // fill (buffers left uninitialised: every element is written exactly once)
    s.sp_col.reset(new int32_t[(size_t)std::max<int64_t>(s.sp_ptr[(size_t)n_rows], 1)]);
    s.sp_val.reset(new float[(size_t)std::max<int64_t>(s.sp_ptr[(size_t)n_rows], 1)]);
    // page 0 is filled here (its entries leave the CSR stream); the gradient-side pages' entries STAY in the CSR stream,
    // so their pages are filled on the device from the uploaded stream (k_fill_hot_pages): 64 MB per page and million
    // rows that neither the host writes nor PCIe carries
    s.xhot0.reset(new float[(size_t)std::max<int64_t>(n_rows, 1) * kHotT]);
    const int64_t *sp_ptr = s.sp_ptr.data();
    const int8_t *slot = hb.slot.data();
    int32_t *sp_col = s.sp_col.get();
    float *sp_val = s.sp_val.get(), *xhot = s.xhot0.get();
    std::vector<std::vector<slotmask_t>> tmask((size_t)T, std::vector<slotmask_t>((size_t)nb, 0u));
    std::vector<std::vector<int64_t>> tout((size_t)T, std::vector<int64_t>((size_t)nb, 0));
    parallel_chunks(n_rows, T, [&](int t, int64_t lo, int64_t hi) {
        for (int64_t r = lo; r < hi; ++r) {
            slotmask_t seen = 0;
            int64_t o = sp_ptr[r], outb = 0;
            float *xr = xhot + (size_t)r * kHotT;
            for (int h = 0; h < kHotT; ++h) xr[h] = 0.f;
            for (int64_t p = row_ptr[r]; p < row_ptr[r + 1]; ++p) {
                const int8_t h = slot[(size_t)col[p]];
                if (h >= 0) {
                    seen |= (slotmask_t)1 << h;
                    if (h < kHotT) xr[h] = (float)val[p];
                }
                if (h < 0 || h >= kHotT) {
                    sp_col[(size_t)o] = col[p];
                    sp_val[(size_t)o] = (float)val[p];
                    ++o;
                    if (h >= 0) ++outb;
                }
            }
            tmask[(size_t)t][(size_t)(r / batch_rows)] |= seen;
            tout[(size_t)t][(size_t)(r / batch_rows)] += outb;
        }
    });
    for (int t = 0; t < T; ++t)
        for (int64_t b = 0; b < nb; ++b) {
            s.hot_masks[(size_t)b] |= tmask[(size_t)t][(size_t)b];
            s.bwd_out[(size_t)b] += tout[(size_t)t][(size_t)b];
        }
    return s;
}
template HotSplit split_hot_rows<float>(int64_t, const int64_t *, const int32_t *, const float *, int32_t, int64_t, HotBlock &, int);
template HotSplit split_hot_rows<double>(int64_t, const int64_t *, const int32_t *, const double *, int32_t, int64_t, HotBlock &, int);

std::vector<int32_t> forward_row_order(int64_t n_rows, int64_t batch_rows, const int64_t *row_ptr, int64_t window, int threads) {
    std::vector<int32_t> order((size_t)n_rows);
    const int64_t nb = n_rows > 0 ? (n_rows + batch_rows - 1) / batch_rows : 0;
    parallel_chunks(nb, std::min<int>(threads, (int)std::max<int64_t>(nb, 1)), [&](int, int64_t blo, int64_t bhi) {
        std::vector<int64_t> start;
        for (int64_t b = blo; b < bhi; ++b) {
            const int64_t row0 = b * batch_rows, rows = std::min(batch_rows, n_rows - row0);
            const int64_t win = window > 0 ? window : std::max<int64_t>(rows, 1);
            for (int64_t w0 = 0; w0 < rows; w0 += win) {
                const int64_t w1 = std::min(rows, w0 + win);
                int64_t maxlen = 0;
                for (int64_t r = w0; r < w1; ++r) maxlen = std::max(maxlen, row_ptr[row0 + r + 1] - row_ptr[row0 + r]);
                start.assign((size_t)maxlen + 2, 0);
                for (int64_t r = w0; r < w1; ++r) ++start[(size_t)(maxlen - (row_ptr[row0 + r + 1] - row_ptr[row0 + r])) + 1];
                for (size_t i = 1; i < start.size(); ++i) start[i] += start[i - 1];
                for (int64_t r = w0; r < w1; ++r) {
                    const size_t key = (size_t)(maxlen - (row_ptr[row0 + r + 1] - row_ptr[row0 + r]));
                    order[(size_t)(row0 + w0 + start[key]++)] = (int32_t)r;
                }
                // windows alternate longest-first / shortest-first: a workgroup takes the same position of every window it visits
                if (window > 0 && ((w0 / win) & 1)) std::reverse(order.begin() + (row0 + w0), order.begin() + (row0 + w1));
            }
        }
    });
    return order;
}

template <typename FT>
SortedRows sort_rows_by_feature(int64_t n_rows, const int64_t *row_ptr, const int32_t *col, const FT *val, int threads) {
    SortedRows s;
    s.scol.resize((size_t)row_ptr[n_rows]);
    s.sval.resize((size_t)row_ptr[n_rows]);
    std::vector<char> dupv((size_t)threads, 0);      // one byte per thread (vector<bool> packs bits: concurrent writes would race)
    parallel_chunks(n_rows, threads, [&](int t, int64_t lo, int64_t hi) {
        std::vector<int32_t> idx;
        bool dup = false;
        for (int64_t r = lo; r < hi; ++r) {
            const int64_t p0 = row_ptr[r], len = row_ptr[r + 1] - p0;
            idx.resize((size_t)len);
            std::iota(idx.begin(), idx.end(), 0);
            std::stable_sort(idx.begin(), idx.end(), [&](int32_t x, int32_t y) { return col[p0 + x] < col[p0 + y]; });   // equal ids keep their stored order
            for (int64_t j = 0; j < len; ++j) {
                s.scol[(size_t)(p0 + j)] = col[p0 + idx[(size_t)j]];
                s.sval[(size_t)(p0 + j)] = (double)val[p0 + idx[(size_t)j]];
                if (j && s.scol[(size_t)(p0 + j)] == s.scol[(size_t)(p0 + j - 1)]) dup = true;
            }
        }
        dupv[(size_t)t] = dup ? 1 : 0;
    });
    for (char b : dupv) s.dup = s.dup || b != 0;
    return s;
}
template SortedRows sort_rows_by_feature<float>(int64_t, const int64_t *, const int32_t *, const float *, int);
template SortedRows sort_rows_by_feature<double>(int64_t, const int64_t *, const int32_t *, const double *, int);

std::vector<uint32_t> own_bitmaps(const std::vector<HostBatch> &hbs, const std::vector<int32_t> &hot_ids, int32_t dim) {
    const size_t words = (size_t)dim / 32 + 1;
    std::vector<uint32_t> own(hbs.size() * words, 0u);
    for (size_t b = 0; b < hbs.size(); ++b) {
        uint32_t *bits = own.data() + b * words;
        const HostBatch &hb = hbs[b];
        for (const std::vector<int32_t> *lst : {&hb.split_seg, &hb.split_short})
            for (int32_t c : *lst) { const int32_t f = hb.cfeat[(size_t)c]; bits[f >> 5] |= 1u << (f & 31); }
        for (int32_t f : hot_ids)
            if (f >= 0) bits[f >> 5] |= 1u << (f & 31);
    }
    return own;
}

// Host-side metadata of one batch from its column offsets (the transposed stream itself is built
// on the device, csc_build.hip): the column open at the start of every 64-entry range and the
// columns whose sum is assembled by k_fixup.
void finish_batch_meta(HostBatch &hb, int32_t nnz, std::vector<int32_t> &cnt, std::vector<int32_t> &base) {
    const size_t nc = hb.cfeat.size();
    // destinations of the column pieces: a feature with one piece stores straight to its G row; a
    // feature with several (row-blocked stream) gets consecutive piece rows, in stream (= row block)
    // order, that k_fixup2 sums.  `cnt` / `base` are zeroed scratch arrays of dimension + 1 entries.
    {
        std::vector<int32_t> multi;
        hb.n_feats = 0;
        for (size_t s = 0; s < nc; ++s) {
            const int32_t c = ++cnt[hb.cfeat[s]];
            if (c == 1) ++hb.n_feats;
            if (c == 2) multi.push_back(hb.cfeat[s]);
        }
        std::sort(multi.begin(), multi.end());
        hb.mp_feat = multi;
        hb.mp_ptr.assign(multi.size() + 1, 0);
        for (size_t m = 0; m < multi.size(); ++m) {
            base[multi[m]] = hb.mp_ptr[m];
            hb.mp_ptr[m + 1] = hb.mp_ptr[m] + cnt[multi[m]];
        }
        hb.n_pieces = multi.empty() ? 0 : hb.mp_ptr[multi.size()];
        hb.cdst.resize(nc);
        for (size_t s = 0; s < nc; ++s) {
            const int32_t f = hb.cfeat[s];
            hb.cdst[s] = cnt[f] > 1 ? -1 - (base[f]++) : f;
        }
        for (size_t s = 0; s < nc; ++s) { cnt[hb.cfeat[s]] = 0; base[hb.cfeat[s]] = 0; }
    }
    const int32_t n_ranges = (int32_t)((nnz + kRangeLen - 1) / kRangeLen);
    hb.range_seg.assign((size_t)n_ranges, 0);
    size_t s = 0;
    for (int32_t rho = 0; rho < n_ranges; ++rho) {
        const int32_t pos = rho * kRangeLen;
        while (s + 1 < nc && hb.cptr[s + 1] <= pos) ++s;
        hb.range_seg[(size_t)rho] = (int32_t)s;
    }
    hb.split_seg.clear();
    hb.split_short.clear();
    // the same predicates k_backward applies: a column spanning two ranges whose remainder in the
    // second is <= kExtend is finished by the first range's slot and needs no fixup; the others are
    // summed by k_fixup, a slot each when they span <= 8 ranges, else a wave each
    for (size_t c = 0; c < nc; ++c) {
        const int32_t ra = hb.cptr[c] / kRangeLen, rb = (hb.cptr[c + 1] - 1) / kRangeLen;
        if (rb > ra && !(rb == ra + 1 && hb.cptr[c + 1] - rb * kRangeLen <= kExtend))
            (rb - ra + 1 <= 8 ? hb.split_short : hb.split_seg).push_back((int32_t)c);
    }
}

// cost of walking range rho (fmhip_host.h: kCostUnit per entry, kCloseCost per column that closes inside the range)
int64_t range_cost(const HostBatch &hb, int32_t cnnz, int32_t rho) {
    const int32_t n_ranges = (int32_t)hb.range_seg.size();
    const int32_t beg = rho * kRangeLen, end = std::min(beg + kRangeLen, cnnz);
    const int32_t nc = (int32_t)hb.cfeat.size();
    const int32_t closes = (rho + 1 < n_ranges ? hb.range_seg[(size_t)rho + 1] : nc) - hb.range_seg[(size_t)rho];
    return (int64_t)(end - beg) * kCostUnit + (int64_t)closes * kCloseCost;
}

int walk_order_default() {
    if (const char *ev = getenv("FMHIP_BWD_ORDER")) {           // measurement knob: 0 = stream order, 1 = cold first
        const int v = atoi(ev);
        if (v == kWalkOrderStream || v == kWalkOrderColdFirst) return v;
    }
    return kWalkOrderColdFirst;
}

// Band-affine placement of one batch's ranges (BwdArgs::xlist).  first/last: the rows of the first and last entry of every
// range.  A range that lies inside ONE column and spans at most a band and a half of rows is "affine" to the band of its
// middle row; XCD x owns a run of consecutive bands (two at 250k-row batches) and its list starts with their ranges, band by band,
// so that one band's slice of P (rows / 16 x 4 Kp bytes: 2 MB at 250k rows of Kp = 32) is what that XCD's L2 holds while
// they are walked; every other range is "free" and fills the lists up to equal length.  Returns the affine count.
//
// kWalkOrderColdFirst also gives every free range a COST, entries + 2.65 x (columns that close inside it) — a stretch of cold
// features, with a column close and a row store every entry or two, costs the walk up to 3.6 times a hot one per entry —
// and deals the free blocks, the most expensive first, to the list with the least accumulated cost (a band-affine range
// counts its entries).  walk[x] is then the order in which a WHOLE-BATCH launch walks list x: the free ranges in that
// order, then the band runs.  The launch used to END with its most expensive work on all eight XCDs at once — the lists
// closed with the coldest ranges of the stream — and a workgroup's wave slots are free only when its slowest wave is done;
// now its last round is the cheapest work there is (C3: backward 120.9 -> 115.4 us, C2 129.9 -> 120.0, C5's width 161.7 ->
// 146.1; profiles/bwd_dispatch.md).  lists / seg keep the interval form: the same ranges per XCD, every run ascending,
// which is what a feature-interval launch searches.
int32_t plan_bands(const HostBatch &hb, int32_t cnnz, int64_t rows, const std::vector<int32_t> &first, const std::vector<int32_t> &last,
                   std::vector<int32_t> (&lists)[kXcds], int32_t (&seg)[kXcds][kXSegs + 1], int order, std::vector<int32_t> (*walk)[kXcds]) {
    const int32_t n_ranges = (int32_t)hb.range_seg.size();
    // bands of about 16k rows (2 MB of P at Kp = 32, 4 MB at Kp = 64: C3 and C5's width measured the same with 16 and 32
    // bands of 250k rows), a multiple of the XCD count, at most 8 per XCD
    int n_bands = (int)std::min<int64_t>(((rows + 16383) / 16384 + kXcds - 1) / kXcds * kXcds, (kXSegs - 1) * kXcds);
    n_bands = std::max(n_bands, kRowBands);
    if (const char *ev = getenv("FMHIP_ROW_BANDS")) {           // measurement knob: a multiple of kXcds, at most 8 per XCD
        const int v = atoi(ev);
        if (v >= kXcds && v <= (kXSegs - 1) * kXcds && v % kXcds == 0) n_bands = v;
    }
    const int per_xcd = n_bands / kXcds;
    const int64_t band_rows = std::max<int64_t>((rows + n_bands - 1) / n_bands, 1);
    std::vector<std::vector<int32_t>> by_band((size_t)n_bands);
    std::vector<int32_t> free_ranges;
    for (int32_t rho = 0; rho < n_ranges; ++rho) {
        const int32_t beg = rho * kRangeLen, end = std::min(beg + kRangeLen, cnnz);
        const int32_t seg = hb.range_seg[(size_t)rho];
        const bool one_column = hb.cptr[(size_t)seg] <= beg && hb.cptr[(size_t)seg + 1] >= end;
        const int64_t span = (int64_t)last[(size_t)rho] - first[(size_t)rho];
        if (one_column && end - beg == kRangeLen && span >= 0 && span * 2 <= band_rows * 3) {
            const int64_t band = std::min<int64_t>(((int64_t)first[(size_t)rho] + last[(size_t)rho]) / 2 / band_rows, n_bands - 1);
            by_band[(size_t)band].push_back(rho);
        } else {
            free_ranges.push_back(rho);
        }
    }
    int32_t affine = 0;
    for (int x = 0; x < kXcds; ++x) {
        lists[x].clear();
        for (int b = 0; b < kXSegs - 1; ++b) {                     // one run per band (runs of bands the XCD does not have: empty)
            seg[x][b] = (int32_t)lists[x].size();
            if (b >= per_xcd) continue;
            const auto &v = by_band[(size_t)(x * per_xcd + b)];
            lists[x].insert(lists[x].end(), v.begin(), v.end());
            affine += (int32_t)v.size();
        }
        seg[x][kXSegs - 1] = (int32_t)lists[x].size();            // the last run: this XCD's share of the other ranges
    }
    // The free ranges follow in blocks of 32 consecutive ranges, each block to the list that is shortest so far: close to the
    // round-robin of the default placement — every XCD gets hot (few columns per range) and cold (a flush per entry)
    // stretches of the stream alike; handing each XCD one contiguous eighth instead left the XCD with the coldest
    // features far behind the others (C4: backward 203 -> 268 us) — and the lists end within a block of each other.
    constexpr size_t kBlockRanges = 32;
    if (order != kWalkOrderStream) {
        // by cost: the blocks (still 32 consecutive ranges each) sorted by descending cost, ties in stream order
        const size_t n_blocks = (free_ranges.size() + kBlockRanges - 1) / kBlockRanges;
        std::vector<int64_t> bcost(n_blocks, 0);
        for (size_t i = 0; i < free_ranges.size(); ++i) bcost[i / kBlockRanges] += range_cost(hb, cnnz, free_ranges[i]);
        std::vector<int32_t> by_cost(n_blocks);
        for (size_t i = 0; i < n_blocks; ++i) by_cost[i] = (int32_t)i;
        std::stable_sort(by_cost.begin(), by_cost.end(), [&](int32_t p, int32_t q) { return bcost[(size_t)p] > bcost[(size_t)q]; });
        int64_t acc[kXcds];
        std::vector<int32_t> freew[kXcds];                        // the free part of every list in walk order
        for (int x = 0; x < kXcds; ++x) acc[x] = (int64_t)lists[x].size() * kRangeLen * kCostUnit;   // band-affine ranges are full
        for (int32_t bi : by_cost) {
            int best = 0;
            for (int x = 1; x < kXcds; ++x)
                if (acc[x] < acc[best]) best = x;
            const size_t lo = (size_t)bi * kBlockRanges, hi = std::min(lo + kBlockRanges, free_ranges.size());
            freew[best].insert(freew[best].end(), free_ranges.begin() + (std::ptrdiff_t)lo, free_ranges.begin() + (std::ptrdiff_t)hi);
            acc[best] += bcost[(size_t)bi];
        }
        for (int x = 0; x < kXcds; ++x) {
            if (walk) {
                std::vector<int32_t> &wl = (*walk)[x];
                wl.clear();
                wl.insert(wl.end(), freew[x].begin(), freew[x].end());
                wl.insert(wl.end(), lists[x].begin(), lists[x].end());
            }
            std::sort(freew[x].begin(), freew[x].end());          // the interval form's last run ascends
            lists[x].insert(lists[x].end(), freew[x].begin(), freew[x].end());
            seg[x][kXSegs] = (int32_t)lists[x].size();
        }
        return affine;
    }
    for (size_t next = 0; next < free_ranges.size(); next += kBlockRanges) {
        int best = 0;
        for (int x = 1; x < kXcds; ++x)
            if (lists[x].size() < lists[best].size()) best = x;
        const size_t hi = std::min(next + kBlockRanges, free_ranges.size());
        lists[best].insert(lists[best].end(), free_ranges.begin() + (std::ptrdiff_t)next, free_ranges.begin() + (std::ptrdiff_t)hi);
    }
    for (int x = 0; x < kXcds; ++x) {
        seg[x][kXSegs] = (int32_t)lists[x].size();
        if (walk) (*walk)[x] = lists[x];                          // stream order: the interval form is the walk order
    }
    return affine;
}

// ALS level schedule (S/fm/lib/ALS.scala:36-70 walks the features in id order; two columns without a common row touch
// disjoint residuals and q entries, so their closed-form steps commute EXACTLY): one pass over the transpose in id order,
// level(c) = 1 + max over c's rows of the level of the last column that touched the row
int32_t als_levels(const std::vector<int32_t> &cptr, const uint32_t *crow, int64_t rows, std::vector<int32_t> &lev_ptr, std::vector<int32_t> &cols) {
    const size_t nc = cptr.empty() ? 0 : cptr.size() - 1;
    std::vector<int32_t> row_level((size_t)std::max<int64_t>(rows, 0), 0), level(nc, 0);
    int32_t n_levels = 0;
    for (size_t c = 0; c < nc; ++c) {
        int32_t lv = 0;
        for (int32_t p = cptr[c]; p < cptr[c + 1]; ++p) lv = std::max(lv, row_level[crow[(size_t)p] & 0x7fffffffu]);
        ++lv;
        level[c] = lv;
        n_levels = std::max(n_levels, lv);
        for (int32_t p = cptr[c]; p < cptr[c + 1]; ++p) row_level[crow[(size_t)p] & 0x7fffffffu] = lv;
    }
    lev_ptr.assign((size_t)n_levels + 1, 0);
    for (size_t c = 0; c < nc; ++c) ++lev_ptr[(size_t)level[c]];
    for (int32_t l = 1; l <= n_levels; ++l) lev_ptr[(size_t)l] += lev_ptr[(size_t)l - 1];
    cols.assign(nc, 0);
    std::vector<int32_t> at(lev_ptr.begin(), lev_ptr.end() - 1);
    for (size_t c = 0; c < nc; ++c) cols[(size_t)at[(size_t)level[c] - 1]++] = (int32_t)c;   // ascending id inside a level
    return n_levels;
}

void choose_cuts(const int32_t *cnt, int64_t n1, int n_fractions, const double *fractions, int64_t *cuts) {
    int64_t total = 0;
    for (int64_t f = 0; f < n1; ++f) total += cnt[f];
    int64_t above = 0, f = n1 - 1;
    for (int i = 0; i < n_fractions; ++i) {
        const double want = std::min(std::max(fractions[i], 0.0), 1.0) * (double)total;
        while (f > 0 && (double)above < want) above += cnt[(size_t)f--];
        cuts[i] = f + 1 < n1 ? f + 1 : 0;
    }
}

std::vector<int64_t> interval_edges(const std::vector<int64_t> &cuts, int64_t n1, int W) {
    std::vector<int64_t> edge{0};
    for (int64_t x : cuts) {
        const int64_t xr = W > 0 ? x / W * W : x;           // the plan rounds already; a plan made for another world may not have
        if (xr > edge.back() && xr < n1) edge.push_back(xr);
    }
    edge.push_back(n1);
    return edge;
}

Share shard_share(int64_t lo, int64_t hi, bool top_interval, int64_t n1, int W, int R) {
    Share s;
    s.hi_r = top_interval ? shard_top(n1, W) : hi;           // the top interval reaches into the slack rows
    s.chunk = (s.hi_r - lo) / W;
    s.vlo = lo + (int64_t)R * s.chunk;
    s.vhi = s.vlo + s.chunk;
    return s;
}

CompactEdges compact_edges(const std::vector<int64_t> &cuts, int64_t n1, const int32_t *cut_pos, int32_t n_u) {
    CompactEdges c{{0}, {0}};
    for (size_t i = 0; i < cuts.size(); ++i) {
        if (cuts[i] > c.edge.back() && cuts[i] < n1) {
            c.edge.push_back(cuts[i]);
            c.pe.push_back(cut_pos[i]);
        }
    }
    c.edge.push_back(n1);
    c.pe.push_back(n_u);
    return c;
}

std::vector<ApplyGroup> apply_groups(const std::vector<int64_t> &edges, int64_t total_rows, int first_interval) {
    std::vector<ApplyGroup> g;
    int64_t pend_hi = -1;      // the top of the rows waiting for a launch (-1: none)
    for (int i = first_interval; i >= 0; --i) {
        const int64_t lo = edges[(size_t)i];
        if (pend_hi < 0) pend_hi = edges[(size_t)i + 1];
        if (i > 0 && (pend_hi - lo) * 8 < total_rows) continue;
        g.push_back({i, lo, pend_hi});
        pend_hi = -1;
    }
    return g;
}

// ---- the split step's backward window -----------------------------------------------------------------------------------
BwVerdict bw_window_step(BwWindow w, int64_t n1, int64_t lo, int64_t hi, bool finish) {
    auto refuse = [&](BwRefusal why, int64_t want, int64_t got) { return BwVerdict{why, want, got, 0, w}; };
    if (w.closed()) return refuse(BwRefusal::kClosed, 0, 0);
    if (finish && lo != 0) return refuse(BwRefusal::kFinishAboveZero, 0, 0);
    const bool fresh = w.next == INT64_MAX;
    if (fresh ? hi < n1 && lo == 0 : w.up) {
        const int64_t want = fresh ? 0 : w.next;
        if (lo != want) return refuse(BwRefusal::kNotAscending, want, lo);
        return BwVerdict{BwRefusal::kNone, 0, 0, kOwnUpper, BwWindow{hi >= n1 ? -1 : hi, true}};
    }
    if (fresh ? hi < n1 : hi != w.next) return refuse(BwRefusal::kNotDescending, fresh ? n1 : w.next, hi);
    return BwVerdict{BwRefusal::kNone, 0, 0, kOwnLower, BwWindow{lo == 0 ? -1 : lo, false}};
}

std::string bw_refusal_text(const BwVerdict &v) {
    char buf[200] = "";
    switch (v.refusal) {
        case BwRefusal::kNone: break;
        case BwRefusal::kClosed: return "fmhip_step_backward without fmhip_step_forward";
        case BwRefusal::kFinishAboveZero: return "finish = 1 belongs to the interval that starts at feature 0";
        case BwRefusal::kNotAscending:
            snprintf(buf, sizeof buf, "feature intervals must tile [0, n+1) in ascending order (expected lo = %lld, got %lld)", (long long)v.want,
                     (long long)v.got);
            break;
        case BwRefusal::kNotDescending:
            snprintf(buf, sizeof buf, "feature intervals must tile [0, n+1) in descending order (expected hi = %lld, got %lld), or start at feature 0 and ascend",
                     (long long)v.want, (long long)v.got);
            break;
    }
    return buf;
}

// HitRate / Recall / Precision / NDCG at k, MRR and MAP of the ranks fmhip_rank returns (include/fmhip_ranking.h states each).
// A context's ranks are sorted first: MAP needs them ascending, and equal neighbours are then the duplicates to refuse.
int64_t rank_metrics(int64_t n_contexts, const int64_t *rel_ptr, const int32_t *rank, int32_t k, RankMetricSums *out) {
    RankMetricSums s;
    std::vector<int32_t> r;
    for (int64_t c = 0; c < n_contexts; ++c) {
        const int64_t n = rel_ptr[c + 1] - rel_ptr[c];
        if (n == 0) {
            ++s.skipped;
            continue;
        }
        r.assign(rank + rel_ptr[c], rank + rel_ptr[c + 1]);
        std::sort(r.begin(), r.end());
        if (r[0] < 0) return c;
        for (int64_t j = 1; j < n; ++j)
            if (r[(size_t)j] == r[(size_t)j - 1]) return c;
        ++s.contexts;
        s.relevant += n;
        int64_t hits = 0;
        double dcg = 0.0, idcg = 0.0, ap = 0.0;
        for (int64_t j = 0; j < n; ++j) {
            if (r[(size_t)j] < k) {
                ++hits;
                dcg += 1.0 / log2((double)r[(size_t)j] + 2.0);
            }
            if (j < k) idcg += 1.0 / log2((double)j + 2.0);
            ap += (double)(j + 1) / ((double)r[(size_t)j] + 1.0);
        }
        s.hit_rate += hits > 0 ? 1.0 : 0.0;
        s.recall += (double)hits / (double)n;
        s.precision += (double)hits / (double)k;
        s.ndcg += dcg / idcg;
        s.mrr += 1.0 / ((double)r[0] + 1.0);
        s.map += ap / (double)n;
    }
    if (s.contexts > 0) {
        const double n = (double)s.contexts;
        s.hit_rate /= n;
        s.recall /= n;
        s.precision /= n;
        s.ndcg /= n;
        s.mrr /= n;
        s.map /= n;
    }
    *out = s;
    return -1;
}

// ---- relational data (include/fmhip_relational.h) ---------------------------------------------------------------------

int64_t relational_bad_mapping(int64_t n_rows, const int32_t *map, int64_t block_rows) {
    for (int64_t r = 0; r < n_rows; ++r)
        if (map[r] < 0 || (int64_t)map[r] >= block_rows) return r;
    return -1;
}

SharedFeature first_shared_feature(int n_parts, const int32_t *const *feat, const int64_t *n_feat, int64_t dimension) {
    SharedFeature best;
    std::vector<int32_t> owner((size_t)std::max<int64_t>(dimension, 0) + 1, -1);
    for (int p = 0; p < n_parts; ++p)
        for (int64_t i = 0; i < n_feat[p]; ++i) {
            const int32_t f = feat[p][i];
            if (f < 0 || (int64_t)f > dimension) continue;        // (an unused slot of a hot block's id list)
            int32_t &o = owner[(size_t)f];
            if (o < 0) o = p;
            else if (o != p && (best.feature < 0 || f < best.feature || (f == best.feature && p < best.b))) best = SharedFeature{f, o, p};
        }
    return best;
}

void RelationInverse::append_batch(const int32_t *map, int64_t rows, int64_t block_rows, int32_t cut, std::vector<int32_t> &count) {
    if (count.size() < (size_t)block_rows) count.assign((size_t)block_rows, 0);
    Batch b;
    b.row_off = (int64_t)trow.size();
    b.t_off = (int64_t)tj.size();
    b.tptr_off = (int64_t)tptr.size();
    b.w_off = (int64_t)wt.size();
    b.l_off = (int64_t)lt.size();
    // counting sort of the batch's rows by block row: the counts, the touched block rows ascending, their offsets, the placement
    for (int64_t r = 0; r < rows; ++r)
        if (count[(size_t)map[r]]++ == 0) tj.push_back(map[r]);
    std::sort(tj.begin() + b.t_off, tj.end());
    b.n_touched = (int32_t)((int64_t)tj.size() - b.t_off);
    int32_t at = 0;
    for (int32_t t = 0; t < b.n_touched; ++t) {
        int32_t &c = count[(size_t)tj[(size_t)(b.t_off + t)]];
        const int32_t len = c;
        tptr.push_back(at);
        // the list's work: one item that writes the block row, or ceil(len / cut) chunks into partial rows + one second-pass item
        if (len <= cut) {
            wt.push_back(t); wbeg.push_back(at); wdst.push_back(tj[(size_t)(b.t_off + t)]);
        } else {
            lt.push_back(t); lfirst.push_back(b.n_part); lcount.push_back((len + cut - 1) / cut);
            for (int32_t o = 0; o < len; o += cut) { wt.push_back(t); wbeg.push_back(at + o); wdst.push_back(-1 - b.n_part++); }
        }
        c = at;              // the count becomes the list's cursor
        at += len;
    }
    tptr.push_back(at);
    trow.resize((size_t)(b.row_off + rows));
    for (int64_t r = 0; r < rows; ++r) trow[(size_t)(b.row_off + count[(size_t)map[r]]++)] = (int32_t)r;     // ascending inside a list
    for (int32_t t = 0; t < b.n_touched; ++t) count[(size_t)tj[(size_t)(b.t_off + t)]] = 0;                 // the scratch is left zeroed
    b.n_work = (int32_t)((int64_t)wt.size() - b.w_off);
    b.n_long = (int32_t)((int64_t)lt.size() - b.l_off);
    max_part = std::max(max_part, b.n_part);
    batches.push_back(b);
}

// ---- the BPR trainer (include/fmhip_bpr.h) ------------------------------------------------------------------------------

void bpr_positive_lists(int64_t n_ctx, int64_t n_inter, const int32_t *inter_ctx, const int32_t *inter_cand, std::vector<int64_t> &ptr,
                        std::vector<int32_t> &rows) {
    // counting sort by context, every list sorted, its repeats dropped, the lists closed up
    std::vector<int64_t> at((size_t)n_ctx + 1, 0);
    for (int64_t i = 0; i < n_inter; ++i) ++at[(size_t)inter_ctx[i] + 1];
    for (int64_t u = 0; u < n_ctx; ++u) at[(size_t)u + 1] += at[(size_t)u];
    std::vector<int32_t> all((size_t)n_inter);
    {
        std::vector<int64_t> cur(at.begin(), at.end() - 1);
        for (int64_t i = 0; i < n_inter; ++i) all[(size_t)cur[(size_t)inter_ctx[i]]++] = inter_cand[i];
    }
    ptr.assign((size_t)n_ctx + 1, 0);
    rows.clear();
    rows.reserve((size_t)n_inter);
    for (int64_t u = 0; u < n_ctx; ++u) {
        auto lo = all.begin() + at[(size_t)u], hi = all.begin() + at[(size_t)u + 1];
        std::sort(lo, hi);
        hi = std::unique(lo, hi);
        rows.insert(rows.end(), lo, hi);
        ptr[(size_t)u + 1] = (int64_t)rows.size();
    }
}

int32_t bpr_candidate(uint64_t seed, uint32_t p, uint32_t c, uint32_t t, int32_t M, const int32_t *list, int32_t len, int *attempts, int *forced) {
    int a = 0, f = 0;
    const int32_t row = rng::negative_row(seed, p, t, (uint32_t)M, list, len, &a, &f, c << 4);
    if (attempts) *attempts = a;
    if (forced) *forced = f;
    return row;
}

int32_t bpr_negative(uint64_t seed, uint32_t p, uint32_t t, int32_t M, const int32_t *list, int32_t len, int *attempts, int *forced) {
    return bpr_candidate(seed, p, 0, t, M, list, len, attempts, forced);
}

int64_t bpr_alias_table(int64_t M, const double *weights, rng::AliasEntry *out) {
    for (int64_t i = 0; i < M; ++i)
        if (!(weights[i] > 0.0) || !std::isfinite(weights[i])) return i;
    double sum = 0.0;
    for (int64_t i = 0; i < M; ++i) sum += weights[i];
    if (!std::isfinite(sum)) return -2;
    std::vector<double> q((size_t)M);
    std::vector<int32_t> small, large;
    for (int64_t i = 0; i < M; ++i) {
        q[(size_t)i] = weights[i] / sum * (double)M;
        (q[(size_t)i] < 1.0 ? small : large).push_back((int32_t)i);
    }
    for (int64_t i = 0; i < M; ++i) out[i] = rng::AliasEntry{0xffffffffu, (int32_t)i};
    while (!small.empty() && !large.empty()) {
        const int32_t l = small.back(), g = large.back();
        small.pop_back();
        large.pop_back();
        const double scaled = floor(q[(size_t)l] * 4294967296.0);
        out[l] = rng::AliasEntry{scaled >= 4294967295.0 ? 0xffffffffu : (uint32_t)scaled, g};
        q[(size_t)g] = (q[(size_t)g] + q[(size_t)l]) - 1.0;
        (q[(size_t)g] < 1.0 ? small : large).push_back(g);
    }
    return -1;
}

void bpr_log_proposal(int64_t M, const double *weights, float *out) {
    double sum = 0.0;
    for (int64_t i = 0; i < M; ++i) sum += weights[i];
    for (int64_t i = 0; i < M; ++i) {
        const double r = weights[i] / sum;
        out[i] = (float)(r > 0.0 ? log(r) : log(weights[i]) - log(sum));      // (a quotient that underflows: still finite)
    }
}

int32_t bpr_proposal_candidate(uint64_t seed, uint32_t p, uint32_t c, uint32_t t, int32_t M, const rng::AliasEntry *tab, const int32_t *list,
                               int32_t len, int *attempts, int *forced) {
    int a = 0, f = 0;
    const int32_t row = rng::proposal_row(seed, p, t, (uint32_t)M, tab, list, len, &a, &f, c << 4);
    if (attempts) *attempts = a;
    if (forced) *forced = f;
    return row;
}

void warp_weight_table(int64_t M, int C, float *out) {
    out[0] = 0.f;
    double h = 0.0;
    int64_t j = 0;
    for (int n = C; n >= 1; --n) {      // (M - 1) / n grows as n falls: the sum runs on from where it stood
        const int64_t r = std::max<int64_t>(1, (M - 1) / n);
        while (j < r) h += 1.0 / (double)++j;
        out[n] = (float)h;
    }
}

int warp_first_violator(const float *scores, int C, float s_pos, float margin) {
    const float thr = s_pos - margin;
    for (int c = 0; c < C; ++c)
        if (scores[c] > thr) return c + 1;
    return 0;
}

// ---- the MCMC learner's draws -------------------------------------------------------------------------------------------

double mcmc_uniform(uint64_t seed, uint32_t index, uint32_t group, uint32_t t, uint32_t stream) { return rng::uniform(seed, index, group, t, stream); }
double mcmc_normal(uint64_t seed, uint32_t index, uint32_t group, uint32_t t, uint32_t stream) { return rng::normal(seed, index, group, t, stream); }

double mcmc_gamma(uint64_t seed, uint32_t group, uint32_t t, uint32_t stream, double shape, double rate, int *attempts) {
    const bool boost = shape < 1.0;
    const double a = boost ? shape + 1.0 : shape;
    const double d = a - 1.0 / 3.0, c = 1.0 / sqrt(9.0 * d);
    double out = a / rate;                  // (never reached: an attempt is accepted with probability > 0.95)
    int j = 0;
    for (; j < (1 << 20); ++j) {
        const double x = rng::normal(seed, 2u * (uint32_t)j, group, t, stream), u = rng::uniform(seed, 2u * (uint32_t)j + 1u, group, t, stream);
        double v = 1.0 + c * x;
        v = v * v * v;
        if (v <= 0.0) continue;
        if (log(u) < x * x / 2.0 + d - d * v + d * log(v)) {
            out = d * v / rate;
            ++j;
            break;
        }
    }
    if (attempts) *attempts = j;
    if (boost) out *= pow(rng::uniform(seed, 0xffffffffu, group, t, stream), 1.0 / shape);
    return out;
}

const char *mcmc_bad_setting(const McmcPriors &p, double reg0, double init_lambda) {
    auto pos = [](double x) { return std::isfinite(x) && x > 0.0; };
    if (!pos(p.alpha_0)) return "alpha_0";
    if (!pos(p.beta_0)) return "beta_0";
    if (!pos(p.alpha_lambda)) return "alpha_lambda";
    if (!pos(p.beta_lambda)) return "beta_lambda";
    if (!pos(p.gamma_0)) return "gamma_0";
    if (!std::isfinite(p.mu_0)) return "mu_0";
    if (!(std::isfinite(reg0) && reg0 >= 0.0)) return "reg0";
    if (!pos(init_lambda)) return "init_lambda";
    return nullptr;
}

double mcmc_draw_alpha(uint64_t seed, uint32_t t, const McmcPriors &p, int64_t n_rows, double sse) {
    return mcmc_gamma(seed, 0, t, rng::kStreamAlpha, (p.alpha_0 + (double)n_rows) / 2.0, (p.beta_0 + sse) / 2.0, nullptr);
}

void mcmc_draw_group(uint64_t seed, uint32_t t, uint32_t g, const McmcPriors &p, int64_t m, double sum_theta, double sum_dev2, double mu_old,
                     double *lambda, double *mu) {
    const double dm = mu_old - p.mu_0;
    *lambda = mcmc_gamma(seed, g, t, rng::kStreamLambda, (p.alpha_lambda + (double)m + 1.0) / 2.0, (p.beta_lambda + sum_dev2 + p.gamma_0 * (dm * dm)) / 2.0,
                         nullptr);
    const double w = (double)m + p.gamma_0;
    *mu = (sum_theta + p.gamma_0 * p.mu_0) / w + rng::normal(seed, 0, g, t, rng::kStreamMu) / sqrt(w * *lambda);
}

int64_t mcmc_bad_group(const int32_t *group, int64_t n, int32_t n_groups) {
    for (int64_t i = 0; i < n; ++i)
        if (group[i] < 0 || group[i] >= n_groups) return i;
    return -1;
}

void mcmc_group_plan(const int32_t *cfeat, int64_t n_cols, int64_t num_attribute, const int32_t *group, int32_t n_groups, int chunk_slots,
                     McmcGroupPlan *plan) {
    const size_t G = (size_t)n_groups;
    plan->counts.assign(G, 0);
    for (int64_t s = 0; s < n_cols; ++s)
        if (cfeat[s] < num_attribute) ++plan->counts[(size_t)group[cfeat[s]]];
    // a counting sort: stable, so a group's slots stay ascending
    std::vector<int64_t> at(G + 1, 0);
    for (size_t a = 0; a < G; ++a) at[a + 1] = at[a] + plan->counts[a];
    plan->order.assign((size_t)at[G], 0);
    plan->chunk_ptr.assign(1, 0);
    plan->chunk_group.clear();
    plan->group_chunks.assign(G + 1, 0);
    for (size_t a = 0; a < G; ++a) {
        for (int64_t lo = at[a]; lo < at[a + 1]; lo += chunk_slots) {
            plan->chunk_group.push_back((int32_t)a);
            plan->chunk_ptr.push_back((int32_t)std::min<int64_t>(lo + chunk_slots, at[a + 1]));
        }
        plan->group_chunks[a + 1] = (int32_t)plan->chunk_group.size();
    }
    for (int64_t s = 0; s < n_cols; ++s)
        if (cfeat[s] < num_attribute) plan->order[(size_t)at[(size_t)group[cfeat[s]]]++] = (int32_t)s;
}

void sgda_group_plan(const int32_t *group, int64_t n, int32_t n_groups, int chunk_rows, McmcGroupPlan *plan) {
    std::vector<int32_t> ids((size_t)n);
    std::iota(ids.begin(), ids.end(), 0);       // every row is a slot of its own, all of them trained
    mcmc_group_plan(ids.data(), n, n, group, n_groups, chunk_rows, plan);
}

double mcmc_truncated_normal(uint64_t seed, uint32_t row, uint32_t t, double a, int *attempts) { return rng::truncated_normal(seed, row, t, a, attempts); }
double mcmc_truncated_mean(double a) { return rng::truncated_normal_mean(a); }

const char *mcmc_bad_task(int32_t task, int32_t clip, double clip_lo, double clip_hi) {
    if (task != 0 && task != 1) return "unknown task (FMHIP_MCMC_REGRESSION = 0, FMHIP_MCMC_CLASSIFICATION = 1)";
    if (!clip) return nullptr;
    if (task == 1) return "clip goes with the regression task: a classification handle's predictions are probabilities";
    if (!(std::isfinite(clip_lo) && std::isfinite(clip_hi) && clip_lo < clip_hi)) return "the clip range must be finite with clip_lo < clip_hi";
    return nullptr;
}

// ---- ... its block-structure sweep (include/fmhip_mcmc_relational.h) ------------------------------------------------------

McmcPartOrder mcmc_part_order(int n_parts, const int32_t *const *feat, const int64_t *n_feat) {
    McmcPartOrder out;
    std::vector<int32_t> lo((size_t)n_parts, INT32_MAX), hi((size_t)n_parts, -1);
    for (int p = 0; p < n_parts; ++p)
        for (int64_t x = 0; x < n_feat[p]; ++x) {
            lo[(size_t)p] = std::min(lo[(size_t)p], feat[p][x]);
            hi[(size_t)p] = std::max(hi[(size_t)p], feat[p][x]);
        }
    out.order.resize((size_t)n_parts);
    for (int p = 0; p < n_parts; ++p) out.order[(size_t)p] = p;
    // (a part without features sorts last: nothing of it is walked)
    std::stable_sort(out.order.begin(), out.order.end(), [&](int x, int y) { return lo[(size_t)x] < lo[(size_t)y]; });
    for (int x = 0; x + 1 < n_parts; ++x) {
        const int a = out.order[(size_t)x], b = out.order[(size_t)x + 1];
        if (hi[(size_t)b] < 0) break;
        if (lo[(size_t)b] <= hi[(size_t)a]) {
            out.a = a;
            out.b = b;
            out.feature = lo[(size_t)b];
            break;
        }
    }
    return out;
}

void mcmc_block_counts(const int32_t *map, int64_t n_rows, int64_t block_rows, std::vector<double> &n) {
    n.assign((size_t)block_rows, 0.0);
    for (int64_t r = 0; r < n_rows; ++r) n[(size_t)map[r]] += 1.0;
}

int64_t mcmc_block_trained(const int32_t *cfeat, const int32_t *cptr, const uint32_t *crow, int64_t n_cols, int64_t num_attribute, const double *n,
                           std::vector<int32_t> &trained) {
    trained.assign((size_t)n_cols, 0);
    int64_t count = 0;
    for (int64_t s = 0; s < n_cols; ++s) {
        if (cfeat[s] >= num_attribute) continue;
        bool used = false;
        for (int32_t p = cptr[s]; p < cptr[s + 1] && !used; ++p) used = !n || n[crow[p] & 0x7fffffffu] > 0.0;
        trained[(size_t)s] = used ? 1 : 0;
        count += used;
    }
    return count;
}

}  // namespace host
}  // namespace fmhip
