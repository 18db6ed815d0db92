// fmhip_dataset.hip — `DataSet(rdd).cache()` + `transposeInput` (S/DataSet.scala:42-62, 31-38) behind the C ABI:
// fmhip_dataset_create as a sequence of phases — its pure host passes (validation, the dense hot block's choice and split, forward
// row order, ALS row sort, own bitmaps) live in fmhip_host.cpp, what calls HIP (uploads, the per-batch device transposes of
// csc_build.hip with their column index) here — and the dataset entry points of include/fmhip.h.  The step that consumes all
// this: fmhip_step.hip.
#include "fmhip_internal.h"
#include "../../include/fmhip_weights.h"
#include "csc_build.h"

#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <memory>
#include <new>
#include <type_traits>
#include <vector>

using namespace fmhip;
using namespace fmhip::host;

static_assert(FMHIP_HOT_PAGES == kHotPages, "header and kernels disagree on the hot pages");
static_assert(FMHIP_RANGE_LEN == kRangeLen, "header and kernels disagree on the CSC range length");

namespace fmhip {
namespace host {

// ---- dataset construction -------------------------------------------------------

template <typename T>
int upload(DevBuf<T> &dst, const T *src, size_t n) {
    TRY(dst.alloc(n));
    if (n) HIP_TRY(hipMemcpy(dst.p, src, n * sizeof(T), hipMemcpyHostToDevice));
    return FMHIP_OK;
}

// FMHIP_BUILD_TIMING=1: the phases of fmhip_dataset_create on stderr (what `DataSet.cache()` costs, and where)
struct PhaseTimer {
    bool on;
    std::chrono::steady_clock::time_point t;
    PhaseTimer() : on(getenv("FMHIP_BUILD_TIMING") != nullptr), t(std::chrono::steady_clock::now()) {}
    void lap(const char *what) {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[fmhip build] %-28s %8.1f ms\n", what, std::chrono::duration<double, std::milli>(now - t).count());
        t = now;
    }
};

// The gradient-side pages of the dense hot block, filled on the device from the CSR stream that was just uploaded (their
// entries stay in it): 8 lanes per row walk the row's entries, an entry whose feature sits in slot h >= kHotT of the id table
// (ascending inside a page: a binary search per page) stores its value to xhot[page][row][h % kHotT].  One writer per
// element: a feature chosen for the block occurs at most once per row.
__global__ __launch_bounds__(256) void k_fill_hot_pages(const int64_t *row_ptr, const int32_t *col, const float *val, int64_t n_rows,
                                                        const int32_t *hot_ids, int pages, float *xhot, int64_t page_floats) {
    __shared__ int32_t ids[kHotPages * kHotT];
    for (int i = threadIdx.x; i < pages * kHotT; i += 256) ids[i] = hot_ids[i];
    __syncthreads();
    const int64_t r = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 3;
    const int l = threadIdx.x & 7;
    if (r >= n_rows) return;
    for (int64_t p = row_ptr[r] + l; p < row_ptr[r + 1]; p += 8) {
        const int32_t c = col[p];
        for (int pg = 1; pg < pages; ++pg) {
            const int32_t *t = ids + pg * kHotT;
            // the page's live slots come first, ascending; unused slots are -1
            int n = 0;
            while (n < kHotT && t[n] >= 0) ++n;
            if (n == 0 || c < t[0] || c > t[n - 1]) continue;
            int lo = 0, hi = n;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (t[mid] < c) lo = mid + 1;
                else hi = mid;
            }
            if (lo < n && t[lo] == c) xhot[(size_t)pg * page_floats + (size_t)r * kHotT + lo] = val[p];
        }
    }
}

// ---- the phases of dataset_create_impl that call HIP -------------------------------------------------------------

// the batch table: each batch's rows and its slices of the CSR stream (row_ptr; orig_row_ptr = the caller's) and of the transposes
int batch_table(fmhip_dataset &d, const int64_t *row_ptr, const int64_t *orig_row_ptr, const HotSplit *sp) {
    const int64_t nb = d.n_rows > 0 ? (d.n_rows + d.batch_rows - 1) / d.batch_rows : 0;
    d.nnz_sparse = row_ptr[d.n_rows];
    d.batches.resize((size_t)nb);
    for (int64_t b = 0; b < nb; ++b) {
        BatchMeta &bm = d.batches[(size_t)b];
        bm.row0 = b * d.batch_rows;
        bm.rows = std::min(d.batch_rows, d.n_rows - bm.row0);
        bm.nnz0 = row_ptr[bm.row0];
        bm.nnz_total = orig_row_ptr[bm.row0 + bm.rows] - orig_row_ptr[bm.row0];
        bm.hot_mask = sp ? sp->hot_masks[(size_t)b] : 0u;
        const int64_t bn = row_ptr[bm.row0 + bm.rows] - bm.nnz0, cn = bn - (sp ? sp->bwd_out[(size_t)b] : 0);
        d.nnz_sparse_bwd += cn;
        if (bn > (int64_t)0x7fffffff - 2 * kRangeLen || bm.rows > 0x7fffffff)
            return fail(FMHIP_ERR_UNSUPPORTED, "batch %lld holds %lld nonzeros; the per-batch limit is 2^31", (long long)b, (long long)bn);
        bm.nnz = (int32_t)bn;
        bm.cnnz = (int32_t)cn;
        d.max_rows = std::max(d.max_rows, bm.rows);
    }
    return FMHIP_OK;
}

// page 0 of the dense hot block from the host; pages 1.. zeroed and filled on the device from the uploaded CSR stream (a block has rows)
int upload_hot_pages(fmhip_dataset &d, const float *xhot0) {
    const size_t page_floats = (size_t)std::max<int64_t>(d.n_rows, 1) * kHotT;
    hipError_t he = hipMemcpy(d.xhot.p, xhot0, page_floats * sizeof(float), hipMemcpyHostToDevice);
    if (he == hipSuccess && d.hot_pages > 1) {
        he = hipMemsetAsync(d.xhot.p + page_floats, 0, page_floats * (size_t)(d.hot_pages - 1) * sizeof(float), nullptr);
        if (he == hipSuccess) {
            hipLaunchKernelGGL(k_fill_hot_pages, dim3((unsigned)((d.n_rows * 8 + 255) / 256)), dim3(256), 0, nullptr, d.row_ptr.p, d.col.p, d.val.p, d.n_rows,
                               d.d_hot_ids.p, d.hot_pages, d.xhot.p, (int64_t)page_floats);
            he = hipGetLastError();
        }
        if (he == hipSuccess) he = hipStreamSynchronize(nullptr);
    }
    if (he != hipSuccess) return fail(FMHIP_ERR_HIP, "filling the dense hot block's pages: %s", hipGetErrorString(he));
    return FMHIP_OK;
}

// the fp64 ALS learner's copies: values and labels, and every row once more sorted by feature
template <typename FT>
int upload_als_copies(fmhip_dataset &d, const int64_t *row_ptr, const int32_t *col, const FT *val, const FT *y, int threads) {
    const std::vector<double> val64 = converted<double>(val, d.nnz, 1), y64 = converted<double>(y, d.n_rows, 1);
    const SortedRows sr = sort_rows_by_feature(d.n_rows, row_ptr, col, val, threads);
    d.als_dup = sr.dup;
    TRY(upload(d.val64, val64.data(), val64.size()));
    TRY(upload(d.y64, y64.data(), y64.size()));
    TRY(d.cval64.alloc((size_t)d.nnz));
    TRY(upload(d.scol, sr.scol.data(), sr.scol.size()));
    return upload(d.sval64, sr.sval.data(), sr.sval.size());
}

// what the per-batch transposes work in, allocated once for the largest batch
struct TransposeScratch {
    DevBuf<uint32_t> drop, idx_a, idx_b;
    DevBuf<int32_t> keys_a, keys_b, rowid, starts, feats, count, rr_first, rr_last;
    DevBuf<uint8_t> flags, tmp;
    CscScratch sc;
    std::vector<int32_t> cnt, base, h_first, h_last;   // finish_batch_meta's zeroed scratch; the range rows read back
    int alloc(size_t max_nnz, int key_bits, int32_t dim, const std::vector<uint32_t> &drop_bits) {
        if (!drop_bits.empty()) TRY(upload(drop, drop_bits.data(), drop_bits.size()));
        size_t tmp_bytes = 0;
        const hipError_t he = max_nnz ? csc_scratch_bytes(max_nnz, key_bits, &tmp_bytes) : hipSuccess;
        if (he != hipSuccess) return fail(FMHIP_ERR_HIP, "rocPRIM scratch query failed: %s", hipGetErrorString(he));
        TRY(keys_a.alloc(max_nnz)); TRY(keys_b.alloc(max_nnz)); TRY(idx_a.alloc(max_nnz)); TRY(idx_b.alloc(max_nnz));
        TRY(rowid.alloc(max_nnz)); TRY(flags.alloc(max_nnz));
        TRY(starts.alloc(max_nnz + 1)); TRY(feats.alloc(max_nnz + 1));   // (row-blocked streams repeat a feature once per block)
        TRY(count.alloc(1)); TRY(tmp.alloc(tmp_bytes + 16));
        sc.keys_a = keys_a.p; sc.keys_b = keys_b.p; sc.idx_a = idx_a.p; sc.idx_b = idx_b.p; sc.rowid = rowid.p;
        sc.flags = flags.p; sc.starts = starts.p; sc.feats = feats.p; sc.count = count.p; sc.tmp = tmp.p; sc.tmp_bytes = tmp_bytes;
        cnt.assign((size_t)dim + 2, 0);
        base.assign((size_t)dim + 2, 0);
        return FMHIP_OK;
    }
};

// the column index (offsets, feature ids) of the batch just transposed, read back; the pseudo-column of the dropped entries cut off
int read_columns(const TransposeScratch &ts, const BatchMeta &bm, int64_t b, int32_t drop_key, HostBatch &hb) {
    int32_t nc = 0;
    hipError_t he = hipMemcpy(&nc, ts.sc.count, sizeof nc, hipMemcpyDeviceToHost);
    if (he == hipSuccess) {
        hb.cfeat.resize((size_t)nc);
        hb.cptr.resize((size_t)nc + 1);
        if (nc) {
            he = hipMemcpy(hb.cfeat.data(), ts.sc.feats, (size_t)nc * sizeof(int32_t), hipMemcpyDeviceToHost);
            if (he == hipSuccess) he = hipMemcpy(hb.cptr.data(), ts.sc.starts, (size_t)nc * sizeof(int32_t), hipMemcpyDeviceToHost);
        }
        hb.cptr[(size_t)nc] = bm.nnz;
        if (he == hipSuccess && ts.drop.p && nc > 0 && hb.cfeat[(size_t)nc - 1] == drop_key) {
            hb.cfeat.pop_back();               // the stream ends where the pseudo-column starts
            hb.cptr.pop_back();
        }
        if (he == hipSuccess && hb.cptr.back() != bm.cnnz)
            return fail(FMHIP_ERR_HIP, "batch %lld: the transpose holds %d entries, the host counted %d", (long long)b, hb.cptr.back(), bm.cnnz);
    }
    if (he != hipSuccess) return fail(FMHIP_ERR_HIP, "device transpose of batch %lld failed: %s", (long long)b, hipGetErrorString(he));
    return FMHIP_OK;
}

// ALS level schedule of a single-batch dataset (fmhip_host.h, als_levels) from its transpose's row ids
int als_schedule(fmhip_dataset &d, const BatchMeta &bm, const HostBatch &hb) {
    std::vector<uint32_t> h_crow((size_t)bm.cnnz);
    const hipError_t he = hipMemcpy(h_crow.data(), d.crow.p + bm.nnz0, h_crow.size() * sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (he != hipSuccess) return fail(FMHIP_ERR_HIP, "reading the transpose back for the ALS level schedule: %s", hipGetErrorString(he));
    std::vector<int32_t> cols;
    als_levels(hb.cptr, h_crow.data(), bm.rows, d.als_lev_ptr, cols);
    TRY(upload(d.als_lev_cols, cols.data(), cols.size()));
    d.h_als_lev_cols.swap(cols);
    return FMHIP_OK;
}

// band-affine placement of batch b's ranges (fmhip_host.h, plan_bands): its lists, then the same lists in walk order, behind xlist_all
int band_plan(fmhip_dataset &d, int64_t b, const HostBatch &hb, TransposeScratch &ts, std::vector<int32_t> &xlist_all) {
    BatchMeta &bm = d.batches[(size_t)b];
    const int32_t nr = (int32_t)hb.range_seg.size();
    if ((size_t)nr > ts.rr_first.n) { TRY(ts.rr_first.alloc((size_t)nr)); TRY(ts.rr_last.alloc((size_t)nr)); }
    ts.h_first.resize((size_t)nr);
    ts.h_last.resize((size_t)nr);
    hipError_t he = csc_range_rows(nullptr, d.crow.p + bm.nnz0, bm.cnnz, kRangeLen, nr, ts.rr_first.p, ts.rr_last.p);
    if (he == hipSuccess) he = hipMemcpy(ts.h_first.data(), ts.rr_first.p, (size_t)nr * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (he == hipSuccess) he = hipMemcpy(ts.h_last.data(), ts.rr_last.p, (size_t)nr * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (he != hipSuccess) return fail(FMHIP_ERR_HIP, "range rows of batch %lld: %s", (long long)b, hipGetErrorString(he));
    std::vector<int32_t> lists[kXcds], walk[kXcds];
    bm.x_affine = plan_bands(hb, bm.cnnz, bm.rows, ts.h_first, ts.h_last, lists, bm.xseg, walk_order_default(), &walk);
    for (int x = 0; x < kXcds; ++x) {
        bm.xoff[x] = (int64_t)xlist_all.size();
        bm.xlen[x] = (int32_t)lists[x].size();
        xlist_all.insert(xlist_all.end(), lists[x].begin(), lists[x].end());
    }
    for (int x = 0; x < kXcds; ++x) {                 // the walk order of the same lists (whole-batch launches)
        bm.woff[x] = (int64_t)xlist_all.size();
        xlist_all.insert(xlist_all.end(), walk[x].begin(), walk[x].end());
    }
    return FMHIP_OK;
}

// Phase 7: per-batch row -> column transposes, built on the device (csc_build.hip); only the small column index (offsets,
// feature ids) comes back to the host, where each batch's metadata, the ALS levels and the band plan are made from it
int build_transposes(fmhip_dataset &d, bool keep64, int64_t want_rb, const std::vector<uint32_t> &drop_bits, std::vector<HostBatch> &hbs) {
    const int32_t dim = (int32_t)d.dimension;
    int32_t max_nnz = 0;
    for (const BatchMeta &bm : d.batches) max_nnz = std::max(max_nnz, bm.nnz);
    // gradient-side hot pages: their entries are keyed dim + 1 and sort behind every real column
    const bool drop = !drop_bits.empty();
    const int32_t drop_key = dim + 1;
    int key_bits = 1;
    while (key_bits < 31 && ((int64_t)1 << key_bits) <= (int64_t)dim + (drop ? 1 : 0)) ++key_bits;
    // optional row blocking of the transposes (FMHIP_TUNE_ROW_BLOCK): entries sorted by (row block,
    // feature) so that a block's slice of P stays L2-resident while its columns are walked
    int rb_bits = 0;
    if (want_rb > 0) {
        const int64_t blocks = (d.max_rows + want_rb - 1) / want_rb;
        while (((int64_t)1 << rb_bits) < blocks) ++rb_bits;
        if (key_bits + rb_bits > 31) rb_bits = 0;
    }
    d.rb_rows = rb_bits > 0 ? want_rb : 0;
    const int32_t rb_div = d.rb_rows > 0 ? (int32_t)std::min<int64_t>(d.rb_rows, INT32_MAX) : INT32_MAX;
    TransposeScratch ts;
    TRY(ts.alloc((size_t)max_nnz, key_bits, dim, drop_bits));
    std::vector<int32_t> xlist_all;
    for (size_t b = 0; b < hbs.size(); ++b) {
        const BatchMeta &bm = d.batches[b];
        HostBatch &hb = hbs[b];
        const hipError_t he = csc_build_batch(nullptr, ts.sc, d.row_ptr.p, d.col.p, d.val.p, keep64 ? d.val64.p : nullptr, bm.row0, bm.rows, bm.nnz0, bm.nnz,
                                              key_bits, rb_div, rb_bits, d.crow.p, d.cval.p, keep64 ? d.cval64.p : nullptr, ts.drop.p, drop_key);
        if (he != hipSuccess) return fail(FMHIP_ERR_HIP, "device transpose of batch %lld failed: %s", (long long)b, hipGetErrorString(he));
        TRY(read_columns(ts, bm, (int64_t)b, drop_key, hb));
        finish_batch_meta(hb, bm.cnnz, ts.cnt, ts.base);
        if (keep64 && d.rb_rows == 0 && !hb.cfeat.empty() && bm.cnnz > 0) TRY(als_schedule(d, bm, hb));
        // large batches of feature-sorted transposes only
        if (d.rb_rows == 0 && hb.range_seg.size() >= 1024) TRY(band_plan(d, (int64_t)b, hb, ts, xlist_all));
    }
    TRY(upload(d.xlist, xlist_all.data(), xlist_all.size()));
    d.h_xlist.swap(xlist_all);
    return FMHIP_OK;
}

// Phase 8: the batches' column indexes packed end to end (BatchMeta holds the offsets), with the bitmap of the features whose
// gradient rows the fixup launch assembles (cut columns + hot block), per batch: the merged finish skips them in its dense pass.
// Kept for models of up to 2^24 features (2 MiB per batch).
int pack_column_index(fmhip_dataset &d, std::vector<HostBatch> &hbs) {
    const int64_t dim = d.dimension, nb = (int64_t)hbs.size();
    std::vector<uint32_t> own;
    if (d.rb_rows == 0 && dim < (1 << 24) && nb * (dim / 32 + 1) <= ((int64_t)1 << 26)) {
        d.own_words = dim / 32 + 1;
        own = own_bitmaps(hbs, d.hot_ids, (int32_t)dim);
        for (int64_t b = 0; b < nb; ++b) d.batches[(size_t)b].own_off = b * d.own_words;
    }
    std::vector<int32_t> cfeat, cptr, range_seg, split_seg, split_short, cdst, mp_feat, mp_ptr;
    auto append = [](std::vector<int32_t> &all, const std::vector<int32_t> &one, int32_t *n) {      // -> where `one` starts in `all`
        if (n) *n = (int32_t)one.size();
        all.insert(all.end(), one.begin(), one.end());
        return (int64_t)(all.size() - one.size());
    };
    for (int64_t b = 0; b < nb; ++b) {
        BatchMeta &bm = d.batches[(size_t)b];
        HostBatch &hb = hbs[(size_t)b];
        bm.n_feats = hb.n_feats;
        bm.n_pieces = hb.n_pieces;
        append(cdst, hb.cdst, nullptr);
        append(mp_ptr, hb.mp_ptr, nullptr);
        append(cptr, hb.cptr, nullptr);
        bm.mp_off = append(mp_feat, hb.mp_feat, &bm.n_mp);
        bm.col_off = append(cfeat, hb.cfeat, &bm.n_cols);
        bm.range_off = append(range_seg, hb.range_seg, &bm.n_ranges);
        bm.split_off = append(split_seg, hb.split_seg, &bm.n_split);
        bm.split_short_off = append(split_short, hb.split_short, &bm.n_split_short);
        d.max_pieces = std::max(d.max_pieces, bm.n_pieces);
        d.max_ranges = std::max(d.max_ranges, bm.n_ranges);
        HostBatch().cfeat.swap(hb.cfeat);
    }
    d.h_cfeat = cfeat;
    d.h_cptr = cptr;
    d.h_split = split_seg;
    d.h_split_short = split_short;
    TRY(upload(d.cfeat, cfeat.data(), cfeat.size())); TRY(upload(d.cptr, cptr.data(), cptr.size()));
    TRY(upload(d.range_seg, range_seg.data(), range_seg.size()));
    TRY(upload(d.split_seg, split_seg.data(), split_seg.size())); TRY(upload(d.split_short, split_short.data(), split_short.size()));
    TRY(upload(d.cdst, cdst.data(), cdst.size()));
    TRY(upload(d.mp_feat, mp_feat.data(), mp_feat.size())); TRY(upload(d.mp_ptr, mp_ptr.data(), mp_ptr.size()));
    return upload(d.own_bits, own.data(), own.size());
}

// scoring = true: rows + labels only (FMModel.predict / Model.computeRMSE on held-out data,
// S/driver.scala:100-112) — no transposes, no hot block, nothing a training step needs
// hot_opt: -1 = the process-wide defaults (FMHIP_TUNE_HOT_BLOCK, FMHIP_TUNE_HOT_PAGES), 0 = no hot block, n >= 1 = up to n pages of it;
// rb_opt: -1 = the default (FMHIP_TUNE_ROW_BLOCK)
template <typename FT>
int dataset_create_impl(int device, int64_t n_rows, const int64_t *row_ptr, const int32_t *col, const FT *val,
                        const FT *y, int64_t batch_rows, bool scoring, fmhip_dataset_t *out, int hot_opt = -1,
                        int64_t rb_opt = -1, const double *weight = nullptr) {
    const bool want_hot = hot_opt < 0 ? tune_default(kTuneHot) > 0 : hot_opt > 0;
    const int max_hot_pages = std::max(1, std::min(kHotPages, hot_opt > 0 ? hot_opt : tune_default(kTuneHotPages)));
    const int64_t want_rb = rb_opt < 0 ? std::max(tune_default(kTuneRowBlock), 0) : rb_opt;
    if (!out) return fail(FMHIP_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (n_rows < 0) return fail(FMHIP_ERR_INVALID, "n_rows < 0");
    if (!row_ptr) return fail(FMHIP_ERR_INVALID, "row_ptr is NULL");
    if (row_ptr[0] != 0) return fail(FMHIP_ERR_INVALID, "row_ptr[0] must be 0");
    PhaseTimer pt;
    // ---- 1. validate (before the first HIP call)
    const RowCheck chk = validate_rows(n_rows, row_ptr, col, host_threads(std::max(n_rows, row_ptr[n_rows])));
    if (chk.bad_row >= 0) return fail(FMHIP_ERR_INVALID, "row_ptr decreases at row %lld", (long long)chk.bad_row);
    const int64_t nnz = row_ptr[n_rows];
    if (nnz > 0 && (!col || !val)) return fail(FMHIP_ERR_INVALID, "col/val is NULL");
    if (n_rows > 0 && !y && !scoring) return fail(FMHIP_ERR_INVALID, "y is NULL");
    if (chk.bad_entry >= 0) return fail(FMHIP_ERR_INVALID, "negative feature index at entry %lld", (long long)chk.bad_entry);
    const int32_t dim = chk.dim;
    if (weight) {     // per-row example weights (include/fmhip_weights.h): finite and >= 0
        const int64_t bad = validate_weights(n_rows, weight, host_threads(n_rows));
        if (bad >= 0) return fail(FMHIP_ERR_INVALID, "weight[%lld] = %g: a row's weight must be finite (as fp32) and >= 0", (long long)bad, weight[bad]);
    }
    pt.lap("validate");
    TRY(set_device(device));
    std::unique_ptr<fmhip_dataset> d(new (std::nothrow) fmhip_dataset());
    if (!d) return fail(FMHIP_ERR_NOMEM, "out of host memory");
    d->device = device;
    d->n_rows = n_rows;
    d->nnz = nnz;
    d->dimension = dim;  // S/DataSet.scala:27-29
    d->scoring_only = scoring;
    if (scoring) batch_rows = 262144;   // bounds the forward's workspace; invisible to the caller
    if (batch_rows <= 0 || batch_rows > n_rows) batch_rows = std::max<int64_t>(n_rows, 1);
    d->batch_rows = batch_rows;
    const int64_t nb = n_rows > 0 ? (n_rows + batch_rows - 1) / batch_rows : 0;
    const int T = host_threads(n_rows);
    // ---- 2. dense hot block (FMHIP_TUNE_HOT_BLOCK, FMHIP_TUNE_HOT_PAGES; fmhip_host.h, choose_hot_block): x_rh sits in xhot[page][r][slot].
    // A single-batch dataset the ALS learner could walk (its whole transpose, at most kAlsMaxNnz nonzeros) is split only when the
    // caller asks for the block by name (fmhip_dataset_opts::hot_block >= 1: such a dataset is for SGD, fmhip_als_epoch refuses
    // it); larger single-batch datasets — full-batch SGD — are split like any other.
    HotSplit sp;
    bool split = false;
    if (want_hot && (nb > 1 || nnz > kAlsMaxNnz || hot_opt > 0) && nnz > 0 && !scoring) {
        HotBlock hb = choose_hot_block(n_rows, row_ptr, col, val, dim, max_hot_pages, want_rb > 0, T);
        if (hb.pages) {
            sp = split_hot_rows(n_rows, row_ptr, col, val, dim, batch_rows, hb, T);
            split = true;
            d->hot_T = kHotT;
            d->hot_pages = hb.pages;
            d->hot_ids.swap(hb.hot_ids);
            d->hot_max_id = *std::max_element(d->hot_ids.begin(), d->hot_ids.end());
            d->hot0_max_id = *std::max_element(d->hot_ids.begin(), d->hot_ids.begin() + kHotT);
        }
    }
    pt.lap("hot block: choose + split");
    // ---- 3. batch table, over the CSR stream as the device will hold it
    const int64_t *sp_row_ptr = split ? sp.sp_ptr.data() : row_ptr;
    const int32_t *sp_col = split ? sp.sp_col.get() : col;
    TRY(batch_table(*d, sp_row_ptr, row_ptr, split ? &sp : nullptr));
    const int64_t nnz_s = d->nnz_sparse;
    // ---- 4. forward walk order of each batch: rows by (sparse) length, longest first, ties in row order
    {
        const char *ow = getenv("FMHIP_ORDER_WINDOW");   // experiment: sort inside windows of this many rows (0 = the whole batch)
        const std::vector<int32_t> order = forward_row_order(n_rows, batch_rows, sp_row_ptr, ow ? atoll(ow) : 0, T);
        TRY(upload(d->row_order, order.data(), order.size()));
    }
    pt.lap("row order + upload");
    // ---- 5. fp32 copies of the streams (device arithmetic is fp32) and H2D
    {
        std::vector<float> valf;
        const float *val_up = split ? sp.sp_val.get() : reinterpret_cast<const float *>(val);   // (FT = float: the caller's array as it is)
        if (!split && !std::is_same<FT, float>::value) {
            valf = converted<float>(val, nnz_s, host_threads(nnz_s));
            val_up = valf.data();
        }
        const std::vector<float> yf = y ? converted<float>(y, n_rows, 1) : std::vector<float>((size_t)n_rows, 0.f);
        TRY(upload(d->row_ptr, sp_row_ptr, (size_t)n_rows + 1)); TRY(upload(d->col, sp_col, (size_t)nnz_s));
        TRY(upload(d->val, val_up, (size_t)nnz_s)); TRY(upload(d->y, yf.data(), (size_t)n_rows));
        if (weight) {
            const std::vector<float> cf = converted<float>(weight, n_rows, 1);
            for (float c : cf) d->weight_sum += (double)c;
            TRY(upload(d->c, cf.data(), (size_t)n_rows));
            d->weighted = true;
        }
        if (!scoring) { TRY(d->crow.alloc((size_t)nnz_s)); TRY(d->cval.alloc((size_t)nnz_s)); }
        if (split) {
            TRY(d->xhot.alloc((size_t)std::max<int64_t>(n_rows, 1) * kHotT * (size_t)d->hot_pages));
            TRY(upload(d->d_hot_ids, d->hot_ids.data(), d->hot_ids.size()));
            TRY(upload_hot_pages(*d, sp.xhot0.get()));
        }
    }
    sp.xhot0.reset();
    sp.sp_val.reset();
    pt.lap("fp32 re-pack + H2D");
    if (scoring) {
        *out = d.release();
        return FMHIP_OK;
    }
    // ---- 6. fp64 ALS copies (single-batch datasets without a hot block)
    const bool keep64 = !split && nb == 1 && nnz <= kAlsMaxNnz;
    if (keep64) TRY(upload_als_copies(*d, row_ptr, col, val, y, T));
    // ---- 7. device transposes and per-batch metadata
    std::vector<HostBatch> hbs((size_t)nb);
    TRY(build_transposes(*d, keep64, want_rb, sp.drop_bits, hbs));
    pt.lap("device transposes + metadata");
    // ---- 8. pack and upload the column index
    TRY(pack_column_index(*d, hbs));
    pt.lap("pack + upload column index");
    *out = d.release();
    return FMHIP_OK;
}

// one thread per row: the entries of features below `cut` first, then the others, each group in its stored order
__global__ __launch_bounds__(256) void k_row_partition(const int64_t *row_ptr, int64_t n_rows, const int32_t *col, const float *val, int32_t cut,
                                                       int32_t *col_out, float *val_out, int64_t *split) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n_rows) return;
    const int64_t p0 = row_ptr[r], p1 = row_ptr[r + 1];
    int64_t h = p0;
    for (int64_t p = p0; p < p1; ++p)
        if (col[p] < cut) { col_out[h] = col[p]; val_out[h] = val[p]; ++h; }
    split[r] = h;
    for (int64_t p = p0; p < p1; ++p)
        if (col[p] >= cut) { col_out[h] = col[p]; val_out[h] = val[p]; ++h; }
}

// Stable partition of every row's stored entries at feature id `cut` (the two-pass forward, fm_kernels.h kFwdPartA / B) into a
// COPY of the CSR stream (col_part / val_part) that only the two-pass forward reads: the dataset's own streams never move, so
// threads that score or train other models on the same dataset are not disturbed (the first version swapped the
// partitioned copy in for the streams under a launch that might still be reading them).  One partition per dataset: it is
// re-made for another cut unless a pipelined run is using it (part_users, fmhip_comm.hip) — then the call fails and says so.
int partition_rows_locked(fmhip_dataset_t d, int64_t cut_feature) {
    const int32_t cut = (int32_t)std::min<int64_t>(cut_feature, INT32_MAX);
    if (d->split_cut == cut) return FMHIP_OK;
    if (d->part_users > 0)
        return fail(FMHIP_ERR_INVALID, "the dataset's rows are partitioned at feature %lld and a pipelined data-parallel run is using that partition: "
                                       "models that share a dataset must share the top cut of their plans (asked for: %d)", (long long)d->split_cut, cut);
    const int64_t nnz_s = d->nnz_sparse;
    TRY(d->row_split.ensure((size_t)std::max<int64_t>(d->n_rows, 1)));
    TRY(d->col_part.ensure((size_t)std::max<int64_t>(nnz_s, 1)));
    TRY(d->val_part.ensure((size_t)std::max<int64_t>(nnz_s, 1)));
    // an earlier partition may still be read by launches queued on some model's stream (a run releases it when it has
    // ENQUEUED its steps): drain the device before the copy is overwritten
    if (d->split_cut >= 0) HIP_TRY(hipDeviceSynchronize());
    d->split_cut = -1;                     // (a failure below leaves no half-made partition behind)
    if (d->n_rows > 0) {
        hipLaunchKernelGGL(k_row_partition, dim3((unsigned)((d->n_rows + 255) / 256)), dim3(256), 0, nullptr, d->row_ptr.p, d->n_rows, d->col.p, d->val.p,
                           cut, d->col_part.p, d->val_part.p, d->row_split.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(nullptr));
    }
    d->split_cut = cut;
    return FMHIP_OK;
}

}  // namespace host
}  // namespace fmhip

extern "C" {

int fmhip_dataset_create(int device, int64_t n_rows, const int64_t *row_ptr, const int32_t *col, const double *val,
                         const double *y, int64_t batch_rows, fmhip_dataset_t *out) {
    return dataset_create_impl<double>(device, n_rows, row_ptr, col, val, y, batch_rows, false, out);
}

int fmhip_dataset_create_opts(int device, int64_t n_rows, const int64_t *row_ptr, const int32_t *col, const double *val,
                              const double *y, const fmhip_dataset_opts *opts, fmhip_dataset_t *out) {
    if (!opts || opts->struct_size != (int32_t)sizeof(fmhip_dataset_opts))
        return fail(FMHIP_ERR_INVALID, "opts is NULL or its struct_size is not sizeof(fmhip_dataset_opts)");
    return dataset_create_impl<double>(device, n_rows, row_ptr, col, val, y, opts->batch_rows, false, out, opts->hot_block,
                                       opts->row_block_rows);
}

int fmhip_rows_create(int device, int64_t n_rows, const int64_t *row_ptr, const int32_t *col, const double *val,
                      const double *y, fmhip_dataset_t *out) {
    return dataset_create_impl<double>(device, n_rows, row_ptr, col, val, y, 0, true, out);
}

int fmhip_rows_create_f32(int device, int64_t n_rows, const int64_t *row_ptr, const int32_t *col, const float *val,
                          const float *y, fmhip_dataset_t *out) {
    return dataset_create_impl<float>(device, n_rows, row_ptr, col, val, y, 0, true, out);
}

int fmhip_dataset_create_f32(int device, int64_t n_rows, const int64_t *row_ptr, const int32_t *col, const float *val,
                             const float *y, int64_t batch_rows, fmhip_dataset_t *out) {
    return dataset_create_impl<float>(device, n_rows, row_ptr, col, val, y, batch_rows, false, out);
}

// ---- per-row example weights (include/fmhip_weights.h)

int fmhip_dataset_create_weighted(int device, int64_t n_rows, const int64_t *row_ptr, const int32_t *col, const double *val,
                                  const double *y, const double *weight, const fmhip_dataset_opts *opts, fmhip_dataset_t *out) {
    if (opts && opts->struct_size != (int32_t)sizeof(fmhip_dataset_opts))
        return fail(FMHIP_ERR_INVALID, "opts->struct_size is not sizeof(fmhip_dataset_opts)");
    return dataset_create_impl<double>(device, n_rows, row_ptr, col, val, y, opts ? opts->batch_rows : 0, false, out, opts ? opts->hot_block : -1,
                                       opts ? opts->row_block_rows : -1, weight);
}

int fmhip_rows_create_weighted(int device, int64_t n_rows, const int64_t *row_ptr, const int32_t *col, const double *val,
                               const double *y, const double *weight, fmhip_dataset_t *out) {
    return dataset_create_impl<double>(device, n_rows, row_ptr, col, val, y, 0, true, out, -1, -1, weight);
}

int fmhip_dataset_weights(fmhip_dataset_t d, int *has, double *sum, double *out) {
    if (!d) return fail(FMHIP_ERR_INVALID, "dataset is NULL");
    if (has) *has = d->weighted ? 1 : 0;
    if (sum) *sum = d->weighted ? d->weight_sum : (double)d->n_rows;
    if (!out || d->n_rows == 0) return FMHIP_OK;
    if (!d->weighted) {
        std::fill(out, out + d->n_rows, 1.0);
        return FMHIP_OK;
    }
    TRY(set_device(d->device));
    std::vector<float> h((size_t)d->n_rows);
    HIP_TRY(hipMemcpy(h.data(), d->c.p, h.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (int64_t r = 0; r < d->n_rows; ++r) out[r] = (double)h[(size_t)r];
    return FMHIP_OK;
}

int fmhip_dataset_destroy(fmhip_dataset_t d) {
    if (!d) return FMHIP_OK;
    (void)hipSetDevice(d->device);
    std::unique_ptr<fmhip_dataset>(d).reset();
    return FMHIP_OK;
}

int fmhip_dataset_info(fmhip_dataset_t d, int64_t *n_rows, int64_t *nnz, int64_t *dimension, int64_t *batch_rows,
                       int64_t *n_batches) {
    if (!d) return fail(FMHIP_ERR_INVALID, "dataset is NULL");
    if (n_rows) *n_rows = d->n_rows;
    if (nnz) *nnz = d->nnz;
    if (dimension) *dimension = d->dimension;
    if (batch_rows) *batch_rows = d->batch_rows;
    if (n_batches) *n_batches = (int64_t)d->batches.size();
    return FMHIP_OK;
}

int fmhip_dataset_batch_info(fmhip_dataset_t d, int64_t batch, int64_t *row0, int64_t *rows, int64_t *nnz,
                             int64_t *n_columns) {
    if (!d) return fail(FMHIP_ERR_INVALID, "dataset is NULL");
    TRY(check_batch(d, batch));
    const BatchMeta &bm = d->batches[(size_t)batch];
    if (row0) *row0 = bm.row0;
    if (rows) *rows = bm.rows;
    if (nnz) *nnz = bm.nnz_total;
    if (n_columns) *n_columns = bm.n_feats + __builtin_popcountll((uint64_t)bm.hot_mask) + __builtin_popcountll((uint64_t)(bm.hot_mask >> 64));
    return FMHIP_OK;
}

int fmhip_dataset_get_transpose(fmhip_dataset_t d, int64_t batch, int32_t *feat, int32_t *ptr, int32_t *rows,
                                float *vals) {
    if (!d) return fail(FMHIP_ERR_INVALID, "dataset is NULL");
    TRY(check_batch(d, batch));
    if (d->scoring_only) return fail(FMHIP_ERR_UNSUPPORTED, "a scoring-only dataset has no transposes");
    TRY(set_device(d->device));
    const BatchMeta &bm = d->batches[(size_t)batch];
    // read the stream back and merge the pieces of a feature (one per row block, in row-block = row
    // order) so the caller sees one column per feature whatever the device layout
    std::vector<int32_t> hrow((size_t)bm.cnnz);
    std::vector<float> hval((size_t)bm.cnnz);
    if (bm.cnnz) {
        HIP_TRY(hipMemcpy(hrow.data(), d->crow.p + bm.nnz0, (size_t)bm.cnnz * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(hval.data(), d->cval.p + bm.nnz0, (size_t)bm.cnnz * sizeof(float), hipMemcpyDeviceToHost));
    }
    const int32_t *hf = d->h_cfeat.data() + bm.col_off, *hp = d->h_cptr.data() + bm.col_off + batch;
    std::vector<int32_t> order((size_t)bm.n_cols);
    for (int32_t s = 0; s < bm.n_cols; ++s) order[(size_t)s] = s;
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return hf[x] < hf[y]; });
    // the dense hot block's columns (never present in the transposed stream) are merged in by feature id
    const int n_slots = d->hot_pages * kHotT;
    const size_t page_floats = (size_t)std::max<int64_t>(d->n_rows, 1) * kHotT;
    std::vector<float> hx;
    std::vector<int> hslots;               // the batch's live slots, by ascending feature id
    if (bm.hot_mask) {
        hx.resize((size_t)bm.rows * n_slots);
        for (int pg = 0; pg < d->hot_pages; ++pg)
            HIP_TRY(hipMemcpy(hx.data() + (size_t)pg * bm.rows * kHotT, d->xhot.p + (size_t)pg * page_floats + (size_t)bm.row0 * kHotT,
                              (size_t)bm.rows * kHotT * sizeof(float), hipMemcpyDeviceToHost));
        for (int h = 0; h < n_slots; ++h)
            if (d->hot_ids[(size_t)h] >= 0 && (bm.hot_mask >> h & 1u)) hslots.push_back(h);
        std::sort(hslots.begin(), hslots.end(), [&](int x, int y) { return d->hot_ids[(size_t)x] < d->hot_ids[(size_t)y]; });
    }
    int32_t nf = 0, pos = 0;
    size_t hnext = 0;
    auto emit_hot_below = [&](int64_t bound) {
        for (; hnext < hslots.size(); ++hnext) {
            const int h = hslots[hnext];
            const int32_t id = d->hot_ids[(size_t)h];
            if ((int64_t)id >= bound) break;
            if (feat) feat[nf] = id;
            if (ptr) ptr[nf] = pos;
            ++nf;
            const float *xp = hx.data() + (size_t)(h / kHotT) * bm.rows * kHotT + (h % kHotT);
            for (int64_t r = 0; r < bm.rows; ++r) {
                const float x = xp[(size_t)r * kHotT];
                if (x != 0.f) {
                    if (rows) rows[pos] = (int32_t)r;
                    if (vals) vals[pos] = x;
                    ++pos;
                }
            }
        }
    };
    for (int32_t i = 0; i < bm.n_cols; ++i) {
        const int32_t s = order[(size_t)i];
        if (i == 0 || hf[s] != hf[order[(size_t)i - 1]]) {
            emit_hot_below(hf[s]);
            if (feat) feat[nf] = hf[s];
            if (ptr) ptr[nf] = pos;
            ++nf;
        }
        for (int32_t p = hp[s]; p < hp[s + 1]; ++p, ++pos) {
            if (rows) rows[pos] = hrow[(size_t)p] & 0x7fffffff;
            if (vals) vals[pos] = hval[(size_t)p];
        }
    }
    emit_hot_below(INT64_MAX);
    if (ptr) ptr[nf] = pos;
    return FMHIP_OK;
}

// ---- how a dataset was laid out (measurement aid)

int fmhip_dataset_layout(fmhip_dataset_t d, int32_t *n_hot, int32_t *hot_ids, int64_t *nnz_sparse) {
    if (!d) return fail(FMHIP_ERR_INVALID, "dataset is NULL");
    int32_t n = 0;
    for (int h = 0; h < (int)std::min<size_t>(d->hot_ids.size(), kHotT); ++h)      // page 0: the two-sided page
        if (d->hot_ids[(size_t)h] >= 0) {
            if (hot_ids) hot_ids[n] = d->hot_ids[(size_t)h];
            ++n;
        }
    if (n_hot) *n_hot = n;
    if (nnz_sparse) *nnz_sparse = d->nnz_sparse;
    return FMHIP_OK;
}

int fmhip_dataset_hot_pages(fmhip_dataset_t d, int32_t *n_pages, int32_t *n_ids, int32_t *ids, int64_t *nnz_sparse_backward) {
    if (!d) return fail(FMHIP_ERR_INVALID, "dataset is NULL");
    int32_t n = 0;
    for (size_t h = 0; h < d->hot_ids.size(); ++h)
        if (d->hot_ids[h] >= 0) {
            if (ids) ids[n] = d->hot_ids[h];
            ++n;
        }
    if (n_pages) *n_pages = d->hot_pages;
    if (n_ids) *n_ids = n;
    if (nnz_sparse_backward) *nnz_sparse_backward = d->scoring_only ? 0 : d->nnz_sparse_bwd;
    return FMHIP_OK;
}

int fmhip_dataset_partition_rows(fmhip_dataset_t d, int64_t cut_feature) {
    if (!d) return fail(FMHIP_ERR_INVALID, "dataset is NULL");
    if (cut_feature < 0) return fail(FMHIP_ERR_INVALID, "negative feature id");
    TRY(set_device(d->device));
    std::lock_guard<std::mutex> lock(d->part_mu);
    return partition_rows_locked(d, cut_feature);
}

int fmhip_dataset_band_plan(fmhip_dataset_t d, int64_t *n_ranges, int64_t *planned_ranges, int64_t *band_affine_ranges) {
    if (!d) return fail(FMHIP_ERR_INVALID, "dataset is NULL");
    int64_t all = 0, planned = 0, affine = 0;
    for (const auto &bm : d->batches) {
        all += bm.n_ranges;
        if (bm.xoff[0] >= 0) { planned += bm.n_ranges; affine += bm.x_affine; }
    }
    if (n_ranges) *n_ranges = all;
    if (planned_ranges) *planned_ranges = planned;
    if (band_affine_ranges) *band_affine_ranges = affine;
    return FMHIP_OK;
}

int fmhip_dataset_als_levels(fmhip_dataset_t d, int64_t *n_levels, int64_t *n_columns, int64_t *widest_level) {
    if (!d) return fail(FMHIP_ERR_INVALID, "dataset is NULL");
    const int64_t nl = d->als_lev_ptr.empty() ? 0 : (int64_t)d->als_lev_ptr.size() - 1;
    int64_t widest = 0;
    for (int64_t l = 0; l < nl; ++l) widest = std::max<int64_t>(widest, d->als_lev_ptr[(size_t)l + 1] - d->als_lev_ptr[(size_t)l]);
    if (n_levels) *n_levels = nl;
    if (n_columns) *n_columns = nl ? d->als_lev_ptr.back() : 0;
    if (widest_level) *widest_level = widest;
    return FMHIP_OK;
}

// ---- feature relabelling by frequency (host arithmetic; see include/fmhip.h) -----------------------------------
int fmhip_feature_counts(int64_t nnz, const int32_t *col, int64_t n1, int64_t *counts) {
    if (nnz < 0 || n1 < 1 || n1 > INT32_MAX || !counts || (nnz > 0 && !col)) return fail(FMHIP_ERR_INVALID, "bad arguments");
    const int64_t bad = feature_counts(nnz, col, n1, counts);
    if (bad >= 0) return fail(FMHIP_ERR_INVALID, "col[%lld] = %d outside [0, %lld)", (long long)bad, col[bad], (long long)n1);
    return FMHIP_OK;
}

int fmhip_rank_from_counts(int64_t n1, const int64_t *counts, int32_t *rank, int32_t *by_rank) {
    if (n1 < 1 || n1 > INT32_MAX || !counts || !rank) return fail(FMHIP_ERR_INVALID, "bad arguments");
    rank_from_counts(n1, counts, rank, by_rank);
    return FMHIP_OK;
}

int fmhip_relabel_columns(int64_t nnz, const int32_t *col, int64_t n1, const int32_t *rank, int32_t *out) {
    if (nnz < 0 || n1 < 1 || !rank || (nnz > 0 && (!col || !out))) return fail(FMHIP_ERR_INVALID, "bad arguments");
    const int64_t bad = relabel_columns(nnz, col, n1, rank, out);
    if (bad >= 0) return fail(FMHIP_ERR_INVALID, "col[%lld] outside [0, %lld): nothing can be relied on in `out`", (long long)bad, (long long)n1);
    return FMHIP_OK;
}

}  // extern "C"

// ---- the same three steps on the GPU (the *_gpu entry points): a histogram by atomic adds, a stable descending radix sort
// of (count, id) pairs, a gather — host arithmetic that took 9.7 s for 6M Criteo-shaped rows over 2^25 slots
namespace {
__global__ __launch_bounds__(256) void k_count_ids(const int32_t *col, int64_t n, int64_t n1, unsigned long long *counts, unsigned long long *bad) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t c = col[i];
        if (c < 0 || c >= n1) atomicMin(bad, (unsigned long long)i);
        else atomicAdd(counts + c, 1ull);
    }
}
__global__ __launch_bounds__(256) void k_iota(int32_t *ids, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) ids[i] = (int32_t)i;
}
__global__ __launch_bounds__(256) void k_invert(const int32_t *by_rank, int64_t n, int32_t *rank) {
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256) rank[by_rank[r]] = (int32_t)r;
}
__global__ __launch_bounds__(256) void k_relabel(const int32_t *col, int64_t n, int64_t n1, const int32_t *rank, int32_t *out, unsigned long long *bad) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t c = col[i];
        if (c < 0 || c >= n1) atomicMin(bad, (unsigned long long)i);
        else out[i] = rank[c];
    }
}
constexpr int64_t kRelabelChunk = (int64_t)1 << 26;      // entries per transfer: 256 MB of ids on the card at a time
inline unsigned grid_for(int64_t n) { return (unsigned)std::min<int64_t>(std::max<int64_t>((n + 255) / 256, 1), 16384); }
}  // namespace

extern "C" {

int fmhip_feature_counts_gpu(int device, int64_t nnz, const int32_t *col, int64_t n1, int64_t *counts) {
    if (nnz < 0 || n1 < 1 || n1 > INT32_MAX || !counts || (nnz > 0 && !col)) return fail(FMHIP_ERR_INVALID, "bad arguments");
    TRY(set_device(device));
    DevBuf<unsigned long long> d_cnt, d_bad;
    DevBuf<int32_t> d_col;
    TRY(d_cnt.alloc((size_t)n1));
    TRY(d_bad.alloc(1));
    TRY(d_col.alloc((size_t)std::max<int64_t>(std::min(nnz, kRelabelChunk), 1)));
    HIP_TRY(hipMemset(d_cnt.p, 0, (size_t)n1 * sizeof(unsigned long long)));
    HIP_TRY(hipMemset(d_bad.p, 0xff, sizeof(unsigned long long)));
    for (int64_t at = 0; at < nnz; at += kRelabelChunk) {
        const int64_t n = std::min(kRelabelChunk, nnz - at);
        HIP_TRY(hipMemcpy(d_col.p, col + at, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_count_ids, dim3(grid_for(n)), dim3(256), 0, nullptr, d_col.p, n, n1, d_cnt.p, d_bad.p);
        HIP_TRY(hipGetLastError());
        unsigned long long bad = 0;
        HIP_TRY(hipMemcpy(&bad, d_bad.p, sizeof bad, hipMemcpyDeviceToHost));
        if (bad != ~0ull) return fail(FMHIP_ERR_INVALID, "col[%lld] = %d outside [0, %lld)", (long long)(at + (int64_t)bad), col[at + (int64_t)bad], (long long)n1);
    }
    std::vector<unsigned long long> h((size_t)n1);
    HIP_TRY(hipMemcpy(h.data(), d_cnt.p, (size_t)n1 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    parallel_chunks(n1, host_threads(n1), [&](int, int64_t lo, int64_t hi) {
        for (int64_t f = lo; f < hi; ++f) counts[f] += (int64_t)h[(size_t)f];
    });
    return FMHIP_OK;
}

int fmhip_rank_from_counts_gpu(int device, int64_t n1, const int64_t *counts, int32_t *rank, int32_t *by_rank) {
    if (n1 < 1 || n1 > INT32_MAX || !counts || !rank) return fail(FMHIP_ERR_INVALID, "bad arguments");
    for (int64_t f = 0; f < n1; ++f)
        if (counts[f] < 0) return fail(FMHIP_ERR_INVALID, "counts[%lld] is negative", (long long)f);
    TRY(set_device(device));
    DevBuf<unsigned long long> k_in, k_out;
    DevBuf<int32_t> v_in, v_out, d_rank;
    DevBuf<uint8_t> tmp;
    TRY(k_in.alloc((size_t)n1));
    TRY(k_out.alloc((size_t)n1));
    TRY(v_in.alloc((size_t)n1));
    TRY(v_out.alloc((size_t)n1));
    TRY(d_rank.alloc((size_t)n1));
    size_t tb = 0;
    // descending count; the sort is stable and the ids go in ascending, so ties keep ascending id — the host version's order
    HIP_TRY(rocprim::radix_sort_pairs_desc(nullptr, tb, k_in.p, k_out.p, v_in.p, v_out.p, (size_t)n1, 0, 64, (hipStream_t) nullptr));
    TRY(tmp.alloc(tb + 16));
    HIP_TRY(hipMemcpy(k_in.p, counts, (size_t)n1 * sizeof(int64_t), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_iota, dim3(grid_for(n1)), dim3(256), 0, nullptr, v_in.p, n1);
    HIP_TRY(hipGetLastError());
    HIP_TRY(rocprim::radix_sort_pairs_desc(tmp.p, tb, k_in.p, k_out.p, v_in.p, v_out.p, (size_t)n1, 0, 64, (hipStream_t) nullptr));
    hipLaunchKernelGGL(k_invert, dim3(grid_for(n1)), dim3(256), 0, nullptr, v_out.p, n1, d_rank.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(rank, d_rank.p, (size_t)n1 * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (by_rank) HIP_TRY(hipMemcpy(by_rank, v_out.p, (size_t)n1 * sizeof(int32_t), hipMemcpyDeviceToHost));
    return FMHIP_OK;
}

int fmhip_relabel_columns_gpu(int device, int64_t nnz, const int32_t *col, int64_t n1, const int32_t *rank, int32_t *out) {
    if (nnz < 0 || n1 < 1 || !rank || (nnz > 0 && (!col || !out))) return fail(FMHIP_ERR_INVALID, "bad arguments");
    TRY(set_device(device));
    DevBuf<int32_t> d_rank, d_col, d_out;
    DevBuf<unsigned long long> d_bad;
    const int64_t chunk = std::max<int64_t>(std::min(nnz, kRelabelChunk), 1);
    TRY(d_rank.alloc((size_t)n1));
    TRY(d_col.alloc((size_t)chunk));
    TRY(d_out.alloc((size_t)chunk));
    TRY(d_bad.alloc(1));
    HIP_TRY(hipMemcpy(d_rank.p, rank, (size_t)n1 * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(d_bad.p, 0xff, sizeof(unsigned long long)));
    for (int64_t at = 0; at < nnz; at += kRelabelChunk) {
        const int64_t n = std::min(kRelabelChunk, nnz - at);
        HIP_TRY(hipMemcpy(d_col.p, col + at, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_relabel, dim3(grid_for(n)), dim3(256), 0, nullptr, d_col.p, n, n1, d_rank.p, d_out.p, d_bad.p);
        HIP_TRY(hipGetLastError());
        unsigned long long bad = 0;
        HIP_TRY(hipMemcpy(&bad, d_bad.p, sizeof bad, hipMemcpyDeviceToHost));
        if (bad != ~0ull)
            return fail(FMHIP_ERR_INVALID, "col[%lld] outside [0, %lld): nothing can be relied on in `out`", (long long)(at + (int64_t)bad), (long long)n1);
        HIP_TRY(hipMemcpy(out + at, d_out.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    return FMHIP_OK;
}

}  // extern "C"
