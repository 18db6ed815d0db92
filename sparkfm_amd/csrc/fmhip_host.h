// fmhip_host.h — the library's PURE HOST ARITHMETIC: everything libfmhip.so computes on the host that needs no GPU and no
// HIP header — row shards, feature relabelling, the host passes of the dataset build (validation, the dense hot block's choice and
// split, the forward row order, the ALS row sort, the own bitmaps, the example weights' check), a batch's range / fixup metadata, the band-affine plan of the
// backward's ranges, the ALS sweep's level schedule, the data-parallel plan's cuts, interval edges, equal shares and update groups, the split step's backward window.  fmhip_dataset.hip /
// fmhip_comm.hip call these; tests/host_arith_harness.cpp compiles fmhip_host.cpp with g++ -fsanitize=address,undefined and
// drives them over random shapes (the sanitizers cannot run on the GPU pool, the index arithmetic can run
// here).  Not installed, not part of the ABI.
#pragma once
#include <stdint.h>

#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "fm_constants.h"
#include "mcmc_rng.h"      // rng::AliasEntry

namespace fmhip {
namespace host {

// ---- threads -------------------------------------------------------------------------------------------------
// host cores a pass over `work_items` items may use (FMHIP_HOST_THREADS caps it; at most 32, one per 65536 items)
int host_threads(int64_t work_items);

// f(tid, lo, hi) over [0, n) cut into one contiguous chunk per thread
template <class F>
void parallel_chunks(int64_t n, int threads, F f) {
    if (threads <= 1 || n <= 0) { f(0, (int64_t)0, n); return; }
    std::vector<std::thread> pool;
    pool.reserve((size_t)threads);
    for (int t = 0; t < threads; ++t) {
        const int64_t lo = n * t / threads, hi = n * (t + 1) / threads;
        pool.emplace_back([=]() { f(t, lo, hi); });
    }
    for (auto &th : pool) th.join();
}

// ---- row shards (fmhip_shard_rows) ------------------------------------------------------------------------------
// contiguous shard [lo, hi) of `rank` of `world`, balanced by stored nonzeros (row_ptr[n_rows + 1]); arguments validated by the caller
void shard_bounds(int64_t n_rows, const int64_t *row_ptr, int world, int rank, int64_t *lo, int64_t *hi);

// ---- feature relabelling by frequency (fmhip_feature_counts / _rank_from_counts / _relabel_columns) ----------
// counts[c] += occurrences of c; -> -1, or the index of the first id found outside [0, n1) (counts are then unreliable)
int64_t feature_counts(int64_t nnz, const int32_t *col, int64_t n1, int64_t *counts);
// rank[n1] (and by_rank[n1] unless NULL): position in descending count order, ties by ascending id
void rank_from_counts(int64_t n1, const int64_t *counts, int32_t *rank, int32_t *by_rank);
// out[i] = rank[col[i]]; -> -1, or the index of an id outside [0, n1)
int64_t relabel_columns(int64_t nnz, const int32_t *col, int64_t n1, const int32_t *rank, int32_t *out);

// ---- dataset build (fmhip_dataset_create; FT = float / double, the caller's value type) --------------------------
// the first row where row_ptr decreases (then nothing else is looked at); the first negative entry of col (NULL: not swept); the largest id
struct RowCheck { int64_t bad_row = -1, bad_entry = -1; int32_t dim = 0; };
RowCheck validate_rows(int64_t n_rows, const int64_t *row_ptr, const int32_t *col, int threads);
// per-row example weights (include/fmhip_weights.h): every weight finite — as the fp32 it is stored as — and >= 0.  -> -1, or the
// first row whose weight is not (NaN, +-inf, beyond FLT_MAX, negative; -0.0 passes: it is 0)
int64_t validate_weights(int64_t n_rows, const double *weight, int threads);
// dst[i] = (D)src[i]
template <typename D, typename S>
std::vector<D> converted(const S *src, int64_t n, int threads) {
    std::vector<D> dst((size_t)n);
    parallel_chunks(n, threads, [&](int, int64_t lo, int64_t hi) {
        for (int64_t i = lo; i < hi; ++i) dst[(size_t)i] = (D)src[i];
    });
    return dst;
}
// The dense hot block's features: candidates by descending count (ties: ascending id), page 0 takes up to kHotT of those present in
// >= 10 % of the rows (at least 2, or there is no block), the next (max_pages - 1) * kHotT down to 2.5 % fill pages 1.. (none if
// row_blocked).  One stored twice in a row, or with a value that is 0 as fp32, is refused and the next candidate moves up.  Counts
// are exact up to exact_nnz stored entries, from every s-th row beyond.  -> pages = 0: no block; else hot_ids[pages * kHotT]
// (-1 = unused; live slots first and ascending inside a page), p0 = page 0's live slots, slot[dim + 1] = a feature's slot or -1,
// kept[r + 1] = row r's entries outside page 0
constexpr int64_t kHotExactNnz = (int64_t)8 << 20;
struct HotBlock { int pages = 0; size_t p0 = 0; std::vector<int32_t> hot_ids; std::vector<int8_t> slot; std::vector<int64_t> kept; };
template <typename FT>
HotBlock choose_hot_block(int64_t n_rows, const int64_t *row_ptr, const int32_t *col, const FT *val, int32_t dim, int max_pages, bool row_blocked,
                          int threads, int64_t exact_nnz = kHotExactNnz);
// The rows without page 0's entries: sp_ptr (hb.kept summed in place and moved here) / sp_col / sp_val in stored order, values as
// fp32; xhot0[n_rows][kHotT] = page 0 (0 = absent); per batch of batch_rows rows the slots seen and the kept entries of pages 1..;
// drop_bits: bitmap of the ids of pages 1.. (empty if there are none).  The arrays are allocated uninitialised and written once.
struct HotSplit {
    std::vector<int64_t> sp_ptr, bwd_out;
    std::unique_ptr<int32_t[]> sp_col;
    std::unique_ptr<float[]> sp_val, xhot0;
    std::vector<slotmask_t> hot_masks; std::vector<uint32_t> drop_bits;
};
template <typename FT>
HotSplit split_hot_rows(int64_t n_rows, const int64_t *row_ptr, const int32_t *col, const FT *val, int32_t dim, int64_t batch_rows, HotBlock &hb,
                        int threads);
// forward walk order: per batch of batch_rows rows (window > 0: per window of that many of its rows) the local row ids by stored
// length, longest first, ties in row order; with a window the odd windows are reversed
std::vector<int32_t> forward_row_order(int64_t n_rows, int64_t batch_rows, const int64_t *row_ptr, int64_t window, int threads);
// every row's entries stably sorted by feature id (the ALS learner's q pass); dup: some row stores an id twice
struct SortedRows { std::vector<int32_t> scol; std::vector<double> sval; bool dup = false; };
template <typename FT>
SortedRows sort_rows_by_feature(int64_t n_rows, const int64_t *row_ptr, const int32_t *col, const FT *val, int threads);

// ---- one batch's metadata from its column offsets --------------------------------------------------------------
struct HostBatch {
    std::vector<int32_t> cfeat, cptr, range_seg, split_seg, split_short, cdst, mp_feat, mp_ptr;
    int32_t n_feats = 0, n_pieces = 0;
};
// cfeat / cptr given: the column open at the start of every 64-entry range, the columns whose sum k_fixup assembles (short: up
// to 8 ranges, else long), the destination of every column piece.  cnt / base: zeroed scratch of dimension + 1 entries (left zeroed)
void finish_batch_meta(HostBatch &hb, int32_t nnz, std::vector<int32_t> &cnt, std::vector<int32_t> &base);
// per batch, dim / 32 + 1 words: the features whose gradient rows the fixup launch assembles (cut columns + live hot_ids)
std::vector<uint32_t> own_bitmaps(const std::vector<HostBatch> &hbs, const std::vector<int32_t> &hot_ids, int32_t dim);

// Band-affine placement of one batch's ranges (BwdArgs::xlist).  first/last: the rows of the first and last entry of every
// range.  -> the number of ranges placed by their band; lists[x] = XCD x's range ids, seg[x] = the runs of lists[x], each
// ascending (the INTERVAL form: a feature-interval launch clips every run to its window by binary search).
// order: how the free ranges (those no band claims) are dealt and in what order a whole-batch launch walks a list —
//   kWalkOrderStream     in blocks of 32 in stream order (hot features first) to the shortest list; walked as the runs stand
//   kWalkOrderColdFirst  in blocks of 32, the most expensive block first, to the list of least accumulated cost; a launch
//                        walks the free ranges in that order and the band runs after them
// walk (optional): walk[x] = list x in that WALK order (the same ranges as lists[x])
enum { kWalkOrderStream = 0, kWalkOrderColdFirst = 1 };
// cost of a range in units of 1 / kCostUnit entries: kCostUnit per entry + kCloseCost per column that closes inside it.  The
// walk takes 15.6 ns per 1,000 entries inside hot columns and 57 ns where every entry closes one (profiles/r05_experiments.md
// section 3): a close costs (57 - 15.6) / 15.6 = 2.65 entries
constexpr int64_t kCostUnit = 20, kCloseCost = 53;
int64_t range_cost(const HostBatch &hb, int32_t cnnz, int32_t rho);
int walk_order_default();     // kWalkOrderColdFirst unless FMHIP_BWD_ORDER names another
int32_t plan_bands(const HostBatch &hb, int32_t cnnz, int64_t rows, const std::vector<int32_t> &first, const std::vector<int32_t> &last,
                   std::vector<int32_t> (&lists)[kXcds], int32_t (&seg)[kXcds][kXSegs + 1], int order = kWalkOrderStream,
                   std::vector<int32_t> (*walk)[kXcds] = nullptr);

// ---- ALS level schedule (S/fm/lib/ALS.scala:36-70 walks the features in id order) ------------------------------
// level(c) = 1 + the largest level of an earlier column sharing a row with c.  crow: the transpose's row ids (bit 31 = a flag,
// masked off), cptr[nc + 1].  -> number of levels; lev_ptr[levels + 1], cols[nc] = columns sorted by (level, id)
int32_t als_levels(const std::vector<int32_t> &cptr, const uint32_t *crow, int64_t rows, std::vector<int32_t> &lev_ptr, std::vector<int32_t> &cols);

// ---- the data-parallel plan (fmhip_dp_plan, fmhip_comm.hip) ------------------------------------------------------
// cnt[n1]: stored nonzeros per feature.  cuts[i] = the id at or above which the share fractions[i] (ascending) of them lies, 0 = collapsed
void choose_cuts(const int32_t *cnt, int64_t n1, int n_fractions, const double *fractions, int64_t *cuts);
// interval edges {0, cuts inside (0, n1) ascending and distinct ..., n1}; W > 0: every cut rounded DOWN to a multiple of W first
std::vector<int64_t> interval_edges(const std::vector<int64_t> &cuts, int64_t n1, int W);
// the sharded update's equal shares: top = n1 rounded up to a multiple of W; rank R's share of [lo, hi_r) (hi_r = top for the top interval)
inline int64_t shard_top(int64_t n1, int W) { return (n1 + W - 1) / W * W; }
struct Share { int64_t hi_r, chunk, vlo, vhi; };
Share shard_share(int64_t lo, int64_t hi, bool top_interval, int64_t n1, int W, int R);
// the touched-rows exchange's intervals: feature ids [edge[i], edge[i+1]) (edge == interval_edges(cuts, n1, 0)) are the rows
// [pe[i], pe[i+1]) of the compact gradient; cut_pos[i]: where cuts[i] falls in the step's union of n_u rows
struct CompactEdges { std::vector<int64_t> edge, pe; };
CompactEdges compact_edges(const std::vector<int64_t> &cuts, int64_t n1, const int32_t *cut_pos, int32_t n_u);
// The update launches of the intervals [edges[i], edges[i+1]) as their slices arrive, first_interval down to 0: an interval
// of less than an eighth of total_rows waits and shares the next one's launch; interval 0 always launches.  -> one group per
// launch, in that order: the rows [lo, hi) and the interval `at` whose arrival it waits for
struct ApplyGroup { int at; int64_t lo, hi; };
std::vector<ApplyGroup> apply_groups(const std::vector<int64_t> &edges, int64_t total_rows, int first_interval);

// ---- the split step's backward window (fmhip_step_backward; StepState, fmhip_internal.h) -------------------------------
// Which of the two ranges that straddle a feature interval's edges a step_backward call walks: a straddling range belongs to
// whichever of its two intervals is walked FIRST (the other one's fixup then finds its partials).  Descending calls own their
// lower edge, ascending calls their upper one; a schedule that mixes the orders says so per call.
enum { kOwnLower = 1, kOwnUpper = 2 };
// The caller's intervals tile [0, n1) in DESCENDING order (a range straddling two intervals is walked with the upper one, whose
// partials the lower one's fixup then reads) or, from feature 0 up, in ASCENDING order (the mirror rule); the first call after
// the forward says which: it ends at n1 (or beyond) or starts at 0.  next: -1 = closed (no forward, or the tiling is complete),
// INT64_MAX = open and no interval walked yet, else the edge the next interval must end at (up: start at)
struct BwWindow {
    int64_t next = -1;
    bool up = false;
    static BwWindow opened() { return BwWindow{INT64_MAX, false}; }
    bool closed() const { return next < 0; }
    bool operator==(const BwWindow &o) const { return next == o.next && up == o.up; }
};
enum class BwRefusal { kNone, kClosed, kFinishAboveZero, kNotAscending, kNotDescending };
// the interval [lo, hi) (0 <= lo <= hi, checked by the caller; finish: it carries the step's statistics) against window w: accepted
// (refusal kNone) with the straddling ranges it owns and the window after it, or refused — `next` is then w itself
struct BwVerdict {
    BwRefusal refusal;
    int64_t want, got;      // kNotAscending / kNotDescending: the edge the window expected and the caller's
    int own;
    BwWindow next;
};
BwVerdict bw_window_step(BwWindow w, int64_t n1, int64_t lo, int64_t hi, bool finish);
std::string bw_refusal_text(const BwVerdict &v);      // fmhip_step_backward's error message for a refusal

// ---- ranking metrics of given ranks (fmhip_rank_metrics, include/fmhip_ranking.h) ------------------------------------
// ranks[rel_ptr[c] .. rel_ptr[c+1]) are the 0-based ranks of context c's relevant rows; the metrics are cut at k >= 1 and
// averaged (fp64 sums in context order) over the contexts that have a relevant row.  The caller has checked k, rel_ptr (not
// NULL when n_contexts > 0, non-negative, non-decreasing) and rank (not NULL when there are ranks).
struct RankMetricSums {
    int64_t contexts = 0, skipped = 0, relevant = 0;
    double hit_rate = 0, recall = 0, precision = 0, ndcg = 0, mrr = 0, map = 0;
};
// -> -1, or the first context that holds a negative rank or two equal ranks (out is then unreliable)
int64_t rank_metrics(int64_t n_contexts, const int64_t *rel_ptr, const int32_t *rank, int32_t k, RankMetricSums *out);

// ---- relational data (fmhip_relational_create, include/fmhip_relational.h) ---------------------------------------------
// -> -1, or the first row whose mapping entry lies outside [0, block_rows)
int64_t relational_bad_mapping(int64_t n_rows, const int32_t *map, int64_t block_rows);
// The parts' feature lists (any order, repeats inside a part allowed, ids outside [0, dimension] skipped) must be pairwise
// disjoint.  -> feature = -1, or the LOWEST feature id two parts share with the two lowest parts (a < b) that hold it
struct SharedFeature { int32_t feature = -1; int a = -1, b = -1; };
SharedFeature first_shared_feature(int n_parts, const int32_t *const *feat, const int64_t *n_feat, int64_t dimension);
// The inverse map of ONE relation, batch after batch (append_batch in batch order): per batch the block rows it touches,
// ascending (tj), and for each the batch-local rows that point at it, ascending (trow [tptr[t], tptr[t+1])) — a counting sort.
// Beside it the segmented sum's work list: a list of up to `cut` rows is ONE item whose sum is the block row's (wdst = the block
// row); a longer one is cut into chunks of `cut` rows (wdst = -1 - its partial row) plus one second-pass entry (lt: the touched
// index, lfirst / lcount: its partial rows).  Everything is O(rows + touched): nothing is sized by batches x block rows.
// All offsets inside a batch's slices are relative to the slice (Batch: where the slices start).
struct RelationInverse {
    struct Batch {
        int64_t row_off = 0, t_off = 0, tptr_off = 0, w_off = 0, l_off = 0;
        int32_t n_touched = 0, n_work = 0, n_long = 0, n_part = 0;
    };
    std::vector<int32_t> trow, tj, tptr, wt, wbeg, wdst, lt, lfirst, lcount;
    std::vector<Batch> batches;
    int32_t max_part = 0;
    // map: the batch's `rows` entries, all in [0, block_rows) (checked by the caller); count: scratch, zeroed or empty, left zeroed
    void append_batch(const int32_t *map, int64_t rows, int64_t block_rows, int32_t cut, std::vector<int32_t> &count);
};

// ---- the BPR trainer (fmhip_bpr_create, include/fmhip_bpr.h) ---------------------------------------------------------------------
// The contexts' positives from the interactions (any order, repeats allowed; every entry inside its block: checked by the caller):
// ptr[n_ctx + 1], rows = the lists one after the other, each ascending and distinct — what _ffi.row_lists builds in Python.
void bpr_positive_lists(int64_t n_ctx, int64_t n_inter, const int32_t *inter_ctx, const int32_t *inter_cand, std::vector<int64_t> &ptr,
                        std::vector<int32_t> &rows);
// The negative row of pair p at epoch t: the host twin of k_bpr_sample (rng::negative_row, mcmc_rng.h — the same integer code, so
// the two agree bit for bit).  list: the context's positives (ascending, distinct, len < M).  attempts / forced: nullable
int32_t bpr_negative(uint64_t seed, uint32_t p, uint32_t t, int32_t M, const int32_t *list, int32_t len, int *attempts, int *forced = nullptr);
// Candidate c = 0 .. 63 of the adaptive sampler (include/fmhip_bpr_adaptive.h): the same rule with the counter's group word
// offset by c << 4 — the host twin of k_bpr_sample_walk's draws.  bpr_negative is its c = 0 case.
int32_t bpr_candidate(uint64_t seed, uint32_t p, uint32_t c, uint32_t t, int32_t M, const int32_t *list, int32_t len, int *attempts,
                      int *forced = nullptr);

// The weighted proposal (include/fmhip_proposal.h).  The alias table of M weights by Vose's method in fp64, in a stated order so
// that a Python twin gives the same entries: S = the sum of the weights, index ascending; q_i = w_i / S * M; the small list holds
// the i with q_i < 1 and the large list the others, both index-ascending, both used as stacks (the last entry is taken first).
// While neither is empty: l = small's last, g = large's last, both taken off; bucket l = {floor(q_l * 2^32) clamped to
// 2^32 - 1, g}; q_g = (q_g + q_l) - 1; g goes onto small if q_g < 1, else back onto large.  What is left on either list keeps
// its own row: {2^32 - 1, itself}.  -> -1, or the first row whose weight is not finite and > 0, or -2 when S overflows (out is
// then not written).
int64_t bpr_alias_table(int64_t M, const double *weights, rng::AliasEntry *out);
// The sampled softmax's log-Q table (include/fmhip_softmax.h): out[i] = (float)log(w_i / S) in fp64, S as above.  weights: M doubles
// that bpr_alias_table has accepted (finite, > 0, a finite sum), so every out[i] is finite and <= 0.
void bpr_log_proposal(int64_t M, const double *weights, float *out);
// Candidate c of pair p under the table: the host twin of the weighted kernels' draws (rng::proposal_row, group0 = c << 4)
int32_t bpr_proposal_candidate(uint64_t seed, uint32_t p, uint32_t c, uint32_t t, int32_t M, const rng::AliasEntry *tab, const int32_t *list,
                               int32_t len, int *attempts, int *forced = nullptr);

// WARP (include/fmhip_warp.h).  The weight table: out[0] = 0 and, for n = 1 .. C, out[n] = (float)H(max(1, (M - 1) / n)) with
// H(r) = sum_{j = 1 .. r} 1 / j in fp64, j ascending — one pass over j = 1 .. M - 1 for all n.  out: C + 1 floats; M >= 2, C >= 1.
void warp_weight_table(int64_t M, int C, float *out);
// N of a pair: 1 + the lowest c in [0, C) with scores[c] > s_pos - margin (one fp32 subtraction; a strict test, so a tie and a NaN
// on either side are no violation), 0 when there is none — the host twin of the walk's FirstViolator rule.
int warp_first_violator(const float *scores, int C, float s_pos, float margin);

// ---- the MCMC learner's draws (fmhip_mcmc_epoch, include/fmhip_mcmc.h; the generator: mcmc_rng.h) ------------------------------
// Counters are (index, group, t, stream); t = the epochs the handle has completed.
double mcmc_uniform(uint64_t seed, uint32_t index, uint32_t group, uint32_t t, uint32_t stream);
double mcmc_normal(uint64_t seed, uint32_t index, uint32_t group, uint32_t t, uint32_t stream);
// Gamma(shape, rate) by Marsaglia-Tsang without the squeeze: attempt j takes the normal of index 2j and the uniform of index
// 2j + 1 of (group, t, stream).  A shape below 1 draws shape + 1 and scales by uniform(index 2^32 - 1)^(1 / shape).
// attempts (nullable): how many attempts the draw took.  shape, rate > 0 and finite (checked by the caller)
double mcmc_gamma(uint64_t seed, uint32_t group, uint32_t t, uint32_t stream, double shape, double rate, int *attempts);
// libFM's hyper-priors: alpha ~ Gamma(alpha_0 / 2, beta_0 / 2), lambda_g ~ Gamma(alpha_lambda / 2, beta_lambda / 2),
// mu_g ~ N(mu_0, 1 / (gamma_0 lambda_g))
struct McmcPriors { double alpha_0 = 1, beta_0 = 1, alpha_lambda = 1, beta_lambda = 1, gamma_0 = 1, mu_0 = 0; };
// nullptr, or the name of the first setting that is not finite and > 0 (mu_0: finite; reg0: finite and >= 0)
const char *mcmc_bad_setting(const McmcPriors &p, double reg0, double init_lambda);
// alpha ~ Gamma((alpha_0 + N) / 2, rate (beta_0 + sse) / 2), sse = the sum of the squared residuals of the N rows
double mcmc_draw_alpha(uint64_t seed, uint32_t t, const McmcPriors &p, int64_t n_rows, double sse);
// group g's regulariser and mean from its m trained parameters: sum_theta = sum theta_i, sum_dev2 = sum (theta_i - mu_old)^2.
// lambda ~ Gamma((alpha_lambda + m + 1) / 2, rate (beta_lambda + sum_dev2 + gamma_0 (mu_old - mu_0)^2) / 2), then with it
// mu ~ N((sum_theta + gamma_0 mu_0) / (m + gamma_0), 1 / ((m + gamma_0) lambda)) = mean + z / sqrt((m + gamma_0) lambda)
void mcmc_draw_group(uint64_t seed, uint32_t t, uint32_t g, const McmcPriors &p, int64_t m, double sum_theta, double sum_dev2, double mu_old,
                     double *lambda, double *mu);
// One epoch's hyper-parameter draws, for every kind of handle: alpha (unless probit: the link keeps what the state holds), then
// lambda and mu of every (parameter group g < k1, attribute group a < G) at [g * G + a], stream id g + (a << 16).
// count_of(a) = m_a; partials_of(g, a, add) calls add(sum theta, sum (theta - mu_old)^2) once per partial pair of (g, a), in the
// order they are to be added (none: the draw from the prior).
template <class CountOf, class PartialsOf>
void mcmc_draw_state(uint64_t seed, uint32_t t, const McmcPriors &p, bool probit, int64_t n_rows, double sse, int k1, int G, CountOf count_of,
                     PartialsOf partials_of, double *alpha, double *lambda, double *mu) {
    if (!probit) *alpha = mcmc_draw_alpha(seed, t, p, n_rows, sse);
    for (int g = 0; g < k1; ++g)
        for (int a = 0; a < G; ++a) {
            double sum_theta = 0.0, sum_dev2 = 0.0;
            partials_of(g, a, [&](double theta, double dev2) {
                sum_theta += theta;
                sum_dev2 += dev2;
            });
            const size_t at = (size_t)g * (size_t)G + (size_t)a;
            mcmc_draw_group(seed, t, (uint32_t)g + ((uint32_t)a << 16), p, count_of(a), sum_theta, sum_dev2, mu[at], &lambda[at], &mu[at]);
        }
}
// ---- ... its attribute groups (include/fmhip_mcmc_groups.h) ----
constexpr int kMcmcMaxGroups = 4096;        // FMHIP_MCMC_MAX_GROUPS
constexpr int kMcmcGroupChunk = 512;        // column slots per chunk of k_mcmc_group_sums (a workgroup each)
// -1, or the first feature i < n whose id group[i] lies outside [0, n_groups)
int64_t mcmc_bad_group(const int32_t *group, int64_t n, int32_t n_groups);
// The plan of the grouped hyper-parameter sums: the TRAINED column slots (cfeat[s] < num_attribute) in a stable order by group —
// slots of one group keep their ascending order — cut into chunks of at most chunk_slots slots that never straddle a group.
//   order[chunk_ptr[c] .. chunk_ptr[c + 1]): the slots of chunk c, all of group chunk_group[c]; chunks sit in group order and
//   group a's are [group_chunks[a], group_chunks[a + 1]) (none for a group without a trained slot); counts[a] = m_a.
// group: num_attribute ids, each in [0, n_groups) (checked by the caller: mcmc_bad_group)
struct McmcGroupPlan {
    std::vector<int32_t> order, chunk_ptr, chunk_group, group_chunks;
    std::vector<int64_t> counts;
};
void mcmc_group_plan(const int32_t *cfeat, int64_t n_cols, int64_t num_attribute, const int32_t *group, int32_t n_groups, int chunk_slots,
                     McmcGroupPlan *plan);
// ---- the SGDA learner's plan (include/fmhip_sgda.h): the same construction over ALL n feature rows (row i is its own slot) —
// order holds feature ids, ascending inside a group; counts[a] = the features of group a; an empty group has no chunk.
// group: n ids, each in [0, n_groups) (checked by the caller: mcmc_bad_group)
constexpr int kSgdaMaxGroups = 4096;        // FMHIP_SGDA_MAX_GROUPS
constexpr int kSgdaChunk = 128;             // feature rows per chunk of k_sgda_lambda_partials (a workgroup each: 100 k rows give 782, three per CU)
void sgda_group_plan(const int32_t *group, int64_t n, int32_t n_groups, int chunk_rows, McmcGroupPlan *plan);
// ---- ... and its tasks (include/fmhip_mcmc_task.h) ----
// the probit link's latent draw of a row: z ~ N(0,1) given z > a, counter (row, attempt, t, stream 5); attempts: nullable
double mcmc_truncated_normal(uint64_t seed, uint32_t row, uint32_t t, double a, int *attempts);
// ... and its expectation E[z | z > a] (the epoch without sampling)
double mcmc_truncated_mean(double a);
// nullptr, or why (task, clip, [clip_lo, clip_hi]) is refused: an unknown task, a clip with the classification task, a clip
// range that is not finite with lo < hi
const char *mcmc_bad_task(int32_t task, int32_t clip, double clip_lo, double clip_hi);
// ---- ... and its block-structure sweep over relational data (include/fmhip_mcmc_relational.h) ----
// The order the parts are walked in: by ascending id range.  feat[p]: part p's feature ids (any order, repeats allowed; a part
// without features keeps its place).  The flat sweep walks ascending ids, so the ranges must not interleave: a = -1, or the two
// parts (a's range starts lower) and the lowest feature of b that lies inside a's range
struct McmcPartOrder {
    std::vector<int> order;
    int a = -1, b = -1;
    int32_t feature = -1;
};
McmcPartOrder mcmc_part_order(int n_parts, const int32_t *const *feat, const int64_t *n_feat);
// n[j] = the data rows that map to block row j (map: n_rows entries in [0, block_rows), checked by the caller)
void mcmc_block_counts(const int32_t *map, int64_t n_rows, int64_t block_rows, std::vector<double> &n);
// trained[s] = 1 when column s is in T — its id below num_attribute (quirk Q1) and an entry in a block row with n[j] > 0 (crow:
// the CSC row words, bit 31 a flag; n = NULL: the plain part, every row counts) -> |T| of the part
int64_t mcmc_block_trained(const int32_t *cfeat, const int32_t *cptr, const uint32_t *crow, int64_t n_cols, int64_t num_attribute, const double *n,
                           std::vector<int32_t> &trained);

}  // namespace host
}  // namespace fmhip
