// fmhip_internal.h — host-side state behind the opaque handles of include/fmhip.h / fmhip_experimental.h, shared by the
// translation units of libfmhip.so (fmhip_api.hip: the C ABI of models and training; fmhip_score.hip: of scoring;
// fmhip_dataset.hip: datasets; fmhip_step.hip: the single-GPU step in pieces; fmhip_comm.hip: the data-parallel step).
// Not installed, not part of the ABI.
#pragma once
#include "../../include/fmhip_experimental.h"   // (includes fmhip.h: the library implements both surfaces)
#include "../../include/fmhip_pairing.h"        // (enum fmhip_pairing: the model carries the switch)
#include "../../include/fmhip_relational.h"     // (fmhip_relational_t: the handle's state is declared below)
#include "../../include/fmhip_bpr.h"            // (fmhip_bpr_t: likewise)
#include "../../include/fmhip_ftrl.h"           // (FMHIP_OPT_FTRL: the third value a model's rule reports)
#include "fm_kernels.h"
#include "fm_pairing.h"      // (PairArgs, RelFinishArgs: the builders the step and the scoring pass share are declared below)
#include "fm_relational.h"
#include "fm_softmax.h"      // (SoftmaxArgs: the pre-pass the BPR trainer's softmax step and its scoring pass share)
#include "fmhip_host.h"   // the pure host arithmetic (shards, relabelling, batch metadata, band plan, ALS levels, the dp plan's cuts and shares)

#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstring>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <vector>

namespace fmhip {
struct AlsArgs;     // als_kernels.h
struct ColumnPlan;
namespace host {

// records the calling thread's error message (fmhip_last_error) and returns `code`
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

#define HIP_TRY(expr)                                                                        \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess)                                                                \
            return fail(_e == hipErrorOutOfMemory ? FMHIP_ERR_NOMEM : FMHIP_ERR_HIP,         \
                        "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

#define TRY(expr)               \
    do {                        \
        int _r = (expr);        \
        if (_r != FMHIP_OK) return _r; \
    } while (0)

template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    int alloc(size_t count) {
        release();
        if (count == 0) return FMHIP_OK;
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&p), count * sizeof(T));
        if (e != hipSuccess) {
            p = nullptr;
            return fail(FMHIP_ERR_NOMEM, "hipMalloc(%zu bytes) failed: %s", count * sizeof(T), hipGetErrorString(e));
        }
        n = count;
        return FMHIP_OK;
    }
    int ensure(size_t count) { return count <= n ? FMHIP_OK : alloc(count); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    ~DevBuf() { release(); }
};

constexpr int64_t kAlsMaxNnz = (int64_t)1 << 27;

struct BatchMeta {
    int64_t row0 = 0, rows = 0;
    int64_t nnz0 = 0;   // offset of the batch in the global CSR/CSC entry arrays
    int32_t nnz = 0;        // entries of the batch in the CSR stream (what the forward walks)
    int32_t cnnz = 0;       // ... in the CSC stream (<= nnz: the gradient-side hot pages' entries are not in it)
    int32_t n_cols = 0;     // compressed columns (features present in the batch)
    int64_t col_off = 0;    // offset into cfeat; cptr offset is col_off + batch index
    int32_t n_ranges = 0;
    int64_t range_off = 0;
    int32_t n_split = 0;          // cut columns spanning > 8 ranges
    int64_t split_off = 0;
    int32_t n_split_short = 0;    // cut columns spanning <= 8 ranges
    int64_t split_short_off = 0;
    int32_t n_feats = 0;    // distinct features present (== n_cols unless the stream is row-blocked)
    int32_t n_mp = 0;       // features cut into several pieces (one per row block they occur in)
    int64_t mp_off = 0;     // offset into mp_feat; mp_ptr offset is mp_off + batch index
    int32_t n_pieces = 0;   // piece rows those features need
    int64_t nnz_total = 0;  // stored nonzeros of the batch incl. those held in the dense hot block
    unsigned __int128 hot_mask = 0;  // hot slots (all pages: up to 128) with at least one nonzero in this batch
    int64_t own_off = -1;   // offset (in words) of the batch's bitmap of fixup-owned features, -1 = none
    // band-affine placement of the backward's ranges (fmhip_dataset.hip: plan_bands): per XCD a list of range ids, the
    // ranges of its own row bands first; xoff[x] = offset of list x in fmhip_dataset::xlist, -1 = no plan for this batch
    int64_t xoff[fmhip::kXcds] = {-1, -1, -1, -1, -1, -1, -1, -1};
    int32_t xlen[fmhip::kXcds] = {};
    int32_t xseg[fmhip::kXcds][fmhip::kXSegs + 1] = {};   // list x = runs [xseg[x][s], xseg[x][s+1]) of ascending range ids (one per band, then the rest)
    int32_t x_affine = 0;   // ranges that were placed by their band (the rest fill the lists evenly)
    int64_t woff[fmhip::kXcds] = {};   // list x once more in WALK order (plan_bands), xlen[x] ids from here: what a whole-batch launch reads
};

// Where a backward delivers its gradient rows when NOT into the model's packed buffer: the touched-rows exchange
// (fmhip_comm.hip) points the column walk at a compact buffer that holds one row per feature of the step's union
struct GradView {
    float *scal, *Gw, *Gb, *GV;
    const int32_t *cdst;       // per compressed column of the batch: its row in GV / Gw / Gb
    const int32_t *hot_pos;    // per slot of the dense hot block: its row (-1 = unused slot)
};

// What a mini-batch step carries from one of its pieces to the next (forward -> backward intervals -> [exchange] -> update), and
// the ONLY place that writes it: every route moves it through the transitions below ("The step's state").
struct StepState {
    // where this step's gradient rows go: the model's packed gradient (nullptr), or a compact view for the length of a ViewScope
    const GradView *view = nullptr;
    bool grad_dirty = false;      // the PACKED gradient holds a gradient that has not been applied/zeroed
    bool hot_pending = false;     // the dense hot block's gradient of the current step is still to be formed
    BwWindow bw;                  // the feature intervals fmhip_step_backward may still walk
    int64_t last_nnz = 0, last_rows = 0;
    int fwd_parts = 0;            // per-block statistic partials the last forward launch wrote

    // The touched-rows exchange sets its compact buffer as the step's target ONCE: under it no transition cleans or dirties the
    // packed gradient — a gradient pending from fmhip_step_compute is still there, and still to be applied, afterwards
    struct ViewScope {
        StepState &s;
        ViewScope(StepState &s_, const GradView *v) : s(s_) { s.view = v; }
        ~ViewScope() { s.view = nullptr; }
        ViewScope(const ViewScope &) = delete;
    };
    // forward begins: must the target be zeroed first?  Never a view (its rows are clean after every update) — and the packed
    // gradient is not written by such a step: a pending memset of it (8.9 GB at C5's width) would be wasted
    bool must_zero() const { return !view && grad_dirty; }
    // the target holds this step's contribution (a forward's rows to come, or a rank's zeros): what fmhip_step_stats reports
    void written(int64_t nnz, int64_t rows) {
        if (!view) grad_dirty = true;
        last_nnz = nnz;
        last_rows = rows;
    }
    // forward done: + the backward window opens and the hot block is armed (hot: the dataset has one)
    void forward_done(int64_t nnz, int64_t rows, bool hot) {
        written(nnz, rows);
        bw = BwWindow::opened();
        hot_pending = hot;
    }
    // the relational step arms the block per part (each part's whole-batch backward consumes it) and leaves it disarmed
    void arm_hot(bool hot) { hot_pending = hot; }
    void hot_formed() { hot_pending = false; }
    void backward_walked(const BwWindow &next) { bw = next; }     // fmhip_step_backward: one accepted interval
    void backward_over() { bw = BwWindow{}; }                     // an exchange mode walked its own intervals
    // the target's gradient is applied — or the packed buffer zeroed, or a fresh one bound (no view is set in those calls)
    void grad_consumed() { if (!view) grad_dirty = false; }
};

// How a model trains, as ONE value: the residual every training path forms (enum fmhip_loss), whether rows 2j / 2j+1 of a
// batch are one example with the loss applied to their difference (enum fmhip_pairing; fm_pairing.h — the training forward
// then runs in two launches and keeps the rows' predictions in yhat), and the update rule with its settings (enum
// fmhip_optimizer).  The three setters of the C ABI write it, fmhip_dp_plan agrees it over the ranks and keeps a copy, a
// step compares the model's with the plan's; a path that cannot train under a rule says so through refusal().
struct TrainRule {
    int loss = FMHIP_LOSS_SQUARED;
    int pairing = FMHIP_PAIRING_NONE;
    int opt = FMHIP_OPT_SGD;
    double ada_eps = 0.0, ada_init = 0.0;
    // FMHIP_OPT_FTRL (fmhip_ftrl.h; set by fmhip_model_set_ftrl only): beta, the accumulators' initial value, the L1 of w and of V
    double ftrl_beta = 0.0, ftrl_init = 0.0, ftrl_l1w = 0.0, ftrl_l1v = 0.0;
    bool adagrad() const { return opt == FMHIP_OPT_ADAGRAD; }
    bool ftrl() const { return opt == FMHIP_OPT_FTRL; }
    bool paired() const { return pairing != FMHIP_PAIRING_NONE; }
    // the settings by bit pattern (what the ranks agree on is their bits, and -0.0 or a NaN must not compare by value)
    bool same_optimizer(const TrainRule &o) const {
        auto same = [](const double &a, const double &b) { return memcmp(&a, &b, sizeof a) == 0; };
        return opt == o.opt && same(ada_eps, o.ada_eps) && same(ada_init, o.ada_init) && same(ftrl_beta, o.ftrl_beta) &&
               same(ftrl_init, o.ftrl_init) && same(ftrl_l1w, o.ftrl_l1w) && same(ftrl_l1v, o.ftrl_l1v);
    }
    bool operator==(const TrainRule &o) const { return loss == o.loss && pairing == o.pairing && same_optimizer(o); }
};

// The training paths that refuse some rule, and the sentence each (path, rule) pair is refused with — nullptr: the path trains
// under the rule.  The error code is FMHIP_ERR_UNSUPPORTED everywhere.  kTouchedDecay is the touched-rows exchange on a step WITH
// weight decay (without, it takes every rule).  ALS is derived for the default loss and pairing only.
// `weighted`: the dataset carries per-row example weights (include/fmhip_weights.h) — their residual is formed by a finish behind the
// q-mode forward, which the two-pass forward (and so the pipelined exchange) does not have; ALS is derived for unweighted rows.
// kRelational: the relational step (include/fmhip_relational.h) — single rows, unweighted parts.
enum class Path { kSharded, kTouchedDecay, kPipelined, kTwoPass, kAls, kRelational };
inline const char *refusal(Path p, const TrainRule &r, bool weighted = false) {
    if (weighted) switch (p) {
        case Path::kPipelined:
            return "the pipelined exchange runs the two-pass forward, which does not form weighted residuals (some rank's dataset "
                   "carries example weights, fmhip_dataset_create_weighted): use the dense, sharded or touched exchange";
        case Path::kTwoPass:
            return "the two-pass forward does not form weighted residuals (the dataset carries example weights, "
                   "fmhip_dataset_create_weighted): use fmhip_step_forward, and the dense, sharded or touched exchange";
        case Path::kAls:
            return "ALS is derived for the squared loss of unweighted rows: the dataset carries example weights "
                   "(fmhip_dataset_create_weighted)";
        case Path::kRelational:
            return "relational data does not take example weights yet (a block or the plain part was made by "
                   "fmhip_dataset_create_weighted): one weight per data row would scale e_r before the segmented sum";
        default: break;
    }
    switch (p) {
        case Path::kSharded:
            if (r.ftrl())
                return "the sharded exchange does not support FTRL-Proximal (each rank's zeta and accumulators would hold its own "
                       "share only): use the dense, pipelined or touched exchange";
            return !r.adagrad() ? nullptr
                                : "the sharded exchange does not support AdaGrad (each rank's accumulators would hold its own share "
                                  "only): use the dense, pipelined or touched exchange";
        case Path::kTouchedDecay:      // (FTRL: accepted — its L2 is no decay, a row without a gradient does not move)
            return !r.adagrad() ? nullptr
                                : "the touched-rows exchange under AdaGrad needs regw = regv = 0 (with decay every row moves: use the "
                                  "dense or pipelined exchange)";
        case Path::kPipelined:
            return !r.paired() ? nullptr
                               : "the pipelined exchange runs the two-pass forward, which does not form pair residuals "
                                 "(fmhip_model_set_pairing): use the dense, sharded or touched exchange";
        case Path::kTwoPass:
            return !r.paired() ? nullptr
                               : "the two-pass forward does not form pair residuals (fmhip_model_set_pairing): use fmhip_step_forward, "
                                 "and the dense, sharded or touched exchange";
        case Path::kAls:
            if (r.loss != FMHIP_LOSS_SQUARED)
                return "ALS is derived for the squared loss: this model trains under the logistic loss (fmhip_model_set_loss)";
            return !r.paired() ? nullptr
                               : "ALS is derived for the squared loss of single rows: this model trains on pairs of rows "
                                 "(fmhip_model_set_pairing)";
        case Path::kRelational:
            return !r.paired() ? nullptr
                               : "the relational step forms single rows' residuals: this model trains on pairs of rows "
                                 "(fmhip_model_set_pairing) — expand the data and train the pairs on the flat dataset";
    }
    return nullptr;
}

struct ProfRec {
    int kind;
    hipEvent_t a, b;
    int64_t nnz, rows;
    int64_t step;       // the step (fmhip_model::prof_step) the launch belongs to
};

// What ONE scoring call (every entry point of fmhip_score.hip that takes a model) works in: its own stream and workspace, so
// that any number of host threads may score through one frozen model at once (the reference's `predict` runs on executor task
// threads over a read-only model, S/Model.scala:14 under `local[*]`, S/driver.scala:14).  Pooled per model; a call takes a free
// one or makes one (fmhip_score.hip: ScoreLease, inside ScorePass).
struct ScoreCtx {
    hipStream_t s = nullptr;
    hipEvent_t ev = nullptr;        // orders the call behind what the model's own stream has queued (an asynchronous step)
    DevBuf<float> P, e, yhat;
    DevBuf<double> bsum, acc;
    ~ScoreCtx() {
        if (ev) (void)hipEventDestroy(ev);
        if (s) (void)hipStreamDestroy(s);
    }
};

}  // namespace host
}  // namespace fmhip

struct fmhip_dataset {
    using BatchMeta = fmhip::host::BatchMeta;
    template <typename T> using DevBuf = fmhip::host::DevBuf<T>;
    int device = 0;
    int64_t n_rows = 0, nnz = 0, dimension = 0, batch_rows = 0;
    int64_t max_rows = 0;
    int32_t max_ranges = 0;
    std::vector<BatchMeta> batches;
    DevBuf<int64_t> row_ptr;
    DevBuf<int32_t> col;
    DevBuf<float> val, y;
    // per-row example weights (include/fmhip_weights.h; the rule: fm_weights.h): fp32 like y, finite and >= 0; weight_sum: their
    // fp64 sum in row order, of the values as stored.  Not weighted: no array, and every path is the one it always was
    DevBuf<float> c;
    bool weighted = false;
    double weight_sum = 0.0;
    DevBuf<uint32_t> crow;
    DevBuf<float> cval;
    DevBuf<int32_t> row_order;   // per batch: its rows' local ids sorted by stored length, longest first (forward walk order)
    // two-pass forward (fmhip_dataset_partition_rows): every row's stored entries stably partitioned at feature id
    // split_cut — [row_ptr[r], row_split[r]) hold the features below it, [row_split[r], row_ptr[r+1]) the others
    DevBuf<int64_t> row_split;
    int64_t split_cut = -1;      // -1: not partitioned
    // ... in a COPY of the CSR stream that only the two-pass forward reads (col / val themselves never move once the dataset
    // is built: other threads may be scoring or training with them).  part_mu guards the partition's making; part_users counts
    // the pipelined runs that are walking it (it is not re-made for another cut while one does)
    DevBuf<int32_t> col_part;
    DevBuf<float> val_part;
    std::mutex part_mu;
    int part_users = 0;
    int32_t hot0_max_id = -1;    // the largest feature id of the dense hot block's FORWARD page (page 0), -1 = none
    DevBuf<int32_t> cfeat, cptr, range_seg, split_seg, split_short, cdst, mp_feat, mp_ptr;
    // per batch: bitmap over the feature ids [0, dimension] of the rows whose gradient the FIXUP launch assembles (cut
    // columns, hot block) — the merged finish lets those update themselves and skips them in its dense pass
    DevBuf<uint32_t> own_bits;
    int64_t own_words = 0;       // words per batch
    DevBuf<int32_t> xlist;       // band-affine range lists of all batches (BatchMeta::xoff)
    std::vector<int32_t> h_xlist;   // host copy (a feature-interval launch searches the runs for its range window)
    std::vector<int32_t> h_cfeat, h_cptr, h_split, h_split_short;   // host copies (feature-chunked backward needs them)
    int64_t rb_rows = 0;       // rows per row block of the transposes (0 = not row-blocked)
    int32_t max_pieces = 0;
    // dense hot block: the entries of the most frequent features are held as dense [n_rows][kHotT] fp32 pages
    // (0 where the feature is absent).  Page 0 (up to kHotT features) is out of both sparse streams; pages 1.. are out
    // of the CSC stream only (fm_constants.h, kHotPages)
    int32_t hot_T = 0;                 // 0 = no hot block
    int32_t hot_pages = 0;             // pages in use (0 = no hot block)
    int64_t hot_max_id = -1;           // the largest feature id held in any page
    std::vector<int32_t> hot_ids;      // [hot_pages * kHotT] feature id per slot, -1 = unused slot
    DevBuf<float> xhot;                // [hot_pages][n_rows][kHotT]
    DevBuf<int32_t> d_hot_ids;
    int64_t nnz_sparse = 0;            // entries of the CSR stream
    int64_t nnz_sparse_bwd = 0;        // entries of the CSC streams
    bool scoring_only = false;   // rows + labels only (fmhip_rows_create): no transposes, cannot train
    // fp64 copies of the values (CSR order, CSC order) and labels for the fp64 ALS learner; kept only
    // for single-batch datasets of at most kAlsMaxNnz stored nonzeros
    DevBuf<double> val64, cval64, y64;
    // ... and the rows with their entries sorted by feature id (the per-row order of the reference's transposed
    // q pass); als_dup: some row stores a feature twice (the column walk updates a row once per step: refused)
    DevBuf<int32_t> scol;
    DevBuf<double> sval64;
    bool als_dup = false;
    // level schedule of the ALS sweep (single-batch datasets): columns that share no row commute exactly, so the sweep may
    // take them side by side — level(c) = 1 + the largest level of an earlier column (smaller id) sharing a row with c.
    // als_lev_cols: the compressed columns sorted by (level, id); als_lev_ptr[l] .. [l + 1]: level l's slice of it
    DevBuf<int32_t> als_lev_cols;
    std::vector<int32_t> als_lev_ptr, h_als_lev_cols;
};

// A relational dataset (include/fmhip_relational.h): N labels, m relations (a borrowed block + a mapping + the inverse map of every
// batch), an optional borrowed plain part.  The training workspace (per relation: the block's q rows and predictions, P_b / e_b, the
// long lists' partial rows) lives here too: one training call per handle at a time; the scoring calls only read the handle.
struct fmhip_relational {
    template <typename T> using DevBuf = fmhip::host::DevBuf<T>;
    struct Relation {
        fmhip_dataset_t block = nullptr;
        DevBuf<int32_t> map;                                            // [n_rows]
        DevBuf<int32_t> trow, tj, tptr, wt, wbeg, wdst, lt, lfirst, lcount;      // fmhip::host::RelationInverse, on the device
        std::vector<fmhip::host::RelationInverse::Batch> batches;      // where every batch's slices start
        int32_t max_part = 0;
        DevBuf<float> Q, yq, Pb, eb, part, part_e;                      // training workspace (allocated by the first step)
    };
    struct Batch { int64_t row0 = 0, rows = 0; };
    int device = 0;
    int64_t n_rows = 0, batch_rows = 0, dimension = 0, max_rows = 0;
    int64_t block_nnz = 0;                                              // stored nonzeros of all blocks (what every step walks)
    std::vector<std::unique_ptr<Relation>> rels;
    fmhip_dataset_t plain = nullptr;
    DevBuf<float> y;
    DevBuf<double> y64;                                                 // the labels as given (the MCMC learner's residuals are fp64)
    std::vector<Batch> batches;
    // A step is queued, not run, when its call returns, and the workspace above is the HANDLE's: `busy` is recorded behind every
    // step on the stream it ran on, and a step on ANOTHER stream (another model) waits for it before it touches the workspace
    hipEvent_t busy = nullptr;
    hipStream_t busy_stream = nullptr;
    bool busy_set = false;
    ~fmhip_relational() {
        if (busy) (void)hipEventDestroy(busy);
    }
};

// A BPR trainer (include/fmhip_bpr.h): an OWNED relational dataset of 2 n_pairs rows over the two borrowed blocks — relation 0 the
// contexts (its inverse map built once on the host), relation 1 the candidates, whose mapping's odd entries the sampler rewrites
// and whose inverse map the device rebuilds (buffers at their worst case, the batches' counts read back once per resample) —
// the interactions' contexts and the contexts' positives on the device, and a stream of its own for the resample.  Under the
// per-batch redraw (include/fmhip_redraw.h) a batch's draw, inverse map and step are queued on the model's stream and the step reads
// the counts from the device: the host's copy (R->rels[1]->batches) is then stale until the next fetch.
struct fmhip_bpr {
    template <typename T> using DevBuf = fmhip::host::DevBuf<T>;
    int device = 0;
    fmhip_relational_t R = nullptr;
    int64_t n_inter = 0, n_pairs = 0, batch_pairs = 0, n_ctx = 0, M = 0;
    int32_t n_neg = 0;
    uint64_t seed = 0;
    DevBuf<int32_t> ictx, prow, counts;        // counts: [n_batches][4]
    DevBuf<int64_t> pptr;
    // the per-block partials and their sums [3] of the sampler that runs: a resample grows `part` to its sampler's need and ends in a
    // synchronise, so no two draws hold it at once
    DevBuf<unsigned long long> part, total;   // total: [n_batches][3], a slot per batch (a whole-set draw sums into slot 0)
    // the redraw mode (FMHIP_REDRAW_*), the batches whose host counts are older than the device's, and the sampler's counters
    // summed over the last per-batch epoch {pairs, attempts, forced, replaced, violated, trials}
    int redraw = 0;
    std::vector<char> stale;
    bool any_stale = false;
    bool have_epoch_draw = false;
    int64_t epoch_draw[6] = {0, 0, 0, 0, 0, 0};
    DevBuf<char> work;                         // the inverse build's workspace, for the largest batch
    hipStream_t stream = nullptr;
    // the adaptive sampler (include/fmhip_bpr_adaptive.h): candidates per pair, the debug call's record buffers, and the event that
    // puts the sampler (own stream) behind the blocks' forwards (the model's)
    int32_t n_cand = 1;
    DevBuf<int32_t> rec_rows;
    DevBuf<float> rec_scores;
    hipEvent_t fwd_done = nullptr;
    // WARP (include/fmhip_warp.h): the switch and the margin, whether a WARP draw stands since the switch was last set, the pairs'
    // weights (a PairArgs::c over all 2 n_pairs rows) and trial counts, the weight table W[0 .. wtab_cand] on both sides, the
    // debug call's s+ record
    bool warp = false, warp_drawn = false;
    std::vector<char> warp_have;               // per batch: a WARP draw stands since the switch was last set (all: warp_drawn)
    double warp_margin = 1.0;
    DevBuf<float> wc, wtab, rec_pos;
    DevBuf<int32_t> wtrials;
    std::vector<float> h_wtab;
    int32_t wtab_cand = 0;
    // the proposal (include/fmhip_proposal.h): uniform while h_ptab is empty, else the alias table of M entries on both sides
    DevBuf<fmhip::rng::AliasEntry> ptab;
    std::vector<fmhip::rng::AliasEntry> h_ptab;
    // the sampled softmax (include/fmhip_softmax.h): the switch and the log-Q request, the pairs' probabilities of each batch's
    // last step (a PairArgs::c over all 2 n_pairs rows) and which batches have had one since the switch was set, the pre-pass's
    // partials, the proposal's weights as given and — while the correction is in force — log(w_i / sum w) on both sides
    bool softmax = false, sm_logq = false;
    DevBuf<float> sm_pi, lq;
    DevBuf<double> sm_bsum;
    std::vector<char> sm_have;
    std::vector<double> h_pw;
    std::vector<float> h_lq;
    ~fmhip_bpr() {
        if (fwd_done) (void)hipEventDestroy(fwd_done);
        if (R) (void)fmhip_relational_destroy(R);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

struct fmhip_model {
    template <typename T> using DevBuf = fmhip::host::DevBuf<T>;
    using ProfRec = fmhip::host::ProfRec;
    static constexpr int kGradHead = fmhip::kGradHead;
    // rows allocated (and kept zero) behind row n1p of V and of the library's own packed gradient: the sharded exchange
    // (fmhip_comm.hip) cuts [0, n+1) into `world` equal shares, so its last share may reach up to world - 1 rows past n1p
    static constexpr int kSlackRows = 64;
    // Threading rule of the C ABI (include/fmhip.h): calls that CHANGE a model (parameters, training, tuning, gradient
    // buffer, profiling, the data-parallel step) hold `mu` exclusively; the scoring calls and the parameter reads hold it
    // shared and work in a ScoreCtx of their own — they run side by side and never beside a writer.
    std::shared_mutex mu;
    std::mutex pool_mu;                                             // guards the two lists below
    std::vector<std::unique_ptr<fmhip::host::ScoreCtx>> ctx_all;
    std::vector<fmhip::host::ScoreCtx *> ctx_free;
    int device = 0;
    int64_t n = 0, n1 = 0, n1p = 0;
    int32_t k = 0, Kp = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    DevBuf<float> V, w, w0;
    DevBuf<float> grad_own;
    float *grad = nullptr;        // packed gradient in use (own or bound)
    fmhip::host::StepState step;  // what the pieces of a mini-batch step hand on to each other
    DevBuf<float> P, e, part, pieces, hot_part;
    DevBuf<float> part_sl;        // two-pass forward: pass A's {sum_f s_f, linear term} per row
    DevBuf<double> acc;           // {sum e, sum e^2, rows, nonfinite}
    DevBuf<double> bsum;          // k_forward's per-block statistic partials
    // lazy weight decay (fm_apply.hip): the device tables hold U with V = sv*U, w = sw*(stored w); both are
    // exactly 1 unless rows-only updates with decay are pending.  Tracked in fp64 on the host, so the
    // scale itself accumulates no fp32 rounding from step to step.
    double sv = 1.0, sw = 1.0;
    fmhip::host::TrainRule rule;  // how the model trains (the three fmhip_model_set_* calls)
    int sgda_handles = 0;         // live SGDA handles (include/fmhip_sgda.h) over this model: fmhip_dp_plan refuses it while there is one
    DevBuf<float> yhat;           // paired or weighted training forward: [max_rows] predictions between its two launches
    // AdaGrad: per-coordinate accumulators shaped like the parameters — NV [n1p][Kp] like V (packed rows: slot pack_k holds
    // w_i's), Nw [n1p] (unpacked rows only), N0 [1] — one more copy of the model (8.6 GB at 2^25 x 64); the tables stay at
    // scale 1 (sv = sw = 1) while it is set
    DevBuf<float> NV, Nw, N0;
    // FTRL-Proximal: zeta = eta*z per parameter, shaped like the accumulators (which it shares: NV, Nw, N0 hold its n)
    DevBuf<float> ZV, Zw, Z0;
    // fp64 master copy of the parameters (reference layout): exact round trip of what the caller set,
    // and the state the fp64 ALS learner trains; stale once an fp32 SGD step has run
    std::vector<double> h_w, h_v;
    double h_w0 = 0.0;
    bool host64_fresh = false;
    DevBuf<double> als_w0, als_w, als_v, als_e, als_q, als_part;
    // per-model overrides of the tuning keys (fmhip_model_tune); -1 = the process-wide default (fmhip_tune) as it stands
    // at the time of the launch
    int tune[fmhip::kTuneCount];
    int tv(int key) const { return tune[key] >= 0 ? tune[key] : fmhip::tune_default(key); }
    bool profiling = false;
    bool prof_rotate = false;     // time one kernel kind per step, rotating
    int prof_period = 1;          // ... and only on every prof_period-th step
    int64_t prof_step = 0;
    std::vector<ProfRec> prof;

    // packed gradient: [ scalars (kGradHead floats, 8 used) | G_w (n1p) | G_b (n1p) | pad | G_V (n1p*Kp) ]: the
    // small head sits next to the G_V rows of the LOWEST feature ids, which the feature-chunked backward
    // finishes last, so a data-parallel host moves head + last interval in one collective
    size_t head_floats() const { return ((size_t)kGradHead + 2 * (size_t)n1p + 31) / 32 * 32; }
    float *scal() const { return grad; }
    float *Gw() const { return grad + kGradHead; }
    float *Gb() const { return grad + kGradHead + n1p; }
    float *GV() const { return grad + head_floats(); }
    int32_t pack_k() const { return k < Kp ? k : -1; }   // packed rows: slot k of a V row holds w_i
    size_t grad_floats() const { return head_floats() + (size_t)n1p * Kp; }
};


namespace fmhip {
namespace host {

extern thread_local std::string g_err;    // the calling thread's last error message (fmhip_api.hip)
int set_device(int device);
// the model's lock for the length of a C-ABI call (a NULL model is left to the call's own argument check)
struct WriteLock {
    std::unique_lock<std::shared_mutex> lk;
    explicit WriteLock(fmhip_model_t m) { if (m) lk = std::unique_lock<std::shared_mutex>(m->mu); }
};
struct ReadLock {
    std::shared_lock<std::shared_mutex> lk;
    explicit ReadLock(fmhip_model_t m) { if (m) lk = std::shared_lock<std::shared_mutex>(m->mu); }
};
// ---- fmhip_dataset.hip
int partition_rows_locked(fmhip_dataset_t d, int64_t cut_feature);      // fmhip_dataset_partition_rows with d->part_mu held by the caller
// ---- fmhip_api.hip: the column walk's epoch in pieces (fmhip_als_epoch; fmhip_mcmc_epoch in fmhip_mcmc.hip).  The caller holds
// the model's lock.  als_check: every refusal of (m, d), the model untouched; als_begin: als_check, the fp64 masters onto the
// device, the walk's arguments (meaningful when d has rows); als_end: the parameters back into the masters and the fp32 copy;
// als_args: the dataset and parameter fields of the walk's arguments (als_begin's, before y, the regularisers, e and q);
// als_plan: the host's view of d's columns
int als_check(fmhip_model_t m, fmhip_dataset_t d);
AlsArgs als_args(fmhip_model_t m, fmhip_dataset_t d);
ColumnPlan als_plan(fmhip_dataset_t d);
int als_begin(fmhip_model_t m, fmhip_dataset_t d, double reg0, double regw, double regv, AlsArgs *out);
int als_end(fmhip_model_t m);
// ---- fmhip_step.hip
int ensure_workspace(fmhip_model_t m, fmhip_dataset_t d);
int ensure_backward_workspace(fmhip_model_t m, fmhip_dataset_t d);     // ... the part a backward over `d` needs (partials, pieces, hot block)
FwdArgs fwd_args(fmhip_model_t m, fmhip_dataset_t d, const BatchMeta &bm);
// ... of a forward that is not the training forward: outputs of the caller's (nullptr: not written), the residual of `loss`
FwdArgs fwd_args_out(fmhip_model_t m, fmhip_dataset_t d, const BatchMeta &bm, float *P, float *e, double *bsum, float *yhat, int loss);
int check_pair(fmhip_model_t m, fmhip_dataset_t d);
int check_train(fmhip_model_t m, fmhip_dataset_t d);      // + the dataset must have its transposes (and, for a paired model, even batches)
int check_even_batches(fmhip_dataset_t d);                // pairs (rows 2j, 2j+1) must not straddle batches
int check_batch(fmhip_dataset_t d, int64_t batch);
// the pieces of one mini-batch step, all asynchronous on m->stream
int step_forward(fmhip_model_t m, fmhip_dataset_t d, int64_t b);
// the pairs' finish over the model's workspace (P, yhat -> P, e, bsum): `rows` rows whose labels start at y and whose weights at c (NULL: none)
PairArgs pair_args(fmhip_model_t m, const float *y, const float *c, int64_t rows);
// the step size and the regularisation of one SGD step (the C entry points take them one by one)
struct Sgd {
    double eta, reg0, regw, regv;
    double dv() const { return 1.0 - eta * regv; }     // the decay of one step (V, w): what lazy decay multiplies the tables' scale by
    double dw() const { return 1.0 - eta * regw; }
};
// a step whose update happens inside the backward (mode 1: every finished gradient row, FMHIP_TUNE_FUSED_UPDATE) or
// inside the fixup launch (mode 2, the merged finish: dense update beside the fixups, FMHIP_TUNE_MERGED_FINISH) — fmhip_api.hip
struct FusedPlan {
    int mode = 0;
    Sgd sgd{};
    double sv_out = 1.0, sw_out = 1.0;    // the tables' scales after the step
    FusedUpd upd{};
};
// the training forward in two passes (pass 0 = A: features below the dataset's split cut; pass 1 = B: the others + the row's finish)
int step_forward_pass(fmhip_model_t m, fmhip_dataset_t d, int64_t b, int pass);
// src (the relational step): the backward reads these P rows / residuals — a block's P_b / e_b — instead of the model's
struct BwdSource { const float *P, *e; };
int step_backward(fmhip_model_t m, fmhip_dataset_t d, int64_t b, int64_t feat_lo, int64_t feat_hi, bool finish, double *acc,
                  const FusedPlan *fused = nullptr, int own = kOwnLower, const BwdSource *src = nullptr);
// forward + backward + fixup of one batch into the packed gradient (fused: straight into the parameters)
int step_compute(fmhip_model_t m, fmhip_dataset_t d, int64_t b, double *acc, const FusedPlan *fused = nullptr);
// can this step's update run inside the fixup launch / the column walk?  (fills *p; false: a launch of its own, step_apply)
bool plan_fused(fmhip_model_t m, fmhip_dataset_t d, int64_t b, const Sgd &s, FusedPlan *p);
int finish_fused(fmhip_model_t m, const FusedPlan &p);      // what step_apply leaves behind, for a step planned fused
// forward begins: the step's target zeroed if it is the packed gradient and holds an old one
int begin_forward(fmhip_model_t m);
// This rank has run out of rows: its contribution to the step's exchange is zeros (row count 0 included).  rows_clean: the
// exchange leaves every gradient ROW of the target zero behind it, so a clean target needs only the statistics head in front of
// them cleared — which keeps the last step's (already exchanged) sums.  A compact view is always such a target
int zero_contribution(fmhip_model_t m, bool rows_clean);
int fold_scales(fmhip_model_t m);                           // lazily decayed tables back to scale 1
int read_acc(fmhip_model_t m, fmhip_stats *st);             // the fp64 epoch accumulators (synchronises)
int step_apply(fmhip_model_t m, const Sgd &s, fmhip_dataset_t d = nullptr, int64_t b = -1);
int step_apply_interval(fmhip_model_t m, const Sgd &s, int64_t lo, int64_t hi, const float *rows, bool last);
// The sharded update of the feature interval [lo, hi) on stream `s` (one launch): V rows [vlo, vhi) (this rank's share) get
// the dense update, every linear weight of the interval is stepped, the G_V rows of [lo, hi_r) outside the share are zeroed
// (hi_r >= hi: the top interval's equal shares reach into the slack rows).  `last`: also steps w0 and closes the step — but for
// the gradient, which stays the step's until the caller's all-gathers have landed (dp_step_sharded).
int step_apply_shard(fmhip_model_t m, const Sgd &s, int64_t lo, int64_t hi, int64_t hi_r, int64_t vlo, int64_t vhi, const float *rows,
                     bool last, hipStream_t stream);
// the rows-only (lazy-decay) update of the feature rows listed on the device (ids < 0 are skipped), |B| from `rows`
// (device float): the touched-rows exchange of the data-parallel step applies the union of all ranks' rows with it
// the step's target a compact view (StepState): the gradient rows are read from (and zeroed in) its arrays, row j belonging to feature feat[j]
// off / last: the rows [off, off + n_feat) of the list (and of a compact view) only — the touched-rows exchange updates a
// feature interval as soon as its slice has arrived; the step's bookkeeping (w0, the tables' scale) moves with the LAST slice
int step_apply_rows(fmhip_model_t m, const Sgd &s, const int32_t *feat, int32_t n_feat, const float *rows, int64_t off = 0, bool last = true);
// can the update of this step leave rows without a gradient alone (weight decay rides in the tables' scale, or there is
// none)?  Under AdaGrad only without decay; under FTRL always (its L2 is no decay: zero gradient, nothing moves) (`r`: the rule to judge by — the model's own, or the one a plan agreed)
bool lazy_decay_ok(fmhip_model_t m, const Sgd &s, const TrainRule &r);
int read_scal(fmhip_model_t m, fmhip_stats *st);
// ---- fmhip_relational.hip
void part_features(fmhip_dataset_t d, std::vector<int32_t> &out);     // a part's features: its transposes' columns and the hot block's ids
int check_rel_model(fmhip_model_t m, fmhip_relational_t R);           // device and dimension; sets the device
// one relational step of batch b, asynchronous on the model's stream; acc (nullable): the epoch's fp64 accumulators.  pairs (the
// BPR trainer): rows 2p / 2p+1 are one example — the finish leaves Q_r and yhat_r, launch_pair_finish forms the residuals
// hinge (pairs only; the WARP step, include/fmhip_warp.h): the pairs' finish takes the weights' slice c + the batch's first row and
// the hinge residual at this margin in place of the model's loss; nullptr: the model's loss, unweighted
// softmax_n > 0 (the sampled softmax's step, include/fmhip_softmax.h) in the hinge's place: between the two finishes the pre-pass
// (fm_softmax.h) writes the probabilities of the batch's pairs into pi's slice — interactions of softmax_n adjacent pairs, the
// log-Q table lq (nullable) read through relation 1's mapping, its partials into sm_bsum — and the pairs' finish takes them as given
struct PairHinge {
    const float *c;      // [2 * n_pairs] over the whole dataset
    float margin;
    int32_t softmax_n = 0;
    float *pi = nullptr;         // [2 * n_pairs] over the whole dataset
    const float *lq = nullptr;
    double *sm_bsum = nullptr;   // [softmax_blocks of the largest batch][4]
};
// queued (the per-batch redraw): rel_block_forwards has been queued for this model state by the caller — the step does not repeat it.
// dev_counts (nullable; one entry per relation, each nullable): the batch's inverse-map counts {n_touched, n_work, n_long, n_part}
// of that relation ON THE DEVICE — its gather reads n_work and n_long there, clamped to the slices' capacity, on worst-case grids,
// and the host's copy of the counts is not read
struct RelStepQueued {
    bool forwards = false;
    const int32_t *const *dev_counts = nullptr;
};
int rel_step(fmhip_model_t m, fmhip_relational_t R, int64_t b, const Sgd &sgd, double *acc, bool pairs = false, const PairHinge *hinge = nullptr,
             const RelStepQueued &queued = RelStepQueued());
// the capacity of the long lists' slices of a batch of `rows` rows (a long list has more than the cut's rows); its partial rows
// number at most twice that
inline int64_t rel_long_cap(int64_t rows) { return rows / FMHIP_RELATIONAL_SUM_CUT + 1; }
// the beginning of a step alone (the BPR trainer's adaptive sampler reads what it leaves): scales folded, workspace sized, every
// block's kFwdQ forward into its relation's Q / yq, asynchronous on the model's stream
int rel_block_forwards(fmhip_model_t m, fmhip_relational_t R);
// Where a relational finish works: per relation the block's q rows and predictions, and the data rows' P / e / yhat / partials — the
// handle's and the model's workspace in a step, buffers of its own in a scoring pass.  yhat holds the plain part's predictions on
// the way in and, where the finish writes them, the rows' on the way out (a row's is read before it is written)
struct RelBufs {
    float *Q[FMHIP_RELATIONS_MAX], *yq[FMHIP_RELATIONS_MAX];
    float *P, *e, *yhat;
    double *bsum;
};
// every block's kFwdQ forward, over the whole block, into w.Q / w.yq on stream s
int rel_q_forwards(fmhip_model_t m, fmhip_relational_t R, const RelBufs &w, hipStream_t s);
// the finish of the data rows B over w, in its scoring form's layout: the predictions written, no q_only
RelFinishArgs rel_finish_args(fmhip_model_t m, fmhip_relational_t R, const RelBufs &w, const fmhip_relational::Batch &B, int loss);
// ---- fmhip_score.hip: fmhip_pair_logloss over the rows of a relational dataset without a plain part (the caller holds the model's lock shared)
int rel_pair_score(fmhip_model_t m, fmhip_relational_t R, double *logloss, double *concordance, fmhip_stats *stats);
// ... and fmhip_softmax_loss: the rows as interactions of n adjacent pairs (every batch whole ones), lq (nullable) the log-Q table
// read through relation 1's mapping -> sums[0] = the interactions whose positive is on top, sums[1] = the sum of their losses
int rel_softmax_score(fmhip_model_t m, fmhip_relational_t R, int32_t n, const float *lq, double *sums, fmhip_stats *stats);
// the four leading numbers of a statistics block {sum e, sum e^2, rows, rows with a non-finite prediction} (the packed gradient's
// fp32 head, an fp64 accumulator) into *st; nnz, steps and what a fifth slot means are the caller's
template <typename T>
inline void fill_stats(fmhip_stats *st, const T *h) {
    auto count = [](double x) { return (int64_t)llround(x); };
    st->sum_e = h[0];
    st->sse = h[1];
    st->rows = count(h[2]);
    st->nonfinite = count(h[3]);
}

}  // namespace host
}  // namespace fmhip
