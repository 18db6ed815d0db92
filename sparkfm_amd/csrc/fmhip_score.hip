// fmhip_score.hip — the C ABI's scoring calls: predictions, residuals, q, RMSE / log-loss / pairwise log-loss (include/fmhip.h,
// fmhip_pairing.h), ROC AUC (fmhip_metrics.h), top-K and pair scores (fmhip_topk.h), ranks of given rows (fmhip_ranking.h).  They hold the model's lock SHARED and touch
// nothing of it but its parameters: every call works on a stream and in a workspace of its own (ScoreCtx), so any number of host
// threads score through one model at once.  ScorePass is what they all share; the kernels are fm_forward / fm_pairing / fm_auc /
// fm_topk / fm_rank .hip.
#include "fmhip_internal.h"
#include "../../include/fmhip_topk.h"
#include "../../include/fmhip_metrics.h"
#include "../../include/fmhip_ranking.h"
#include "fm_topk.h"
#include "fm_rank.h"
#include "fm_pairing.h"
#include "fm_auc.h"
#include "fm_weights.h"
#include "fm_relational.h"
#include "../../include/fmhip_weights.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <memory>
#include <new>
#include <vector>

using namespace fmhip;
using namespace fmhip::host;

namespace {

// What a call's forwards write into the workspace: per array the most rows one forward covers (-1: the call never asks for it),
// and whether the call sums statistics (the accumulator: five fp64 slots).
struct ScoreNeeds {
    int64_t e, yhat, P;
    bool stats;
};

// where one forward puts the q rows [rows][Kp], the residuals and the predictions (nullptr: not written)
struct ScoreOut {
    float *P, *e, *yhat;
};

// for a forward that writes no statistic partials itself: the launch behind it that does (into bsum, *parts of them)
using PartialsBy = std::function<hipError_t(double *bsum, int *parts)>;

// One scoring call's pass over the batches of its dataset(s): begin() once, forward() per batch, read() for the sums.  It works
// in a ScoreCtx taken from the model's pool (or made), given back when the call returns.
// DESTRUCTOR ORDER: a call declares the device buffers of its own BEFORE its ScorePass (in a struct: as earlier members) — locals
// die in reverse, so ~ScorePass has drained the stream by the time those buffers are freed, on every return path.
struct ScorePass {
    fmhip_model_t m;
    ScoreCtx *ctx = nullptr;
    bool stats = false;
    explicit ScorePass(fmhip_model_t m_) : m(m_) {}
    ScoreCtx &cx() const { return *ctx; }
    ~ScorePass() {
        if (!ctx) return;
        (void)hipStreamSynchronize(ctx->s);       // an early error return must not hand a busy workspace to the next call
        std::lock_guard<std::mutex> g(m->pool_mu);
        m->ctx_free.push_back(ctx);
    }
    int lease() {
        {
            std::lock_guard<std::mutex> g(m->pool_mu);
            if (!m->ctx_free.empty()) {
                ctx = m->ctx_free.back();
                m->ctx_free.pop_back();
                return FMHIP_OK;
            }
        }
        std::unique_ptr<ScoreCtx> fresh(new (std::nothrow) ScoreCtx());
        if (!fresh) return fail(FMHIP_ERR_NOMEM, "out of host memory");
        HIP_TRY(hipStreamCreateWithFlags(&fresh->s, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&fresh->ev, hipEventDisableTiming));
        std::lock_guard<std::mutex> g(m->pool_mu);
        ctx = fresh.get();
        m->ctx_all.push_back(std::move(fresh));
        return FMHIP_OK;
    }

    // the lease; the workspace at the sizes asked for; the stream behind the model's own; the accumulator at zero
    int begin(const ScoreNeeds &n) {
        TRY(lease());
        ScoreCtx &c = cx();
        auto rows = [](int64_t r) { return (size_t)std::max<int64_t>(r, 1); };
        if (n.e >= 0) TRY(c.e.ensure(rows(n.e)));
        if (n.yhat >= 0) TRY(c.yhat.ensure(rows(n.yhat)));
        if (n.P >= 0) TRY(c.P.ensure(rows(n.P) * m->Kp));
        TRY(c.bsum.ensure((size_t)kMaxFwdBlocks * 4));
        stats = n.stats;
        if (stats) TRY(c.acc.ensure(5));
        // behind whatever the model's own stream still has queued (a training step returns before it has run)
        HIP_TRY(hipEventRecord(c.ev, m->stream));
        HIP_TRY(hipStreamWaitEvent(c.s, c.ev, 0));
        if (stats) HIP_TRY(hipMemsetAsync(c.acc.p, 0, 5 * sizeof(double), c.s));
        return FMHIP_OK;
    }

    // The forward of batch `bm` of `d` in `mode` under `loss` into `o` and, when the call sums statistics, the block reduction of
    // its partials into the accumulator (`fifth`: also slot 4, the sum of the rows' log-losses).  With `partials_by` the forward
    // writes no partials: that launch runs between the two and supplies them.
    int forward(fmhip_dataset_t d, const BatchMeta &bm, FwdMode mode, const ScoreOut &o, int loss, bool fifth = false,
                const PartialsBy &partials_by = nullptr) {
        ScoreCtx &c = cx();
        const FwdArgs a = fwd_args_out(m, d, bm, o.P, o.e, partials_by ? nullptr : c.bsum.p, o.yhat, loss);
        int parts = 0;
        HIP_TRY(launch_forward(m->Kp, mode, a, c.s, stats && !partials_by ? &parts : nullptr));
        if (partials_by) HIP_TRY(partials_by(c.bsum.p, &parts));
        if (stats) HIP_TRY(launch_reduce_blocks(c.bsum.p, parts, (int32_t)bm.rows, nullptr, c.acc.p, c.s, fifth));
        return FMHIP_OK;
    }

    // the accumulator's five sums (synchronises); st given: its four leading fields from slots 0..3, everything else zero
    int read(fmhip_stats *st, double h[5]) {
        HIP_TRY(hipMemcpyAsync(h, cx().acc.p, 5 * sizeof(double), hipMemcpyDeviceToHost, cx().s));
        HIP_TRY(hipStreamSynchronize(cx().s));
        if (st) {
            memset(st, 0, sizeof *st);
            fill_stats(st, h);
        }
        return FMHIP_OK;
    }

    // [rows][ld] floats on the device -> the leading `cols` of every row, widened, to out[rows][cols]: one copy on the pass's
    // stream through the reusable host buffer `h`, one synchronisation
    int copy_back(const float *dev, int64_t rows, int ld, int cols, std::vector<float> &h, double *out) {
        h.resize((size_t)rows * ld);
        HIP_TRY(hipMemcpyAsync(h.data(), dev, h.size() * sizeof(float), hipMemcpyDeviceToHost, cx().s));
        HIP_TRY(hipStreamSynchronize(cx().s));
        for (int64_t r = 0; r < rows; ++r)
            for (int f = 0; f < cols; ++f) out[r * cols + f] = (double)h[(size_t)r * ld + f];
        return FMHIP_OK;
    }
};

// One pass of FMModel.predict over a dataset's rows.  The scoring calls are the reference's formulas whatever the model's
// training loss; logloss (fmhip_logloss) scores under the logistic loss instead: st's sums are over e = sigma(yhat) - t and
// *logloss = the sum of the rows' log-losses.
int score_pass(fmhip_model_t m, fmhip_dataset_t d, double *yhat, double *e_out, double *q_out, fmhip_stats *st,
               double *logloss = nullptr) {
    TRY(check_pair(m, d));
    ScorePass pass(m);
    TRY(pass.begin({d->max_rows, yhat ? d->max_rows : -1, q_out ? d->max_rows : -1, true}));     // (P: only to hand q back)
    ScoreCtx &cx = pass.cx();
    const ScoreOut out{q_out ? cx.P.p : nullptr, cx.e.p, yhat ? cx.yhat.p : nullptr};
    std::vector<float> hbuf;
    for (const BatchMeta &bm : d->batches) {
        TRY(pass.forward(d, bm, q_out ? kFwdQ : kFwdResidual, out, logloss ? kLossLogistic : kLossSquared, logloss != nullptr));
        if (yhat) TRY(pass.copy_back(cx.yhat.p, bm.rows, 1, 1, hbuf, yhat + bm.row0));
        if (e_out) TRY(pass.copy_back(cx.e.p, bm.rows, 1, 1, hbuf, e_out + bm.row0));
        if (q_out) TRY(pass.copy_back(cx.P.p, bm.rows, m->Kp, m->k, hbuf, q_out + bm.row0 * m->k));
    }
    if (st) {
        double h[5];
        TRY(pass.read(st, h));
        st->nnz = d->nnz;
        if (logloss) *logloss = h[4];
    }
    return FMHIP_OK;
}

}  // namespace

extern "C" {

int fmhip_predict(fmhip_model_t m, fmhip_dataset_t d, double *yhat) {
    ReadLock lock(m);
    if (!yhat) return fail(FMHIP_ERR_INVALID, "yhat is NULL");
    return score_pass(m, d, yhat, nullptr, nullptr, nullptr);
}

int fmhip_predict_rows(fmhip_model_t m, int64_t n_rows, const int64_t *row_ptr, const int32_t *col, const double *val,
                       double *yhat) {
    ReadLock lock(m);
    if (!m) return fail(FMHIP_ERR_INVALID, "model is NULL");
    if (n_rows > 0 && !yhat) return fail(FMHIP_ERR_INVALID, "yhat is NULL");
    fmhip_dataset_t d = nullptr;
    TRY(fmhip_rows_create(m->device, n_rows, row_ptr, col, val, nullptr, &d));      // scoring-only upload (fmhip_dataset.hip)
    const int rc = n_rows > 0 ? score_pass(m, d, yhat, nullptr, nullptr, nullptr) : FMHIP_OK;
    fmhip_dataset_destroy(d);
    return rc;
}

int fmhip_residual(fmhip_model_t m, fmhip_dataset_t d, double *e) {
    ReadLock lock(m);
    if (!e) return fail(FMHIP_ERR_INVALID, "e is NULL");
    return score_pass(m, d, nullptr, e, nullptr, nullptr);
}

int fmhip_term_q(fmhip_model_t m, fmhip_dataset_t d, double *q) {
    ReadLock lock(m);
    if (!q) return fail(FMHIP_ERR_INVALID, "q is NULL");
    return score_pass(m, d, nullptr, nullptr, q, nullptr);
}

int fmhip_rmse(fmhip_model_t m, fmhip_dataset_t d, double *rmse, fmhip_stats *stats) {
    ReadLock lock(m);
    if (!rmse) return fail(FMHIP_ERR_INVALID, "rmse is NULL");
    fmhip_stats st;
    TRY(score_pass(m, d, nullptr, nullptr, nullptr, &st));
    // S/Model.scala:13-19: sqrt(sum (y - yhat)^2 / size); (y - yhat)^2 == e^2
    *rmse = st.rows > 0 ? std::sqrt(st.sse / (double)st.rows) : 0.0;
    if (stats) *stats = st;
    return FMHIP_OK;
}

int fmhip_logloss(fmhip_model_t m, fmhip_dataset_t d, double *logloss, fmhip_stats *stats) {
    ReadLock lock(m);
    if (!m) return fail(FMHIP_ERR_INVALID, "model is NULL");
    if (!logloss) return fail(FMHIP_ERR_INVALID, "logloss is NULL");
    fmhip_stats st;
    double sum_l = 0.0;
    TRY(score_pass(m, d, nullptr, nullptr, nullptr, &st, &sum_l));
    *logloss = st.rows > 0 ? sum_l / (double)st.rows : 0.0;
    if (stats) *stats = st;
    return FMHIP_OK;
}

// Pairwise ranking score of the pairs (2j, 2j+1) of `d`, whatever the model's loss or pairing: per batch one residual-mode forward
// for the predictions only, then k_pair_score's per-block partials and the block reduction of fmhip_logloss (fp64 sums).
int fmhip_pair_logloss(fmhip_model_t m, fmhip_dataset_t d, double *logloss, double *concordance, fmhip_stats *stats) {
    ReadLock lock(m);
    if (!m) return fail(FMHIP_ERR_INVALID, "model is NULL");
    if (!logloss) return fail(FMHIP_ERR_INVALID, "logloss is NULL");
    TRY(check_pair(m, d));
    TRY(check_even_batches(d));
    ScorePass pass(m);
    TRY(pass.begin({-1, std::max<int64_t>(d->max_rows, 2), -1, true}));
    ScoreCtx &cx = pass.cx();
    for (const BatchMeta &bm : d->batches)
        TRY(pass.forward(d, bm, kFwdResidual, ScoreOut{nullptr, nullptr, cx.yhat.p}, kLossSquared, true, [&](double *bsum, int *parts) {
            return launch_pair_score(cx.yhat.p, d->y.p + bm.row0, (int32_t)(bm.rows / 2), bsum, cx.s, parts);
        }));
    double h[5];       // {concordant pairs, sum e^2, rows, rows with a non-finite prediction, sum of the pairs' log-losses}
    TRY(pass.read(stats, h));
    const double pairs = (double)(d->n_rows / 2);
    *logloss = pairs > 0 ? h[4] / pairs : 0.0;
    if (concordance) *concordance = pairs > 0 ? h[0] / pairs : 0.0;
    if (stats) {
        stats->sum_e = 0.0;        // e_2j = -e_2j+1
        stats->nnz = d->nnz;
    }
    return FMHIP_OK;
}

// Weighted scores over a weighted dataset (include/fmhip_weights.h): per batch the residual-mode forward of fmhip_rmse — its own
// partials give the row count and the rows with a non-finite prediction — then k_weighted_score's partials over the predictions it
// left, summed by the block reduction of fmhip_logloss into an accumulator of the call's own.
int fmhip_weighted_scores(fmhip_model_t m, fmhip_dataset_t d, fmhip_weighted_result *out) {
    if (!out) return fail(FMHIP_ERR_INVALID, "out is NULL");
    if (out->struct_size != (int32_t)sizeof(fmhip_weighted_result))
        return fail(FMHIP_ERR_INVALID, "out->struct_size is %d, not sizeof(fmhip_weighted_result) = %d", (int)out->struct_size,
                    (int)sizeof(fmhip_weighted_result));
    ReadLock lock(m);
    TRY(check_pair(m, d));
    if (!d->weighted)
        return fail(FMHIP_ERR_INVALID, "the dataset carries no example weights (fmhip_dataset_create_weighted / fmhip_rows_create_weighted): "
                                       "its unweighted scores are fmhip_rmse and fmhip_logloss");
    DevBuf<double> wsum, wacc;       // (before the pass: freed after it has drained its stream)
    ScorePass pass(m);
    TRY(wsum.alloc((size_t)weighted_score_blocks(d->max_rows) * 4));
    TRY(wacc.alloc(5));
    TRY(pass.begin({d->max_rows, d->max_rows, -1, true}));
    ScoreCtx &cx = pass.cx();
    HIP_TRY(hipMemsetAsync(wacc.p, 0, 5 * sizeof(double), cx.s));
    for (const BatchMeta &bm : d->batches) {
        TRY(pass.forward(d, bm, kFwdResidual, ScoreOut{nullptr, cx.e.p, cx.yhat.p}, kLossSquared));
        int parts = 0;
        HIP_TRY(launch_weighted_score(cx.yhat.p, d->y.p + bm.row0, d->c.p + bm.row0, (int32_t)bm.rows, wsum.p, cx.s, &parts));
        HIP_TRY(launch_reduce_blocks(wsum.p, parts, (int32_t)bm.rows, nullptr, wacc.p, cx.s, true));
    }
    double h[5], hw[5];       // hw: {sum c, sum c e^2, rows, sum c |e|, sum c l}
    HIP_TRY(hipMemcpyAsync(hw, wacc.p, sizeof hw, hipMemcpyDeviceToHost, cx.s));
    fmhip_stats st;
    TRY(pass.read(&st, h));    // (synchronises the stream)
    const double nan = std::nan("");
    out->reserved = 0;
    out->sum_w = hw[0];
    out->rmse = hw[0] > 0.0 ? std::sqrt(hw[1] / hw[0]) : nan;
    out->mae = hw[0] > 0.0 ? hw[3] / hw[0] : nan;
    out->logloss = hw[0] > 0.0 ? hw[4] / hw[0] : nan;
    out->rows = st.rows;
    out->nonfinite = st.nonfinite;
    return FMHIP_OK;
}

// ---- ROC AUC and per-group AUC (include/fmhip_metrics.h) ---------------------------------------------------------------------
// One 64-bit word per row (group, key of the prediction, label), sorted; the counts are read off the sorted words (fm_auc.hip).
// fmhip_auc forms the words batch by batch behind the residual-mode forward, fmhip_auc_scores from the caller's arrays: the two
// share every line after that.
namespace {

// the refusals that touch neither a handle nor a device
int auc_check_out(fmhip_auc_result *out) {
    if (!out) return fail(FMHIP_ERR_INVALID, "out is NULL");
    if (out->struct_size != (int32_t)sizeof(fmhip_auc_result))
        return fail(FMHIP_ERR_INVALID, "out->struct_size is %d, not sizeof(fmhip_auc_result) = %d", (int)out->struct_size,
                    (int)sizeof(fmhip_auc_result));
    return FMHIP_OK;
}
int auc_check_rows(int64_t n) {
    if (n < 0) return fail(FMHIP_ERR_INVALID, "n = %lld is negative", (long long)n);
    if (n > 0x7fffffffll) return fail(FMHIP_ERR_UNSUPPORTED, "%lld rows: the AUC calls take fewer than 2^31", (long long)n);
    return FMHIP_OK;
}
// the ids must be >= 0; *end_bit: the bits of a word the sort has to look at (33 + what the largest id needs)
int auc_check_groups(const int32_t *group, int64_t n, int *end_bit) {
    int32_t top = 0;
    if (group)
        for (int64_t r = 0; r < n; ++r) {
            if (group[r] < 0) return fail(FMHIP_ERR_INVALID, "group id %d of row %lld is negative", (int)group[r], (long long)r);
            top = group[r] > top ? group[r] : top;
        }
    int bits = 0;
    while (bits < 31 && ((int64_t)top >> bits) != 0) ++bits;
    *end_bit = kAucGroupShift + bits;
    return FMHIP_OK;
}
void auc_fill(fmhip_auc_result *out, const AucSums &a, int64_t n) {
    const double nan = std::nan("");
    out->reserved = 0;
    out->u2 = a.u2;
    out->pairs = (int64_t)a.pairs;
    out->negatives = (int64_t)a.negatives;
    out->positives = n - (int64_t)a.negatives;
    out->groups = (int64_t)a.groups;
    out->groups_scored = (int64_t)a.groups_scored;
    out->auc = a.pairs ? (double)a.u2 / (2.0 * (double)a.pairs) : nan;
    // one scored group: its AUC itself (the weighted mean of one number), so that gauc == auc bit for bit without groups
    out->gauc = a.groups_scored == 0 ? nan : (a.groups_scored == 1 ? out->auc : a.gauc_num / (double)a.rows_scored);
}
struct OwnStream {
    hipStream_t s = nullptr;
    ~OwnStream() {
        if (s) (void)hipStreamDestroy(s);
    }
};

}  // namespace

int fmhip_auc_scores(int device, int64_t n, const float *score, const float *y, const int32_t *group, fmhip_auc_result *out) {
    TRY(auc_check_out(out));
    TRY(auc_check_rows(n));
    if (n > 0 && (!score || !y)) return fail(FMHIP_ERR_INVALID, "score or y is NULL");
    int end_bit = 0;
    TRY(auc_check_groups(group, n, &end_bit));
    AucSums sums{};
    if (n == 0) {
        auc_fill(out, sums, 0);
        return FMHIP_OK;
    }
    TRY(set_device(device));
    DevBuf<float> ds, dy;
    DevBuf<int32_t> dg;
    DevBuf<unsigned long long> words;
    OwnStream st;            // (declared after the buffers: destroyed, and so drained, before they are freed)
    TRY(ds.alloc((size_t)n));
    TRY(dy.alloc((size_t)n));
    if (group) TRY(dg.alloc((size_t)n));
    TRY(words.alloc((size_t)n));
    HIP_TRY(hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking));
    HIP_TRY(hipMemcpyAsync(ds.p, score, (size_t)n * sizeof(float), hipMemcpyHostToDevice, st.s));
    HIP_TRY(hipMemcpyAsync(dy.p, y, (size_t)n * sizeof(float), hipMemcpyHostToDevice, st.s));
    if (group) HIP_TRY(hipMemcpyAsync(dg.p, group, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st.s));
    HIP_TRY(launch_auc_keys(ds.p, dy.p, dg.p, n, words.p, st.s));
    HIP_TRY(auc_from_words(words.p, n, end_bit, st.s, &sums));
    auc_fill(out, sums, n);
    return FMHIP_OK;
}

int fmhip_auc(fmhip_model_t m, fmhip_dataset_t d, const int32_t *group, fmhip_auc_result *out, fmhip_stats *stats) {
    TRY(auc_check_out(out));
    ReadLock lock(m);
    if (!m || !d) return fail(FMHIP_ERR_INVALID, "model or dataset is NULL");
    const int64_t n = d->n_rows;
    TRY(auc_check_rows(n));
    TRY(check_pair(m, d));
    int end_bit = 0;
    TRY(auc_check_groups(group, n, &end_bit));
    AucSums sums{};
    if (stats) {
        memset(stats, 0, sizeof *stats);
        stats->nnz = d->nnz;
    }
    if (n == 0) {
        auc_fill(out, sums, 0);
        return FMHIP_OK;
    }
    DevBuf<int32_t> dg;
    DevBuf<unsigned long long> words;
    ScorePass pass(m);
    TRY(words.alloc((size_t)n));
    if (group) TRY(dg.alloc((size_t)n));
    TRY(pass.begin({d->max_rows, d->max_rows, -1, true}));
    ScoreCtx &cx = pass.cx();
    if (group) HIP_TRY(hipMemcpyAsync(dg.p, group, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, cx.s));
    for (const BatchMeta &bm : d->batches) {
        // the forward of fmhip_rmse / fmhip_predict: the same predictions, the same statistics; then the rows' words
        TRY(pass.forward(d, bm, kFwdResidual, ScoreOut{nullptr, cx.e.p, cx.yhat.p}, kLossSquared));
        HIP_TRY(launch_auc_keys(cx.yhat.p, d->y.p + bm.row0, group ? dg.p + bm.row0 : nullptr, bm.rows, words.p + bm.row0, cx.s));
    }
    HIP_TRY(auc_from_words(words.p, n, end_bit, cx.s, &sums));
    if (stats) {
        double h[5];
        TRY(pass.read(stats, h));
        stats->nnz = d->nnz;
    }
    auc_fill(out, sums, n);
    return FMHIP_OK;
}

// ---- top-K recommendation (include/fmhip_topk.h) ----------------------------------------------------------------------------
// score(c, d) = (yhat(c) + (yhat(d) - w0)) + sum_f q_f(c) q_f(d): one kFwdQ forward per row set — it writes q into a [rows][Kp]
// table and yhat beside it in one launch — then the product and the selection of fm_topk.hip.  The tables live for the length of
// the call only.
namespace {

// ptr [n + 1], the offsets of n contexts' lists in a flat array: non-negative and non-decreasing
int check_offsets(const char *name, const int64_t *ptr, int64_t n) {
    if (ptr[0] < 0) return fail(FMHIP_ERR_INVALID, "%s[0] < 0", name);
    for (int64_t c = 0; c < n; ++c)
        if (ptr[c + 1] < ptr[c]) return fail(FMHIP_ERR_INVALID, "%s decreases at context %lld", name, (long long)c);
    return FMHIP_OK;
}

// what the three calls share: the checks, the pass, the candidates' table Qd [M][Kp] and predictions yd [M], the tables every
// pair kernel reads, the exclusion lists on the device, the way results travel back
struct PairJob {
    fmhip_model_t m;
    fmhip_dataset_t ctx, cand;
    DevBuf<float> Qd, yd;
    DevBuf<int64_t> d_eptr;
    DevBuf<int32_t> d_excl;
    ScorePass pass;
    int64_t B = 0, M = 0;
    PairTables t{};             // the context batch held in cx.P / cx.yhat, the candidates, w0
    std::vector<float> h_score;
    PairJob(fmhip_model_t m_, fmhip_dataset_t c_, fmhip_dataset_t d_) : m(m_), ctx(c_), cand(d_), pass(m_) {}
    // the kFwdQ forward of one batch of `d`: q rows to Q[rows][Kp], predictions to yhat[rows]
    int forward_q(fmhip_dataset_t d, const BatchMeta &bm, float *Q, float *yhat) {
        return pass.forward(d, bm, kFwdQ, ScoreOut{Q, pass.cx().e.p, yhat}, kLossSquared);
    }
    int forward_ctx(const BatchMeta &bm) { return forward_q(ctx, bm, pass.cx().P.p, pass.cx().yhat.p); }
    int begin() {
        if (!m || !ctx || !cand) return fail(FMHIP_ERR_INVALID, "model, contexts or candidates is NULL");
        TRY(check_pair(m, ctx));
        TRY(check_pair(m, cand));
        B = ctx->n_rows;
        M = cand->n_rows;
        if (M > 0x7fffffff) return fail(FMHIP_ERR_INVALID, "%lld candidates: the count must fit an int32", (long long)M);
        TRY(pass.begin({std::max(ctx->max_rows, cand->max_rows), ctx->max_rows, ctx->max_rows, false}));
        if (B == 0 || M == 0) return FMHIP_OK;
        TRY(Qd.alloc((size_t)M * m->Kp));
        TRY(yd.alloc((size_t)M));
        for (const BatchMeta &bm : cand->batches) TRY(forward_q(cand, bm, Qd.p + (size_t)bm.row0 * m->Kp, yd.p + bm.row0));
        t = PairTables{pass.cx().P.p, pass.cx().yhat.p, Qd.p, yd.p, m->w0.p};
        return FMHIP_OK;
    }
    TopkArgs args(int64_t first, int64_t rows) const {      // for rows [first, first + rows) of the context batch
        TopkArgs a{};
        a.t = t;
        a.t.Qc += (size_t)first * m->Kp;
        a.t.yc += first;
        a.B = (int32_t)rows;
        a.M = (int32_t)M;
        return a;
    }
    // The exclusion lists (checked: check_exclusions) to the device, as the caller holds them: d_eptr = excl_ptr [B + 1] and
    // d_excl = excl [excl_ptr[B]], so an offset means on the device what it means to the caller — context c's rows are
    // d_excl[d_eptr[c] .. d_eptr[c + 1]), whatever excl_ptr[0] is, for the kernels and for the host's pointer arithmetic alike.
    int upload_exclusions(const int64_t *excl_ptr, const int32_t *excl) {
        TRY(d_eptr.alloc((size_t)B + 1));
        TRY(d_excl.alloc((size_t)std::max<int64_t>(excl_ptr[B], 1)));
        HIP_TRY(hipMemcpyAsync(d_eptr.p, excl_ptr, ((size_t)B + 1) * sizeof(int64_t), hipMemcpyHostToDevice, pass.cx().s));
        if (excl_ptr[B] > 0) HIP_TRY(hipMemcpyAsync(d_excl.p, excl, (size_t)excl_ptr[B] * sizeof(int32_t), hipMemcpyHostToDevice, pass.cx().s));
        return FMHIP_OK;
    }
    // the end of a chunk: n integers back and, if asked for, n scores beside them, widened — one synchronisation for both copies
    int results_back(const int32_t *d_ints, int32_t *ints, const float *d_score, double *score, int64_t n) {
        HIP_TRY(hipMemcpyAsync(ints, d_ints, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, pass.cx().s));
        if (score) return pass.copy_back(d_score, n, 1, 1, h_score, score);
        HIP_TRY(hipStreamSynchronize(pass.cx().s));
        return FMHIP_OK;
    }
};

// the exclusion lists of fmhip_topk / fmhip_rank: both arrays or neither; offsets non-negative and non-decreasing; per context
// the rows inside [0, M), ascending and distinct
int check_exclusions(const int64_t *excl_ptr, const int32_t *excl, int64_t B, int64_t M) {
    if ((excl_ptr == nullptr) != (excl == nullptr))
        return fail(FMHIP_ERR_INVALID, "excl_ptr and excl must both be given or both be NULL");
    if (!excl_ptr) return FMHIP_OK;
    TRY(check_offsets("excl_ptr", excl_ptr, B));      // (the offsets first: nothing of excl is read through a bad one)
    for (int64_t c = 0; c < B; ++c) {
        for (int64_t p = excl_ptr[c]; p < excl_ptr[c + 1]; ++p) {
            if (excl[p] < 0 || excl[p] >= M)
                return fail(FMHIP_ERR_INVALID, "context %lld excludes candidate %d outside [0, %lld)", (long long)c, (int)excl[p], (long long)M);
            if (p > excl_ptr[c] && excl[p] <= excl[p - 1])
                return fail(FMHIP_ERR_INVALID, "the exclusions of context %lld are not ascending and distinct", (long long)c);
        }
    }
    return FMHIP_OK;
}

}  // namespace

int fmhip_topk(fmhip_model_t m, fmhip_dataset_t contexts, fmhip_dataset_t candidates, int32_t k, const int64_t *excl_ptr,
               const int32_t *excl, int32_t *idx, double *score) {
    ReadLock lock(m);
    if (!m || !contexts || !candidates) return fail(FMHIP_ERR_INVALID, "model, contexts or candidates is NULL");
    if (!idx) return fail(FMHIP_ERR_INVALID, "idx is NULL");
    if (k < 1 || k > FMHIP_TOPK_MAX) return fail(FMHIP_ERR_INVALID, "k = %d outside [1, %d]", (int)k, FMHIP_TOPK_MAX);
    const int64_t B = contexts->n_rows, M = candidates->n_rows;
    TRY(check_exclusions(excl_ptr, excl, B, M));
    DevBuf<int32_t> d_idx;
    DevBuf<float> d_score;
    DevBuf<unsigned long long> part;
    PairJob job(m, contexts, candidates);
    TRY(job.begin());
    if (B == 0) return FMHIP_OK;
    if (M == 0) {
        for (int64_t i = 0; i < B * k; ++i) idx[i] = -1;
        if (score) for (int64_t i = 0; i < B * k; ++i) score[i] = -HUGE_VAL;
        return FMHIP_OK;
    }
    ScoreCtx &cx = job.pass.cx();
    if (excl_ptr) TRY(job.upload_exclusions(excl_ptr, excl));
    const size_t rows_max = (size_t)contexts->max_rows;
    TRY(d_idx.alloc(rows_max * k));
    TRY(d_score.alloc(rows_max * k));
    for (const BatchMeta &bm : contexts->batches) {       // a chunk of contexts = a batch of their dataset
        TRY(job.forward_ctx(bm));
        TopkArgs a = job.args(0, bm.rows);
        a.K = k;
        const int splits = topk_splits(bm.rows, M, &a.split_len);
        TRY(part.ensure((size_t)bm.rows * splits * k));
        a.part = part.p;
        a.excl_ptr = excl_ptr ? job.d_eptr.p + bm.row0 : nullptr;
        a.excl = job.d_excl.p;
        HIP_TRY(launch_pair_topk(m->Kp, a, cx.s));
        HIP_TRY(launch_topk_merge(part.p, (int32_t)bm.rows, splits, k, d_idx.p, d_score.p, cx.s));
        TRY(job.results_back(d_idx.p, idx + bm.row0 * k, d_score.p, score ? score + (size_t)bm.row0 * k : nullptr, bm.rows * k));
    }
    return FMHIP_OK;
}

int fmhip_pair_scores(fmhip_model_t m, fmhip_dataset_t contexts, fmhip_dataset_t candidates, int64_t c0, int64_t c1, double *out) {
    ReadLock lock(m);
    if (!m || !contexts || !candidates) return fail(FMHIP_ERR_INVALID, "model, contexts or candidates is NULL");
    if (c0 < 0 || c1 < c0 || c1 > contexts->n_rows)
        return fail(FMHIP_ERR_INVALID, "contexts [%lld, %lld) outside [0, %lld]", (long long)c0, (long long)c1, (long long)contexts->n_rows);
    const int64_t M = candidates->n_rows;
    if (c1 > c0 && M > 0 && !out) return fail(FMHIP_ERR_INVALID, "out is NULL");
    DevBuf<float> d_out;
    PairJob job(m, contexts, candidates);
    TRY(job.begin());
    if (c1 == c0 || M == 0) return FMHIP_OK;
    ScoreCtx &cx = job.pass.cx();
    // the scores travel in pieces of at most 2^25 floats (whole context rows)
    const int64_t piece_rows = std::max<int64_t>(1, ((int64_t)1 << 25) / std::max<int64_t>(M, 1));
    TRY(d_out.alloc((size_t)std::min(piece_rows, c1 - c0) * M));
    std::vector<float> h_out;
    for (const BatchMeta &bm : contexts->batches) {
        const int64_t lo = std::max(c0, bm.row0), hi = std::min(c1, bm.row0 + bm.rows);
        if (lo >= hi) continue;
        TRY(job.forward_ctx(bm));
        for (int64_t r0 = lo; r0 < hi; r0 += piece_rows) {
            const int64_t rows = std::min(piece_rows, hi - r0);
            TopkArgs a = job.args(r0 - bm.row0, rows);
            (void)topk_splits(rows, M, &a.split_len);
            a.out = d_out.p;
            HIP_TRY(launch_pair_scores(m->Kp, a, cx.s));
            TRY(job.pass.copy_back(d_out.p, rows * M, 1, 1, h_out, out + (size_t)(r0 - c0) * M));
        }
    }
    return FMHIP_OK;
}

// ---- ranking evaluation (include/fmhip_ranking.h) ----------------------------------------------------------------------------
// Per chunk of contexts (a batch of their dataset) the chunk's (context, relevant row) pairs are its QUERIES: their targets'
// order words from k_pair_list, the order words of the chunk's (context, excluded row) pairs from the same kernel, the counting
// sweep k_pair_rank over pieces of at most kRankPiece queries, k_rank_finish (fm_rank.hip).  Integers come back, and one score
// per query if asked for.
namespace {

constexpr int64_t kRankPiece = (int64_t)1 << 20;      // queries per sweep: bounds part[nq][splits] at 2 GB

int check_relevant(int64_t B, int64_t M, const int64_t *rel_ptr, const int32_t *rel, const int64_t *excl_ptr, const int32_t *excl,
                   const int32_t *rank) {
    if (B == 0) return FMHIP_OK;
    if (!rel_ptr) return fail(FMHIP_ERR_INVALID, "rel_ptr is NULL");
    TRY(check_offsets("rel_ptr", rel_ptr, B));
    if (rel_ptr[B] == 0) return FMHIP_OK;
    if (!rel || !rank) return fail(FMHIP_ERR_INVALID, "rel or rank is NULL");
    for (int64_t c = 0; c < B; ++c) {
        int64_t e = excl_ptr ? excl_ptr[c] : 0;
        const int64_t e_end = excl_ptr ? excl_ptr[c + 1] : 0;
        for (int64_t p = rel_ptr[c]; p < rel_ptr[c + 1]; ++p) {
            if (rel[p] < 0 || rel[p] >= M)
                return fail(FMHIP_ERR_INVALID, "relevant row %d of context %lld outside [0, %lld)", (int)rel[p], (long long)c, (long long)M);
            if (p > rel_ptr[c] && rel[p] <= rel[p - 1])
                return fail(FMHIP_ERR_INVALID, "the relevant rows of context %lld are not ascending and distinct", (long long)c);
            while (e < e_end && excl[e] < rel[p]) ++e;       // (both lists ascend: one merge pass)
            if (e < e_end && excl[e] == rel[p])
                return fail(FMHIP_ERR_INVALID, "candidate %d is both relevant and excluded for context %lld", (int)rel[p], (long long)c);
        }
    }
    return FMHIP_OK;
}

}  // namespace

int fmhip_rank(fmhip_model_t m, fmhip_dataset_t contexts, fmhip_dataset_t candidates, const int64_t *rel_ptr, const int32_t *rel,
               const int64_t *excl_ptr, const int32_t *excl, int32_t *rank, double *score) {
    ReadLock lock(m);
    if (!m || !contexts || !candidates) return fail(FMHIP_ERR_INVALID, "model, contexts or candidates is NULL");
    const int64_t B = contexts->n_rows, M = candidates->n_rows;
    TRY(check_exclusions(excl_ptr, excl, B, M));
    TRY(check_relevant(B, M, rel_ptr, rel, excl_ptr, excl, rank));
    DevBuf<int32_t> d_rel, d_qctx, d_epc, d_part, d_rank;
    DevBuf<unsigned long long> d_tk, d_ekey;
    DevBuf<float> d_score;
    PairJob job(m, contexts, candidates);
    TRY(job.begin());
    if (B == 0 || rel_ptr[B] == rel_ptr[0]) return FMHIP_OK;       // (M == 0 with relevant rows was refused above)
    ScoreCtx &cx = job.pass.cx();
    const int64_t r_lo = rel_ptr[0], r_hi = rel_ptr[B];
    TRY(d_rel.alloc((size_t)(r_hi - r_lo)));
    HIP_TRY(hipMemcpyAsync(d_rel.p, rel + r_lo, (size_t)(r_hi - r_lo) * sizeof(int32_t), hipMemcpyHostToDevice, cx.s));
    const bool with_excl = excl_ptr && excl_ptr[B] > excl_ptr[0];
    if (with_excl) TRY(job.upload_exclusions(excl_ptr, excl));
    std::vector<int32_t> h_qctx, h_epc;       // (rewritten only after the synchronisation that ends a piece)
    for (const BatchMeta &bm : contexts->batches) {       // a chunk of contexts = a batch of their dataset
        const int64_t p_lo = rel_ptr[bm.row0], p_hi = rel_ptr[bm.row0 + bm.rows];
        if (p_lo == p_hi) continue;
        TRY(job.forward_ctx(bm));
        // the order words of the chunk's (context, excluded row) pairs, once for all of its queries
        const int64_t e_lo = with_excl ? excl_ptr[bm.row0] : 0, n_excl = with_excl ? excl_ptr[bm.row0 + bm.rows] - e_lo : 0;
        if (n_excl > 0x7fffffffll) return fail(FMHIP_ERR_UNSUPPORTED, "%lld exclusions in one batch of contexts: fewer than 2^31 are taken", (long long)n_excl);
        PairListArgs la{};
        la.t = job.t;
        if (n_excl > 0) {
            h_epc.resize((size_t)n_excl);
            for (int64_t c = 0; c < bm.rows; ++c)
                std::fill(h_epc.begin() + (excl_ptr[bm.row0 + c] - e_lo), h_epc.begin() + (excl_ptr[bm.row0 + c + 1] - e_lo), (int32_t)c);
            TRY(d_epc.ensure((size_t)n_excl));
            TRY(d_ekey.ensure((size_t)n_excl));
            HIP_TRY(hipMemcpyAsync(d_epc.p, h_epc.data(), (size_t)n_excl * sizeof(int32_t), hipMemcpyHostToDevice, cx.s));
            PairListArgs ea = la;
            ea.pc = d_epc.p;
            ea.pd = job.d_excl.p + e_lo;
            ea.n = n_excl;
            ea.key = d_ekey.p;
            HIP_TRY(launch_pair_list(m->Kp, ea, cx.s));
        }
        for (int64_t q_lo = p_lo; q_lo < p_hi; q_lo += kRankPiece) {
            const int64_t nq = std::min(kRankPiece, p_hi - q_lo);
            h_qctx.resize((size_t)nq);
            {
                int64_t c = std::upper_bound(rel_ptr + bm.row0, rel_ptr + bm.row0 + bm.rows + 1, q_lo) - rel_ptr - 1;
                for (int64_t q = 0; q < nq; ++q) {
                    while (rel_ptr[c + 1] <= q_lo + q) ++c;
                    h_qctx[(size_t)q] = (int32_t)(c - bm.row0);
                }
            }
            int32_t split_len = 0;
            const int splits = topk_splits(nq, M, &split_len);
            TRY(d_qctx.ensure((size_t)nq));
            TRY(d_tk.ensure((size_t)nq));
            TRY(d_score.ensure((size_t)nq));
            TRY(d_rank.ensure((size_t)nq));
            TRY(d_part.ensure((size_t)nq * splits));
            HIP_TRY(hipMemcpyAsync(d_qctx.p, h_qctx.data(), (size_t)nq * sizeof(int32_t), hipMemcpyHostToDevice, cx.s));
            PairListArgs ta = la;
            ta.pc = d_qctx.p;
            ta.pd = d_rel.p + (q_lo - r_lo);
            ta.n = nq;
            ta.key = d_tk.p;
            ta.score = d_score.p;
            HIP_TRY(launch_pair_list(m->Kp, ta, cx.s));
            RankArgs ra{};
            ra.t = job.t;
            ra.qctx = d_qctx.p;
            ra.tk = d_tk.p;
            ra.nq = (int32_t)nq;
            ra.M = (int32_t)M;
            ra.split_len = split_len;
            ra.splits = splits;
            ra.part = d_part.p;
            HIP_TRY(launch_pair_rank(m->Kp, ra, cx.s));
            HIP_TRY(launch_rank_finish(d_part.p, (int32_t)nq, splits, d_tk.p, d_qctx.p, n_excl > 0 ? job.d_eptr.p + bm.row0 : nullptr, e_lo,
                                       d_ekey.p, d_rank.p, cx.s));
            TRY(job.results_back(d_rank.p, rank + q_lo, d_score.p, score ? score + q_lo : nullptr, nq));
        }
    }
    return FMHIP_OK;
}

int fmhip_rank_metrics(int64_t n_contexts, const int64_t *rel_ptr, const int32_t *rank, int32_t k, fmhip_rank_metrics_t *out) {
    if (!out) return fail(FMHIP_ERR_INVALID, "out is NULL");
    if (out->struct_size != (int32_t)sizeof(fmhip_rank_metrics_t))
        return fail(FMHIP_ERR_INVALID, "out->struct_size is %d, not sizeof(fmhip_rank_metrics_t) = %d", (int)out->struct_size,
                    (int)sizeof(fmhip_rank_metrics_t));
    if (k < 1) return fail(FMHIP_ERR_INVALID, "k = %d is below 1", (int)k);
    if (n_contexts < 0) return fail(FMHIP_ERR_INVALID, "n_contexts = %lld is negative", (long long)n_contexts);
    if (n_contexts > 0) {
        if (!rel_ptr) return fail(FMHIP_ERR_INVALID, "rel_ptr is NULL");
        TRY(check_offsets("rel_ptr", rel_ptr, n_contexts));
        if (rel_ptr[n_contexts] > rel_ptr[0] && !rank) return fail(FMHIP_ERR_INVALID, "rank is NULL");
    }
    RankMetricSums s;
    const int64_t bad = rank_metrics(n_contexts, rel_ptr, rank, k, &s);
    if (bad >= 0) return fail(FMHIP_ERR_INVALID, "context %lld holds a negative rank or the same rank twice", (long long)bad);
    out->k = k;
    out->contexts = s.contexts;
    out->skipped = s.skipped;
    out->relevant = s.relevant;
    out->hit_rate = s.hit_rate;
    out->recall = s.recall;
    out->precision = s.precision;
    out->ndcg = s.ndcg;
    out->mrr = s.mrr;
    out->map = s.map;
    return FMHIP_OK;
}

}  // extern "C"

// ---- relational data (include/fmhip_relational.h) ----------------------------------------------------------------------------
// Every block's q-mode pass ONCE (its q rows and predictions into buffers of the call's own), then per batch of data rows the plain
// part's q-mode pass and k_rel_finish in residual mode, whose partials the block reduction of fmhip_logloss sums.
namespace {

struct RelScoreBufs {       // (declared before the pass: freed after it has drained its stream)
    std::vector<std::unique_ptr<DevBuf<float>>> Q, yq;
};

// pair_sums (the BPR trainer; no plain part, even batches): the rows 2j / 2j+1 are scored as pairs — k_pair_score's partials over the
// predictions the finish left, as fmhip_pair_logloss — and [0] = the concordant pairs, [1] = the sum of the pairs' log-losses
// softmax_n > 0 (with pair_sums; include/fmhip_softmax.h): the pairs as interactions of softmax_n — the softmax pre-pass in its
// scoring form (fm_softmax.h; lq nullable) in k_pair_score's place, [0] = the interactions with the positive on top, [1] = the
// sum of the interactions' losses
int rel_score_pass(fmhip_model_t m, fmhip_relational_t R, double *yhat, fmhip_stats *st, double *logloss, double *pair_sums = nullptr,
                   int32_t softmax_n = 0, const float *lq = nullptr) {
    TRY(check_rel_model(m, R));
    RelScoreBufs bufs;
    ScorePass pass(m);
    TRY(pass.begin({R->max_rows, R->max_rows, R->plain ? R->max_rows : -1, true}));
    ScoreCtx &cx = pass.cx();
    RelBufs w{};
    for (size_t i = 0; i < R->rels.size(); ++i) {
        fmhip_dataset_t blk = R->rels[i]->block;
        bufs.Q.emplace_back(new DevBuf<float>());
        bufs.yq.emplace_back(new DevBuf<float>());
        TRY(bufs.Q.back()->alloc((size_t)blk->n_rows * m->Kp));
        TRY(bufs.yq.back()->alloc((size_t)blk->n_rows));
        w.Q[i] = bufs.Q.back()->p;
        w.yq[i] = bufs.yq.back()->p;
    }
    w.P = R->plain ? cx.P.p : nullptr;
    w.e = cx.e.p;
    w.yhat = cx.yhat.p;
    w.bsum = cx.bsum.p;
    TRY(rel_q_forwards(m, R, w, cx.s));
    std::vector<float> hbuf;
    for (size_t b = 0; b < R->batches.size(); ++b) {
        const fmhip_relational::Batch &B = R->batches[b];
        if (R->plain) {
            const FwdArgs a = fwd_args_out(m, R->plain, R->plain->batches[b], cx.P.p, nullptr, nullptr, cx.yhat.p, kLossSquared);
            HIP_TRY(launch_forward(m->Kp, kFwdQ, a, cx.s, nullptr));
        }
        const RelFinishArgs fa = rel_finish_args(m, R, w, B, logloss ? kLossLogistic : kLossSquared);
        int parts = 0;
        HIP_TRY(launch_rel_finish(m->Kp, fa, true, cx.s, &parts));
        if (pair_sums && softmax_n > 0) {
            SoftmaxArgs sa{};
            sa.yhat = cx.yhat.p;
            sa.map = R->rels[1]->map.p + B.row0;
            sa.lq = lq;
            sa.bsum = cx.bsum.p;
            sa.n = softmax_n;
            sa.n_inter = (int32_t)(B.rows / (2 * (int64_t)softmax_n));
            HIP_TRY(launch_softmax_pre(sa, cx.s, &parts));
        } else if (pair_sums) HIP_TRY(launch_pair_score(cx.yhat.p, R->y.p + B.row0, (int32_t)(B.rows / 2), cx.bsum.p, cx.s, &parts));
        HIP_TRY(launch_reduce_blocks(cx.bsum.p, parts, (int32_t)B.rows, nullptr, cx.acc.p, cx.s, logloss != nullptr || pair_sums != nullptr));
        if (yhat) TRY(pass.copy_back(cx.yhat.p, B.rows, 1, 1, hbuf, yhat + B.row0));
    }
    double h[5];
    fmhip_stats s;
    TRY(pass.read(&s, h));
    s.nnz = R->block_nnz + (R->plain ? R->plain->nnz : 0);
    if (st) *st = s;
    if (logloss) *logloss = h[4];
    if (pair_sums) {
        pair_sums[0] = h[0];
        pair_sums[1] = h[4];
    }
    return FMHIP_OK;
}

}  // namespace

namespace fmhip {
namespace host {

int rel_pair_score(fmhip_model_t m, fmhip_relational_t R, double *logloss, double *concordance, fmhip_stats *stats) {
    fmhip_stats st;
    double sums[2] = {0.0, 0.0};
    TRY(rel_score_pass(m, R, nullptr, &st, nullptr, sums));
    const double pairs = (double)(R->n_rows / 2);
    *logloss = pairs > 0 ? sums[1] / pairs : 0.0;
    if (concordance) *concordance = pairs > 0 ? sums[0] / pairs : 0.0;
    if (stats) {
        *stats = st;
        stats->sum_e = 0.0;        // e_2j = -e_2j+1
    }
    return FMHIP_OK;
}

int rel_softmax_score(fmhip_model_t m, fmhip_relational_t R, int32_t n, const float *lq, double *sums, fmhip_stats *stats) {
    fmhip_stats st;
    TRY(rel_score_pass(m, R, nullptr, &st, nullptr, sums, n, lq));
    if (stats) {
        *stats = st;
        stats->sum_e = 0.0;        // e_2p = -e_2p+1
    }
    return FMHIP_OK;
}

}  // namespace host
}  // namespace fmhip

extern "C" {

int fmhip_relational_predict(fmhip_model_t m, fmhip_relational_t r, double *yhat) {
    ReadLock lock(m);
    if (!yhat) return fail(FMHIP_ERR_INVALID, "yhat is NULL");
    return rel_score_pass(m, r, yhat, nullptr, nullptr);
}

int fmhip_relational_rmse(fmhip_model_t m, fmhip_relational_t r, double *rmse, fmhip_stats *stats) {
    ReadLock lock(m);
    if (!rmse) return fail(FMHIP_ERR_INVALID, "rmse is NULL");
    fmhip_stats st;
    TRY(rel_score_pass(m, r, nullptr, &st, nullptr));
    *rmse = st.rows > 0 ? std::sqrt(st.sse / (double)st.rows) : 0.0;
    if (stats) *stats = st;
    return FMHIP_OK;
}

int fmhip_relational_logloss(fmhip_model_t m, fmhip_relational_t r, double *logloss, fmhip_stats *stats) {
    ReadLock lock(m);
    if (!logloss) return fail(FMHIP_ERR_INVALID, "logloss is NULL");
    fmhip_stats st;
    double sum_l = 0.0;
    TRY(rel_score_pass(m, r, nullptr, &st, &sum_l));
    *logloss = st.rows > 0 ? sum_l / (double)st.rows : 0.0;
    if (stats) *stats = st;
    return FMHIP_OK;
}

}  // extern "C"
