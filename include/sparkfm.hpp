// sparkfm.hpp — a header-only C++17 mirror of SparkFM's host classes over the C ABI of libfmhip.so (include/fmhip.h).
//
// SparkFM is compiled JVM code; no JVM exists where this was built, so beside the Python mirror (sparkfm_amd/) and the
// Scala / JNI sources a maintainer would add (jvm/), this is the same surface for a COMPILED host: same class names, same
// argument meaning, same call order and error behaviour as the reference —
//
//     sparkfm::DataSet      S/DataSet.scala:42-62            rows of (label, SparseVector), cache / unpersist, size, dimension
//     sparkfm::Relation, sparkfm::RelationalData   S/fm/bs/* (a stub in the reference)   block-structure FM: blocks + mappings
//     sparkfm::FMModel      S/fm/FMModel.scala:9-63          num_attribute, num_factor, public w0 / w / v, reg0 / regw / regv, predict
//                           S/Model.scala:13-19              computeRMSE
//     sparkfm::FMLearn      S/fm/FMLearn.scala:10-12         the plug-in point: learn(fm, dataset): FMModel
//     sparkfm::HipSGD       (build-defined; SparkFM ships ALS only) one learn = one epoch of mini-batch SGD on the GPU
//     sparkfm::HipALS       S/fm/lib/ALS.scala:15-75,202-208 the reference's own learner in fp64 on the GPU
//     sparkfm::HipBPR       (build-defined) BPR over a contexts and a candidates block, negatives drawn on the device (include/fmhip_bpr.h; n_candidates: include/fmhip_bpr_adaptive.h; sampler: include/fmhip_warp.h)
//     sparkfm::FM           S/fm/FM.scala:25-33, S/fm/impl/FactorizationMachines.scala:30-51   the fit loop
//
// Nothing but include/fmhip.h (the product header), include/fmhip_topk.h (top-K recommendation), include/fmhip_pairing.h (pairwise ranking), include/fmhip_metrics.h (ROC AUC), include/fmhip_ranking.h (ranking evaluation), include/fmhip_weights.h (per-row example weights), include/fmhip_relational.h (relational data) include/fmhip_mcmc.h (the MCMC learner), include/fmhip_mcmc_task.h (its tasks) and include/fmhip_bpr.h (the BPR trainer) is used.  The reference throws JVM exceptions (S/DataCollection.scala:36);
// here a non-zero status of the C ABI becomes sparkfm::Error carrying fmhip_last_error().  Parameters live on the host as in
// the reference (public, mutable: `fm.w0`, `fm.w`, `fm.v` with v[f + i*k] = breeze's column-major DenseMatrix(k, n+1)); every
// call that needs them on the device uploads them first, as jvm/HipSGD.scala does (the fit loop calls `learn` once per
// iteration: S/fm/impl/FactorizationMachines.scala:45).  There is no CPU fallback: every computation is a call into libfmhip.so.
#ifndef SPARKFM_HPP
#define SPARKFM_HPP

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <random>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "fmhip.h"
#include "fmhip_topk.h"
#include "fmhip_pairing.h"
#include "fmhip_metrics.h"
#include "fmhip_ranking.h"
#include "fmhip_weights.h"
#include "fmhip_relational.h"
#include "fmhip_mcmc.h"
#include "fmhip_mcmc_task.h"
#include "fmhip_mcmc_groups.h"
#include "fmhip_mcmc_relational.h"
#include "fmhip_bpr.h"
#include "fmhip_bpr_adaptive.h"
#include "fmhip_warp.h"
#include "fmhip_redraw.h"
#include "fmhip_proposal.h"
#include "fmhip_softmax.h"
#include "fmhip_ftrl.h"

namespace sparkfm {

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string &what) : std::runtime_error("fmhip error " + std::to_string(c) + ": " + what), code(c) {}
};
inline void check(int rc) {
    if (rc != FMHIP_OK) throw Error(rc, fmhip_last_error());
}

// breeze.linalg.SparseVector[Double] as the reference uses it: index / data in stored order (need not be sorted)
struct SparseVector {
    std::vector<int32_t> index;
    std::vector<double> data;
};

// S/DataSet.scala:42-62 — the rows live on the host until cache() uploads them (mini-batches of batch_rows rows; 0 = one batch,
// what HipALS needs); unpersist() drops the device copy (S/fm/impl/FactorizationMachines.scala:36,48)
// weights (optional; empty = an unweighted dataset): one example weight c_r >= 0 per row — every training path then forms
// e_r <- c_r * e_r (include/fmhip_weights.h); their values are checked when cache() moves the rows to the device
class DataSet {
  public:
    explicit DataSet(const std::vector<std::pair<double, SparseVector>> &rows, int64_t batch_rows = 0, int device = 0,
                     std::vector<double> weights = {})
        : weights_(std::move(weights)), batch_rows_(batch_rows), device_(device) {
        row_ptr_.push_back(0);
        for (const auto &r : rows) {
            if (r.second.index.size() != r.second.data.size()) throw Error(FMHIP_ERR_INVALID, "index / data length mismatch");
            col_.insert(col_.end(), r.second.index.begin(), r.second.index.end());
            val_.insert(val_.end(), r.second.data.begin(), r.second.data.end());
            y_.push_back(r.first);
            row_ptr_.push_back((int64_t)col_.size());
        }
        check_weights();
    }
    DataSet(std::vector<int64_t> row_ptr, std::vector<int32_t> col, std::vector<double> val, std::vector<double> y, int64_t batch_rows = 0, int device = 0,
            std::vector<double> weights = {})
        : row_ptr_(std::move(row_ptr)), col_(std::move(col)), val_(std::move(val)), y_(std::move(y)), weights_(std::move(weights)),
          batch_rows_(batch_rows), device_(device) {
        if (row_ptr_.size() != y_.size() + 1) throw Error(FMHIP_ERR_INVALID, "row_ptr must have one entry more than there are labels");
        check_weights();
    }
    DataSet(const DataSet &) = delete;
    DataSet &operator=(const DataSet &) = delete;
    ~DataSet() { (void)fmhip_dataset_destroy(h_); }

    DataSet &cache() {      // dataset.cache() + transposeInput (S/DataSet.scala:48-62)
        if (h_) return *this;
        if (weights_.empty()) {
            check(fmhip_dataset_create(device_, (int64_t)y_.size(), row_ptr_.data(), col_.data(), val_.data(), y_.data(), batch_rows_, &h_));
        } else {
            fmhip_dataset_opts opts{(int32_t)sizeof(fmhip_dataset_opts), -1, batch_rows_, -1};
            check(fmhip_dataset_create_weighted(device_, (int64_t)y_.size(), row_ptr_.data(), col_.data(), val_.data(), y_.data(), weights_.data(), &opts, &h_));
        }
        return *this;
    }
    DataSet &unpersist() {
        check(fmhip_dataset_destroy(h_));
        h_ = nullptr;
        return *this;
    }
    int64_t size() const { return (int64_t)y_.size(); }                 // S/DataSet.scala:23-25
    int64_t dimension() const {                                           // S/DataSet.scala:27-29: the largest feature index
        int64_t d = 0;
        for (int32_t c : col_) d = c > d ? c : d;
        return d;
    }
    int64_t n_batches() {
        int64_t nb = 0;
        check(fmhip_dataset_info(cache().h_, nullptr, nullptr, nullptr, nullptr, &nb));
        return nb;
    }
    const std::vector<double> &labels() const { return y_; }
    const std::vector<double> &weights() const { return weights_; }       // empty: unweighted
    int64_t batch_rows() const { return batch_rows_; }
    int64_t nnz() const { return (int64_t)col_.size(); }
    fmhip_dataset_t handle() { return cache().h_; }
    int device() const { return device_; }

  private:
    void check_weights() const {
        if (!weights_.empty() && weights_.size() != y_.size()) throw Error(FMHIP_ERR_INVALID, "weights must hold one weight per row");
    }
    std::vector<int64_t> row_ptr_;
    std::vector<int32_t> col_;
    std::vector<double> val_, y_, weights_;
    int64_t batch_rows_;
    int device_;
    fmhip_dataset_t h_ = nullptr;
};

// Relational data (include/fmhip_relational.h; the reference's S/fm/bs/* is a stub): a Relation is a BLOCK of feature rows — a
// one-batch DataSet with labels 0 — and a MAPPING, data row r using block row mapping[r]; a RelationalData is N labels, one or more
// relations and an optional plain part (a DataSet of the same N rows, batched by the same batch_rows).  It stands for the flat
// DataSet whose row r holds relation 0's entries of block row mapping_0[r], then relation 1's, ..., then the plain part's —
// without building it.  Feature ids are global and the parts' feature sets must be disjoint (checked by the library).  Relations
// and the plain part are BORROWED: they must outlive the RelationalData.
class Relation {
  public:
    Relation(const std::vector<SparseVector> &rows, std::vector<int32_t> mapping, int device = 0)
        : block_(labelled(rows), 0, device), mapping_(std::move(mapping)) {}
    DataSet &block() { return block_; }
    const std::vector<int32_t> &mapping() const { return mapping_; }

  private:
    static std::vector<std::pair<double, SparseVector>> labelled(const std::vector<SparseVector> &rows) {
        std::vector<std::pair<double, SparseVector>> out;
        for (const auto &r : rows) out.emplace_back(0.0, r);
        return out;
    }
    DataSet block_;
    std::vector<int32_t> mapping_;
};

class RelationalData {
  public:
    RelationalData(std::vector<double> y, std::vector<Relation *> relations, DataSet *plain = nullptr, int64_t batch_rows = 0, int device = 0)
        : y_(std::move(y)), relations_(std::move(relations)), plain_(plain), batch_rows_(batch_rows), device_(device) {
        if (relations_.empty()) throw Error(FMHIP_ERR_INVALID, "a RelationalData needs at least one Relation");
        for (Relation *r : relations_)
            if (!r || r->mapping().size() != y_.size()) throw Error(FMHIP_ERR_INVALID, "every mapping must hold one block row per data row");
    }
    RelationalData(const RelationalData &) = delete;
    RelationalData &operator=(const RelationalData &) = delete;
    ~RelationalData() { (void)fmhip_relational_destroy(h_); }

    RelationalData &cache() {
        if (h_) return *this;
        std::vector<fmhip_dataset_t> blocks;
        std::vector<const int32_t *> maps;
        for (Relation *r : relations_) {
            blocks.push_back(r->block().handle());
            maps.push_back(r->mapping().data());
        }
        check(fmhip_relational_create(device_, (int64_t)y_.size(), y_.data(), (int32_t)blocks.size(), blocks.data(), maps.data(),
                                      plain_ ? plain_->handle() : nullptr, batch_rows_, &h_));
        return *this;
    }
    RelationalData &unpersist() {       // the relational handle only: the blocks stay cached with their Relation
        check(fmhip_relational_destroy(h_));
        h_ = nullptr;
        return *this;
    }
    int64_t size() const { return (int64_t)y_.size(); }
    int64_t dimension() {
        int64_t d = plain_ ? plain_->dimension() : 0;
        for (Relation *r : relations_) d = std::max<int64_t>(d, r->block().dimension());
        return d;
    }
    int64_t n_batches() {
        int64_t nb = 0;
        check(fmhip_relational_info(cache().h_, nullptr, nullptr, nullptr, &nb, nullptr));
        return nb;
    }
    const std::vector<double> &labels() const { return y_; }
    int32_t n_parts() const { return (int32_t)relations_.size() + (plain_ ? 1 : 0); }     // the relations, then the plain part
    fmhip_relational_t handle() { return cache().h_; }
    int device() const { return device_; }

  private:
    std::vector<double> y_;
    std::vector<Relation *> relations_;
    DataSet *plain_;
    int64_t batch_rows_;
    int device_;
    fmhip_relational_t h_ = nullptr;
};

// S/fm/FMModel.scala:9-63 — `new FMModel(num_attribute, num_factor)`: w0 = 0, w = 0, v ~ N(mean, stdev) (:17-22; the reference's
// draw is unseeded — quirk Q2 — so parity runs assign w0 / w / v explicitly)
class FMModel {
  public:
    const int64_t num_attribute;
    const int32_t num_factor;
    double w0 = 0.0;
    std::vector<double> w, v;                       // w[n+1]; v[k * (n+1)], element (f, i) at f + i*k
    double reg0 = 0.0, regw = 0.0, regv = 10.0;     // S/fm/FMModel.scala:29-31 (ALS ridge terms; HipSGD carries its own)

    FMModel(int64_t numAttribute, int32_t numFactor, double mean = 0.0, double stdev = 0.01, uint64_t seed = 0, int device = 0)
        : num_attribute(numAttribute), num_factor(numFactor), w((size_t)numAttribute + 1, 0.0), v((size_t)numFactor * ((size_t)numAttribute + 1)), device_(device) {
        std::mt19937_64 gen(seed);
        std::normal_distribution<double> dist(mean, stdev);
        for (double &x : v) x = dist(gen);
    }
    FMModel(const FMModel &) = delete;
    FMModel &operator=(const FMModel &) = delete;
    FMModel(FMModel &&o) noexcept
        : num_attribute(o.num_attribute), num_factor(o.num_factor), w0(o.w0), w(std::move(o.w)), v(std::move(o.v)), reg0(o.reg0), regw(o.regw), regv(o.regv),
          device_(o.device_), h_(o.h_) {
        o.h_ = nullptr;
    }
    ~FMModel() { (void)fmhip_model_destroy(h_); }

    double predict(const SparseVector &features) {                        // S/fm/FMModel.scala:34-55
        const int64_t rp[2] = {0, (int64_t)features.index.size()};
        double yhat = 0.0;
        check(fmhip_predict_rows(upload(), 1, rp, features.index.data(), features.data.data(), &yhat));
        return yhat;
    }
    std::vector<double> predict(DataSet &dataset) {                       // dataset.rdd.mapValues(predict), S/Model.scala:14
        std::vector<double> yhat((size_t)dataset.size());
        check(fmhip_predict(upload(), dataset.handle(), yhat.data()));
        return yhat;
    }
    double computeRMSE(DataSet &dataset) {                                // S/Model.scala:13-19
        double rmse = 0.0;
        check(fmhip_rmse(upload(), dataset.handle(), &rmse, nullptr));
        return rmse;
    }
    // ... and of relational data (fmhip_relational_predict / _rmse / _logloss: every block's forward once per call)
    std::vector<double> predict(RelationalData &dataset) {
        std::vector<double> yhat((size_t)dataset.size());
        check(fmhip_relational_predict(upload(), dataset.handle(), yhat.data()));
        return yhat;
    }
    double computeRMSE(RelationalData &dataset) {
        double rmse = 0.0;
        check(fmhip_relational_rmse(upload(), dataset.handle(), &rmse, nullptr));
        return rmse;
    }
    double computeLogLoss(RelationalData &dataset) {
        double logloss = 0.0;
        check(fmhip_relational_logloss(upload(), dataset.handle(), &logloss, nullptr));
        return logloss;
    }
    double computeLogLoss(DataSet &dataset) {    // mean log-loss of sigmoid(predict) against t = [y > 0], whatever the training loss
        double logloss = 0.0;
        check(fmhip_logloss(upload(), dataset.handle(), &logloss, nullptr));
        return logloss;
    }
    // The weighted scores of predict over a WEIGHTED dataset (fmhip_weighted_scores): sum_w, rmse = sqrt(sum c (yhat - y)^2 / sum c),
    // mae, logloss, rows, nonfinite; NaN ratios when the weights sum to 0.  computeRMSE / computeLogLoss ignore the weights.
    fmhip_weighted_result weightedScores(DataSet &dataset) {
        fmhip_weighted_result r{};
        r.struct_size = (int32_t)sizeof r;
        check(fmhip_weighted_scores(upload(), dataset.handle(), &r));
        return r;
    }
    // Exact sparsity counts of the model as uploaded (fmhip_model_nonzeros, include/fmhip_ftrl.h): nonzero w, nonzero v, and the
    // features whose w and whole v row are zero — what FTRL-Proximal's L1 (HipFTRL) leaves behind
    struct Nonzeros {
        int64_t w_nonzero = 0, v_nonzero = 0, features_all_zero = 0;
    };
    Nonzeros nonzeros() {
        Nonzeros z;
        check(fmhip_model_nonzeros(upload(), &z.w_nonzero, &z.v_nonzero, &z.features_all_zero));
        return z;
    }
    // Pairwise ranking score of the pairs (rows 2j, 2j+1) of `dataset` (fmhip_pair_logloss): the mean of -log sigmoid(+-d) over the
    // pairs' margins d = predict(row 2j) - predict(row 2j+1), the sign by which row carries the larger label ...
    double computePairLogLoss(DataSet &dataset) {
        double logloss = 0.0;
        check(fmhip_pair_logloss(upload(), dataset.handle(), &logloss, nullptr, nullptr));
        return logloss;
    }
    // ... and the share of the pairs the model orders as their labels do (a tie counts one half): the pairwise AUC
    double computePairAccuracy(DataSet &dataset) {
        double logloss = 0.0, concordance = 0.0;
        check(fmhip_pair_logloss(upload(), dataset.handle(), &logloss, &concordance, nullptr));
        return concordance;
    }

    // ROC AUC of predict against the labels t = [y > 0] (fmhip_auc), ranked on the device, exactly: the share of (positive,
    // negative) pairs the model orders correctly, a tie counting one half; NaN when there is no such pair ...
    double computeAUC(DataSet &dataset) { return aucDetails(dataset, nullptr).auc; }
    // ... and GAUC: the AUC inside each group of rows (groups[r]: any id in [0, 2^31), one per row — a user's impressions),
    // averaged by the groups' row counts over the groups that hold both classes
    double computeGroupAUC(DataSet &dataset, const std::vector<int32_t> &groups) { return aucDetails(dataset, &groups).gauc; }
    // every field of the result (the exact integer counts beside the two ratios)
    fmhip_auc_result aucDetails(DataSet &dataset, const std::vector<int32_t> *groups = nullptr) {
        if (groups && (int64_t)groups->size() != dataset.size()) throw Error(FMHIP_ERR_INVALID, "groups must hold one id per row");
        fmhip_auc_result r{};
        r.struct_size = (int32_t)sizeof r;
        check(fmhip_auc(upload(), dataset.handle(), groups ? groups->data() : nullptr, &r, nullptr));
        return r;
    }

    // Per row of `contexts` the k rows of `candidates` the model ranks highest (fmhip_topk): the users x items ranking of
    // S/driver.scala:100-112, a pair's score being predict (S/fm/FMModel.scala:34) of "the context's entries, then the
    // candidate's".  idx[c * k + j]: candidate rows, best first, -1 past the last one; score (nullable) beside it.
    // exclude (nullable): per context the candidate rows that must not be returned, ascending and distinct.
    std::vector<int32_t> recommend(DataSet &contexts, DataSet &candidates, int32_t k, std::vector<double> *score = nullptr,
                                   const std::vector<std::vector<int32_t>> *exclude = nullptr) {
        if (k < 1 || k > FMHIP_TOPK_MAX) throw Error(FMHIP_ERR_INVALID, "k outside [1, FMHIP_TOPK_MAX]");
        const size_t B = (size_t)contexts.size();
        std::vector<int64_t> eptr;
        std::vector<int32_t> eidx;
        if (exclude) {
            if (exclude->size() != B) throw Error(FMHIP_ERR_INVALID, "exclude must hold one list per context");
            eptr.push_back(0);
            for (const auto &e : *exclude) {
                eidx.insert(eidx.end(), e.begin(), e.end());
                eptr.push_back((int64_t)eidx.size());
            }
            if (eidx.empty()) eidx.push_back(0);       // (a non-NULL pointer beside eptr)
        }
        std::vector<int32_t> idx(B * (size_t)k);
        if (B == 0) return idx;
        if (score) score->assign(B * (size_t)k, 0.0);
        check(fmhip_topk(upload(), contexts.handle(), candidates.handle(), k, exclude ? eptr.data() : nullptr,
                         exclude ? eidx.data() : nullptr, idx.data(), score ? score->data() : nullptr));
        return idx;
    }

    // Where the model ranks given candidates (fmhip_rank): relevant[c] = the candidate rows held out for context c, ascending and
    // distinct; -> per context the 0-based position of each of them in the context's COMPLETE ranking (what recommend would
    // return with k = candidates.size()), counted on the device.  exclude (nullable): per context the rows that are not in the
    // ranking; score (nullable): the relevant rows' scores, in the order of the ranks.
    std::vector<std::vector<int32_t>> rankOf(DataSet &contexts, DataSet &candidates, const std::vector<std::vector<int32_t>> &relevant,
                                             const std::vector<std::vector<int32_t>> *exclude = nullptr,
                                             std::vector<std::vector<double>> *score = nullptr) {
        const size_t B = (size_t)contexts.size();
        if (relevant.size() != B) throw Error(FMHIP_ERR_INVALID, "relevant must hold one list per context");
        if (exclude && exclude->size() != B) throw Error(FMHIP_ERR_INVALID, "exclude must hold one list per context");
        std::vector<int64_t> rptr, eptr;
        std::vector<int32_t> ridx, eidx;
        flatten(relevant, rptr, ridx);
        if (exclude) flatten(*exclude, eptr, eidx);
        std::vector<int32_t> rank(ridx.size());
        std::vector<double> sc(score ? ridx.size() : 0);
        check(fmhip_rank(upload(), contexts.handle(), candidates.handle(), rptr.data(), ridx.data(), exclude ? eptr.data() : nullptr,
                         exclude ? eidx.data() : nullptr, rank.data(), score ? sc.data() : nullptr));
        std::vector<std::vector<int32_t>> out(B);
        if (score) score->assign(B, std::vector<double>());
        for (size_t c = 0; c < B; ++c) {
            out[c].assign(rank.begin() + rptr[c], rank.begin() + rptr[c + 1]);
            if (score) (*score)[c].assign(sc.begin() + rptr[c], sc.begin() + rptr[c + 1]);
        }
        return out;
    }
    // HitRate@k, Recall@k, Precision@k, NDCG@k, MRR and MAP of those ranks (fmhip_rank_metrics, on the host), averaged over the
    // contexts that have a relevant row
    fmhip_rank_metrics_t computeRankingMetrics(DataSet &contexts, DataSet &candidates, const std::vector<std::vector<int32_t>> &relevant,
                                               int32_t k = 10, const std::vector<std::vector<int32_t>> *exclude = nullptr) {
        if (k < 1) throw Error(FMHIP_ERR_INVALID, "k must be >= 1");
        return rankingMetrics(rankOf(contexts, candidates, relevant, exclude), k);
    }
    static fmhip_rank_metrics_t rankingMetrics(const std::vector<std::vector<int32_t>> &ranks, int32_t k) {
        std::vector<int64_t> ptr;
        std::vector<int32_t> flat;
        flatten(ranks, ptr, flat);
        fmhip_rank_metrics_t r{};
        r.struct_size = (int32_t)sizeof r;
        check(fmhip_rank_metrics((int64_t)ranks.size(), ptr.data(), flat.data(), k, &r));
        return r;
    }

    // the device replica: created on first use, refreshed from the host fields before every use (they are public and mutable)
    fmhip_model_t upload() {
        if (!h_) check(fmhip_model_create(device_, num_attribute, num_factor, nullptr, &h_));
        check(fmhip_model_set_params(h_, w0, w.data(), v.data()));
        return h_;
    }
    void download() { check(fmhip_model_get_params(h_, &w0, w.data(), v.data())); }

  private:
    // per-context lists -> offsets [n + 1] and the rows in one array (never empty: a non-NULL pointer)
    static void flatten(const std::vector<std::vector<int32_t>> &lists, std::vector<int64_t> &ptr, std::vector<int32_t> &rows) {
        ptr.assign(1, 0);
        rows.clear();
        for (const auto &e : lists) {
            rows.insert(rows.end(), e.begin(), e.end());
            ptr.push_back((int64_t)rows.size());
        }
        rows.reserve(1);
    }
    int device_;
    fmhip_model_t h_ = nullptr;
};

// S/fm/FMLearn.scala:10-12 — the plug-in point; the model is mutated in place and returned (S/fm/lib/ALS.scala:27,40,64,74)
class FMLearn {
  public:
    virtual ~FMLearn() = default;
    virtual FMModel &learn(FMModel &fm, DataSet &dataset) = 0;
    // relational data: a learner that does not train on it says so
    virtual FMModel &learn(FMModel &, RelationalData &) { throw Error(FMHIP_ERR_UNSUPPORTED, "this learner does not train on relational data"); }
    // a learner that trains on more than the fit loop's dataset says how wide the model must be (HipBPR: the larger of its two blocks')
    virtual int64_t dimension() { return 0; }
};

// One learn = one epoch of mini-batch SGD over the dataset's batches (ascending order) — fmhip_sgd_epoch.
// theta <- theta - eta * (sum_{r in batch} e_r h_r(theta) / |batch| + reg * theta), e and h from S/fm/lib/ALS.scala:142-144, :56-58 / :40 / :21
// loss = FMHIP_LOSS_LOGISTIC: e = sigmoid(yhat) - [y > 0], a binary classifier (fmhip_model_set_loss)
// optimizer = FMHIP_OPT_ADAGRAD: per-coordinate steps, g_hat = g/|batch| + reg*theta, n += g_hat^2, theta -= eta*g_hat/(sqrt(n) + adagrad_eps),
// n started at adagrad_init (fmhip_model_set_optimizer; set before every epoch — the same settings keep the accumulators)
// pairs = true: rows 2j and 2j+1 of a batch are one example, the loss applied to their difference (pairwise ranking: BPR under the
// logistic loss with the preferred row first; fmhip_model_set_pairing) — the dataset needs an even row count and an even batch_rows
class HipSGD : public FMLearn {
  public:
    double eta, reg0, regw, regv;
    int loss;
    int optimizer;
    double adagrad_eps, adagrad_init;
    bool pairs;
    fmhip_stats last_stats{};
    explicit HipSGD(double eta_ = 0.05, double reg0_ = 0.0, double regw_ = 0.0, double regv_ = 0.0, int loss_ = FMHIP_LOSS_SQUARED,
                    int optimizer_ = FMHIP_OPT_SGD, double adagrad_eps_ = 1e-10, double adagrad_init_ = 0.1, bool pairs_ = false)
        : eta(eta_), reg0(reg0_), regw(regw_), regv(regv_), loss(loss_), optimizer(optimizer_), adagrad_eps(adagrad_eps_),
          adagrad_init(adagrad_init_), pairs(pairs_) {}
    static HipSGD run(double eta = 0.05, double reg0 = 0.0, double regw = 0.0, double regv = 0.0, int loss = FMHIP_LOSS_SQUARED,
                      int optimizer = FMHIP_OPT_SGD, double adagrad_eps = 1e-10, double adagrad_init = 0.1, bool pairs = false) {
        return HipSGD(eta, reg0, regw, regv, loss, optimizer, adagrad_eps, adagrad_init, pairs);   // cf. ALS.run(), S/fm/lib/ALS.scala:202-208
    }
    FMModel &learn(FMModel &fm, DataSet &dataset) override {
        check(fmhip_model_set_loss(fm.upload(), loss));
        check(fmhip_model_set_pairing(fm.upload(), pairs ? FMHIP_PAIRING_ADJACENT : FMHIP_PAIRING_NONE));
        check(fmhip_model_set_optimizer(fm.upload(), optimizer, adagrad_eps, adagrad_init));
        check(fmhip_sgd_epoch(fm.upload(), dataset.handle(), eta, reg0, regw, regv, nullptr, &last_stats));
        fm.download();
        return fm;
    }
    // one epoch of relational steps (fmhip_relational_sgd_epoch): every block walked once per step; not with pairs
    FMModel &learn(FMModel &fm, RelationalData &dataset) override {
        check(fmhip_model_set_loss(fm.upload(), loss));
        check(fmhip_model_set_pairing(fm.upload(), pairs ? FMHIP_PAIRING_ADJACENT : FMHIP_PAIRING_NONE));
        check(fmhip_model_set_optimizer(fm.upload(), optimizer, adagrad_eps, adagrad_init));
        check(fmhip_relational_sgd_epoch(fm.upload(), dataset.handle(), eta, reg0, regw, regv, nullptr, &last_stats));
        fm.download();
        return fm;
    }
};

// HipSGD under FTRL-Proximal with L1 (include/fmhip_ftrl.h): per-coordinate rates like AdaGrad's plus an L1 term that leaves most of a
// wide model exactly zero (FMModel::nonzeros).  alpha: the step size; beta: added to sqrt(n) in every rate; l1w, l1v: the L1 of the
// linear weights and of the factors (w0 has none); l2_0, l2w, l2v: the L2 of the rule's closed form — no decay: a parameter whose
// gradient is zero keeps every bit; ftrl_init: what the accumulators start at.  The rule is put on the model before every epoch (the
// same settings keep its state; the model's upload before each call writes its own values back, which keeps it too).
class HipFTRL : public FMLearn {
  public:
    double alpha, beta, l1w, l1v, l2_0, l2w, l2v, ftrl_init;
    int loss;
    bool pairs;
    fmhip_stats last_stats{};
    explicit HipFTRL(double alpha_ = 0.1, double beta_ = 1.0, double l1w_ = 0.0, double l1v_ = 0.0, double l2_0_ = 0.0, double l2w_ = 0.0,
                     double l2v_ = 0.0, double ftrl_init_ = 0.0, int loss_ = FMHIP_LOSS_SQUARED, bool pairs_ = false)
        : alpha(alpha_), beta(beta_), l1w(l1w_), l1v(l1v_), l2_0(l2_0_), l2w(l2w_), l2v(l2v_), ftrl_init(ftrl_init_), loss(loss_),
          pairs(pairs_) {}
    static HipFTRL run(double alpha = 0.1, double beta = 1.0, double l1w = 0.0, double l1v = 0.0, double l2_0 = 0.0, double l2w = 0.0,
                       double l2v = 0.0, double ftrl_init = 0.0, int loss = FMHIP_LOSS_SQUARED, bool pairs = false) {
        return HipFTRL(alpha, beta, l1w, l1v, l2_0, l2w, l2v, ftrl_init, loss, pairs);
    }
    FMModel &learn(FMModel &fm, DataSet &dataset) override {
        check(fmhip_sgd_epoch(set_rule(fm), dataset.handle(), alpha, l2_0, l2w, l2v, nullptr, &last_stats));
        fm.download();
        return fm;
    }
    FMModel &learn(FMModel &fm, RelationalData &dataset) override {
        check(fmhip_relational_sgd_epoch(set_rule(fm), dataset.handle(), alpha, l2_0, l2w, l2v, nullptr, &last_stats));
        fm.download();
        return fm;
    }

  private:
    fmhip_model_t set_rule(FMModel &fm) {
        fmhip_model_t m = fm.upload();
        check(fmhip_model_set_loss(m, loss));
        check(fmhip_model_set_pairing(m, pairs ? FMHIP_PAIRING_ADJACENT : FMHIP_PAIRING_NONE));
        check(fmhip_model_set_ftrl(m, beta, ftrl_init, l1w, l1v));
        return m;
    }
};

// The reference's own learner: one learn = one ALS.learn pass (S/fm/lib/ALS.scala:15-75) in fp64 on the GPU, with the MODEL's
// regularisers as the reference uses them (:21, :40, :56).  Needs a one-batch DataSet (batch_rows = 0).
class HipALS : public FMLearn {
  public:
    static HipALS run() { return HipALS(); }
    using FMLearn::learn;
    FMModel &learn(FMModel &fm, DataSet &dataset) override {
        check(fmhip_als_epoch(fm.upload(), dataset.handle(), fm.reg0, fm.regw, fm.regv));
        fm.download();
        return fm;
    }
};

// Bayesian FM by Gibbs sampling on the ALS column walk (include/fmhip_mcmc.h; libFM's MCMC learner, of which the reference's ALS.scala
// is the cut-down copy): one learn = one Gibbs sweep in fp64.  Nothing to tune: the noise precision alpha and every group's
// regulariser lambda and prior mean mu are sampled; the prediction is the average over the draws — of `test` (a one-batch DataSet
// that must outlive the learner; nullptr: none), since the burn-in ended (the running average is reset once, after burn_in epochs).
// opts (public: seed, sample, reg0, init_lambda, libFM's priors) are read when the handle is made — by the first learn for a
// (model, dataset) pair; close() frees it, and must come before the dataset's device copy is dropped and used again.
// task_opts (include/fmhip_mcmc_task.h; read with opts): task = FMHIP_MCMC_CLASSIFICATION trains on the probit link's latent targets
// (latentTargets()), and predictions() / lastPredictions() are then probabilities Phi(yhat), scored by computeLogLoss() and
// computeAccuracy() (computeRMSE() throws); the model holds the last draw, whose score is the probit score — not a logistic one.
// Regression: clip + clip_lo / clip_hi clamp every draw's test prediction; clip_to_labels takes the train labels' min and max.
// setGroups (include/fmhip_mcmc_groups.h; before the first learn): one attribute-group id per feature — at least the model's
// num_attribute of them — and lambda and mu are sampled per (parameter group, attribute group): State's lambda and mu then hold
// (k + 1) * G values, [g * G + a], and groupCounts() the trained features of every group.
// learn(fm, RelationalData) (include/fmhip_mcmc_relational.h) sweeps a one-batch relational train set BY BLOCKS, never expanded — the
// random numbers of the flat run on the expanded rows.  setTest(RelationalData *) gives it a relational test set (normally the
// train set's blocks under other mappings; the DataSet of the constructor serves as well); setPartGroups() makes every part —
// relation 0, 1, ..., the plain part — an attribute group (a group table is not taken with relational data).
class HipMCMC : public FMLearn {
  public:
    struct State {
        double alpha = 1.0;
        std::vector<double> lambda, mu;             // k + 1 each: group 0 = w, 1 + f = factor f; with groups (k + 1) * G each, [g * G + a]
        int64_t iterations = 0;
    };
    fmhip_mcmc_opts opts;
    fmhip_mcmc_task_opts task_opts;
    bool clip_to_labels = false;
    int64_t burn_in;
    fmhip_mcmc_stats last_stats{};
    explicit HipMCMC(uint64_t seed = 0, DataSet *test = nullptr, int64_t burn_in_ = 0, bool sample = true, int32_t task = FMHIP_MCMC_REGRESSION)
        : burn_in(burn_in_), test_(test) {
        check(fmhip_mcmc_opts_default(&opts));
        check(fmhip_mcmc_task_opts_default(&task_opts));
        task_opts.task = task;
        opts.seed = seed;
        opts.sample = sample ? 1 : 0;
    }
    static HipMCMC run(uint64_t seed = 0, DataSet *test = nullptr, int64_t burn_in = 0, bool sample = true, int32_t task = FMHIP_MCMC_REGRESSION) {
        return HipMCMC(seed, test, burn_in, sample, task);
    }
    void setClip(double lo, double hi) {            // regression: clamp every draw's test prediction to [lo, hi]
        task_opts.clip = 1;
        task_opts.clip_lo = lo;
        task_opts.clip_hi = hi;
        clip_to_labels = false;
    }
    void setGroups(const std::vector<int32_t> &groups, int32_t n_groups = 0) {      // n_groups 0: the largest id + 1
        if (h_) throw Error(FMHIP_ERR_INVALID, "the attribute groups are set before the first learn");
        int32_t most = 0;
        for (size_t i = 0; i < groups.size(); ++i) {
            if (groups[i] < 0) throw Error(FMHIP_ERR_INVALID, "feature " + std::to_string(i) + " has a negative group id");
            most = std::max(most, groups[i]);
        }
        if (n_groups != 0 && n_groups <= most) throw Error(FMHIP_ERR_INVALID, "n_groups is below the largest group id + 1");
        groups_ = groups;
        n_groups_ = n_groups != 0 ? n_groups : most + 1;
        grouped_ = true;
    }
    void setPartGroups() {                          // relational data: a part is an attribute group
        if (h_) throw Error(FMHIP_ERR_INVALID, "the attribute groups are set before the first learn");
        part_groups_ = true;
    }
    void setTest(RelationalData *test) {            // a relational test set, in the DataSet's place
        if (h_) throw Error(FMHIP_ERR_INVALID, "the test set is given before the first learn");
        rel_test_ = test;
        test_ = nullptr;
    }
    int32_t numGroups() const { return n_groups_; }
    HipMCMC(const HipMCMC &) = delete;
    HipMCMC &operator=(const HipMCMC &) = delete;
    ~HipMCMC() override { (void)fmhip_mcmc_destroy(h_); }

    using FMLearn::learn;
    FMModel &learn(FMModel &fm, DataSet &dataset) override {
        fmhip_model_t m = fm.upload();
        fmhip_dataset_t d = dataset.handle();
        if (h_ && (m != m_ || d != d_)) close();
        if (!h_) {
            fmhip_mcmc_task_opts to = task_opts;
            if (clip_to_labels) {
                if (dataset.labels().empty()) throw Error(FMHIP_ERR_INVALID, "clip_to_labels needs a train set with rows");
                const auto range = std::minmax_element(dataset.labels().begin(), dataset.labels().end());
                to.clip = 1;
                to.clip_lo = *range.first;
                to.clip_hi = *range.second;
            }
            if (grouped_ && (int64_t)groups_.size() < fm.num_attribute)
                throw Error(FMHIP_ERR_INVALID, "groups holds " + std::to_string(groups_.size()) + " ids but the model has num_attribute = " +
                                                   std::to_string(fm.num_attribute));
            check(fmhip_mcmc_create_task(m, d, test_ ? test_->handle() : nullptr, &opts, &to, &h_));
            if (grouped_) {
                const int rc = fmhip_mcmc_set_groups(h_, groups_.data(), fm.num_attribute, n_groups_);
                if (rc != FMHIP_OK) {
                    (void)fmhip_mcmc_destroy(h_);
                    h_ = nullptr;
                    check(rc);
                }
            }
            n_train_ = dataset.size();
            classification_ = to.task == FMHIP_MCMC_CLASSIFICATION;
            m_ = m;
            d_ = d;
            r_ = nullptr;
            k_ = fm.num_factor;
            if (pending_) {
                pending_ = false;
                setState(pending_state_.alpha, pending_state_.lambda, pending_state_.mu);
            }
        }
        check(fmhip_mcmc_epoch(h_, &last_stats));
        fm.download();
        if (burn_in > 0 && last_stats.iterations == burn_in) check(fmhip_mcmc_reset_average(h_));
        return fm;
    }
    FMModel &learn(FMModel &fm, RelationalData &dataset) override {
        fmhip_model_t m = fm.upload();
        fmhip_relational_t r = dataset.handle();
        if (h_ && (m != m_ || r != r_)) close();
        if (!h_) {
            if (grouped_ && !part_groups_)
                throw Error(FMHIP_ERR_UNSUPPORTED, "relational data takes no group table: setPartGroups() makes every part an attribute group");
            fmhip_mcmc_task_opts to = task_opts;
            if (clip_to_labels) {
                if (dataset.labels().empty()) throw Error(FMHIP_ERR_INVALID, "clip_to_labels needs a train set with rows");
                const auto range = std::minmax_element(dataset.labels().begin(), dataset.labels().end());
                to.clip = 1;
                to.clip_lo = *range.first;
                to.clip_hi = *range.second;
            }
            check(fmhip_mcmc_create_relational(m, r, rel_test_ ? rel_test_->handle() : nullptr, test_ ? test_->handle() : nullptr, &opts, &to,
                                               part_groups_ ? 1 : 0, &h_));
            if (part_groups_) {
                grouped_ = true;
                n_groups_ = dataset.n_parts();
            }
            n_train_ = dataset.size();
            classification_ = to.task == FMHIP_MCMC_CLASSIFICATION;
            m_ = m;
            r_ = r;
            d_ = nullptr;
            k_ = fm.num_factor;
            if (pending_) {
                pending_ = false;
                setState(pending_state_.alpha, pending_state_.lambda, pending_state_.mu);
            }
        }
        check(fmhip_mcmc_epoch(h_, &last_stats));
        fm.download();
        if (burn_in > 0 && last_stats.iterations == burn_in) check(fmhip_mcmc_reset_average(h_));
        return fm;
    }
    State state() {
        State st;
        st.lambda.resize(state_size());
        st.mu.resize(state_size());
        check((grouped_ ? fmhip_mcmc_get_group_state : fmhip_mcmc_get_state)(need(), &st.alpha, st.lambda.data(), st.mu.data(), &st.iterations));
        return st;
    }
    std::vector<int64_t> groupCounts() {            // m_a: the trained features of attribute group a (one entry without groups)
        std::vector<int64_t> counts((size_t)n_groups_);
        check(fmhip_mcmc_group_info(need(), nullptr, counts.data()));
        return counts;
    }
    // before the first learn the state is kept and set when the handle is made (lambda, mu: k + 1 values each)
    void setState(double alpha, const std::vector<double> &lambda, const std::vector<double> &mu) {
        if (!h_) {
            pending_state_.alpha = alpha;
            pending_state_.lambda = lambda;
            pending_state_.mu = mu;
            pending_ = true;
            return;
        }
        if (lambda.size() != state_size() || mu.size() != state_size())
            throw Error(FMHIP_ERR_INVALID, "lambda and mu must hold k + 1 values each ((k + 1) * G with attribute groups)");
        check((grouped_ ? fmhip_mcmc_set_group_state : fmhip_mcmc_set_state)(h_, alpha, lambda.data(), mu.data()));
    }
    void resetAverage() { check(fmhip_mcmc_reset_average(need())); }
    std::vector<double> predictions() {             // the test rows' predictions averaged over the kept draws
        std::vector<double> mean(test_rows());
        check(fmhip_mcmc_predictions(need(), mean.data(), nullptr, nullptr));
        return mean;
    }
    std::vector<double> lastPredictions() {         // ... under the last draw
        std::vector<double> last(test_rows());
        check(fmhip_mcmc_predictions(need(), nullptr, last.data(), nullptr));
        return last;
    }
    int64_t draws() {
        int64_t n = 0;
        check(fmhip_mcmc_predictions(need(), nullptr, nullptr, &n));
        return n;
    }
    std::vector<double> latentTargets() {           // the targets the last epoch trained on (regression, or no epoch yet: the labels)
        std::vector<double> out((size_t)(h_ ? n_train_ : 0));
        check(fmhip_mcmc_latent_targets(need(), out.data()));
        return out;
    }
    double computeLogLoss() {                       // of the averaged probabilities against the test classes [y > 0]
        const std::vector<double> p = probabilities("computeLogLoss");
        double sum = 0.0;
        for (size_t r = 0; r < p.size(); ++r) {
            const double q = std::min(std::max(p[r], 1e-15), 1.0 - 1e-15);
            sum -= test_labels()[r] > 0 ? std::log(q) : std::log1p(-q);
        }
        return p.empty() ? 0.0 : sum / (double)p.size();
    }
    double computeAccuracy() {                      // the share of test rows whose averaged probability is on the label's side of 1/2
        const std::vector<double> p = probabilities("computeAccuracy");
        size_t hits = 0;
        for (size_t r = 0; r < p.size(); ++r) hits += (p[r] > 0.5) == (test_labels()[r] > 0);
        return p.empty() ? 0.0 : (double)hits / (double)p.size();
    }
    double computeRMSE() {                          // of the averaged prediction against the test labels (regression)
        need();
        if (classification_)
            throw Error(FMHIP_ERR_INVALID, "a classification run's predictions are probabilities: score them with computeLogLoss or computeAccuracy");
        const std::vector<double> mean = predictions();
        double sse = 0.0;
        for (size_t r = 0; r < mean.size(); ++r) sse += (mean[r] - test_labels()[r]) * (mean[r] - test_labels()[r]);
        return mean.empty() ? 0.0 : std::sqrt(sse / (double)mean.size());
    }
    void close() {
        check(fmhip_mcmc_destroy(h_));
        h_ = nullptr;
        d_ = nullptr;                               // (the next learn makes a handle for whatever it is given, flat or relational)
        r_ = nullptr;
    }

  private:
    fmhip_mcmc_t need() const {
        if (!h_) throw Error(FMHIP_ERR_INVALID, "HipMCMC has no handle yet: it is made by the first learn(fm, dataset)");
        return h_;
    }
    size_t test_rows() const {
        if (!test_ && !rel_test_) throw Error(FMHIP_ERR_INVALID, "HipMCMC was made without a test set");
        return (size_t)(rel_test_ ? rel_test_->size() : test_->size());
    }
    const std::vector<double> &test_labels() const { return rel_test_ ? rel_test_->labels() : test_->labels(); }
    std::vector<double> probabilities(const char *what) {
        need();
        if (!classification_) throw Error(FMHIP_ERR_INVALID, std::string(what) + " scores a classification run's probabilities (see computeRMSE)");
        return predictions();
    }
    size_t state_size() const { return ((size_t)k_ + 1) * (size_t)n_groups_; }
    DataSet *test_;
    RelationalData *rel_test_ = nullptr;
    bool part_groups_ = false;
    fmhip_relational_t r_ = nullptr;
    std::vector<int32_t> groups_;
    int32_t n_groups_ = 1;
    bool grouped_ = false;
    fmhip_mcmc_t h_ = nullptr;
    fmhip_model_t m_ = nullptr;
    fmhip_dataset_t d_ = nullptr;
    int32_t k_ = 0;
    int64_t n_train_ = 0;
    bool classification_ = false;
    bool pending_ = false;
    State pending_state_;
};

// BPR on implicit feedback (include/fmhip_bpr.h): the contexts (users) once, the candidates (items) once — both one-batch DataSets
// with disjoint feature ids, BORROWED — and per context the candidate rows it interacted with.  The negatives are drawn on the
// device afresh for every epoch and the step is the relational one: no joined row is ever built.  n_pairs = n_neg * interactions;
// the training order is context-ascending, rows ascending and distinct inside a context (the Python mirror's shuffle=False).
// One learn = one epoch (fmhip_bpr_epoch): resample at t = the epochs done, then every batch of batch_pairs pairs.  loss:
// FMHIP_LOSS_LOGISTIC is BPR, FMHIP_LOSS_SQUARED the squared pair loss; the model's pairing flag is neither read nor set.
// n_candidates (1 .. 64; include/fmhip_bpr_adaptive.h): above 1 every epoch draws that many candidates per pair and trains on the
// one the model scores highest at the epoch's start (once per epoch: later batches see slightly stale choices); 1: uniform.
// sampler: kAuto is that; kWarp (include/fmhip_warp.h) keeps per pair the first of the n_candidates candidates that violates
// `margin` (>= 0) against the positive and trains a hinge weighted by the rank estimated from the trials — `loss` is then not set.
// negatives (include/fmhip_proposal.h): kUniform, or kPopularity — candidate row i drawn in proportion to (n_i + smooth)^power, n_i
// the contexts that list row i; setProposal takes any M weights.
// loss = HipBPR::kSoftmax (include/fmhip_softmax.h): the n_neg negatives of an interaction compete in one sampled-softmax loss; the
// trainer's own rule — the model's loss is not set; not with kWarp; batch_pairs a multiple of n_neg.  logq: the proposal's
// log-probabilities are subtracted from the logits (ignored under kUniform).
class HipBPR : public FMLearn {
  public:
    enum Sampler { kAuto = 0, kWarp = 1 };
    enum Negatives { kUniform = 0, kPopularity = 1 };
    enum { kSoftmax = -1 };      // a value of `loss` beside FMHIP_LOSS_SQUARED / FMHIP_LOSS_LOGISTIC, handled here: never passed to the model
    enum Redraw { kEpoch = FMHIP_REDRAW_EPOCH, kBatch = FMHIP_REDRAW_BATCH };      // include/fmhip_redraw.h
    double eta, reg0, regw, regv;
    int loss, optimizer;
    double adagrad_eps, adagrad_init;
    fmhip_stats last_stats{};
    fmhip_bpr_sample_stats sample_stats{};
    fmhip_bpr_adaptive_stats adaptive_stats{};
    fmhip_warp_stats warp_stats{};
    fmhip_redraw_stats redraw_stats{};      // kBatch: the sampler's counters summed over the last epoch's batches; step(fm, batch, t): that draw's
    HipBPR(DataSet &contexts, DataSet &candidates, const std::vector<std::vector<int32_t>> &positives, int32_t n_neg = 1, int64_t batch_pairs = 0,
           uint64_t seed = 0, double eta_ = 0.05, double reg0_ = 0.0, double regw_ = 0.0, double regv_ = 0.0, int loss_ = FMHIP_LOSS_LOGISTIC,
           int optimizer_ = FMHIP_OPT_SGD, double adagrad_eps_ = 1e-10, double adagrad_init_ = 0.1, int32_t n_candidates = 1,
           int sampler = kAuto, double margin = 1.0, int redraw = kEpoch, int negatives = kUniform, double power = 0.75, double smooth = 1.0,
           bool logq = false)
        : eta(eta_), reg0(reg0_), regw(regw_), regv(regv_), loss(loss_), optimizer(optimizer_), adagrad_eps(adagrad_eps_), adagrad_init(adagrad_init_),
          contexts_(contexts), candidates_(candidates), n_neg_(n_neg), batch_pairs_(batch_pairs), seed_(seed), n_candidates_(n_candidates),
          sampler_(sampler), margin_(margin), redraw_(redraw), logq_(logq) {
        if (sampler != kAuto && sampler != kWarp) throw Error(FMHIP_ERR_INVALID, "sampler must be HipBPR::kAuto or HipBPR::kWarp");
        if (redraw != kEpoch && redraw != kBatch) throw Error(FMHIP_ERR_INVALID, "redraw must be HipBPR::kEpoch or HipBPR::kBatch");
        if (!(margin >= 0.0) || !(margin <= 3.4028234663852886e38)) throw Error(FMHIP_ERR_INVALID, "margin must be a finite number >= 0");
        if (sampler == kWarp && loss_ == kSoftmax) throw Error(FMHIP_ERR_INVALID, "sampler = kWarp and loss = kSoftmax each train their own rule: choose one");
        if (sampler == kWarp && loss_ != FMHIP_LOSS_LOGISTIC) throw Error(FMHIP_ERR_INVALID, "sampler = kWarp trains its own hinge: leave loss at its default");
        if (n_candidates < 1 || n_candidates > FMHIP_BPR_MAX_CANDIDATES) throw Error(FMHIP_ERR_INVALID, "n_candidates must be in [1, 64]");
        if ((int64_t)positives.size() != contexts.size()) throw Error(FMHIP_ERR_INVALID, "positives must hold one list per context");
        for (size_t u = 0; u < positives.size(); ++u) {
            std::vector<int32_t> rows = positives[u];
            std::sort(rows.begin(), rows.end());
            rows.erase(std::unique(rows.begin(), rows.end()), rows.end());
            for (int32_t c : rows) {
                inter_ctx_.push_back((int32_t)u);
                inter_cand_.push_back(c);
            }
        }
        if (softmax() && batch_pairs > 0 && batch_pairs < n_pairs() && batch_pairs % n_neg != 0)
            throw Error(FMHIP_ERR_INVALID, "loss = kSoftmax: batch_pairs = " + std::to_string(batch_pairs) + " is no multiple of n_neg = " +
                                               std::to_string(n_neg) + " — a batch would split an interaction's negatives");
        if (negatives != kUniform && negatives != kPopularity) throw Error(FMHIP_ERR_INVALID, "negatives must be HipBPR::kUniform or HipBPR::kPopularity");
        if (negatives == kPopularity) {
            if (!(smooth > 0.0) || !std::isfinite(smooth) || !std::isfinite(power)) throw Error(FMHIP_ERR_INVALID, "smooth must be > 0, power finite");
            std::vector<double> n((size_t)candidates.size(), 0.0);
            for (int32_t c : inter_cand_)
                if (c >= 0 && (size_t)c < n.size()) n[(size_t)c] += 1.0;
            for (double &x : n) x = std::pow(x + smooth, power);
            proposal_ = n;
        }
    }
    HipBPR(const HipBPR &) = delete;
    HipBPR &operator=(const HipBPR &) = delete;
    ~HipBPR() { (void)fmhip_bpr_destroy(h_); }

    int64_t dimension() override { return std::max(contexts_.dimension(), candidates_.dimension()); }
    int64_t n_pairs() const { return (int64_t)inter_ctx_.size() * n_neg_; }
    int32_t n_candidates() const { return n_candidates_; }
    bool warp() const { return sampler_ == kWarp; }
    bool softmax() const { return loss == kSoftmax; }
    bool ownRule() const { return warp() || softmax(); }      // the step's rule is the trainer's: the model's loss is left as it is
    double margin() const { return margin_; }
    int redraw() const { return redraw_; }
    const std::vector<double> &proposal() const { return proposal_; }      // empty: uniform
    // the proposal from the next draw on (fmhip_proposal_set): one weight per candidate row, or an empty vector for uniform
    void setProposal(const std::vector<double> &weights) {
        if (!weights.empty() && (int64_t)weights.size() != candidates_.size()) throw Error(FMHIP_ERR_INVALID, "the proposal takes one weight per candidate row");
        for (double w : weights)
            if (!(w > 0.0) || !std::isfinite(w)) throw Error(FMHIP_ERR_INVALID, "a proposal weight is finite and > 0");
        if (h_) check(fmhip_proposal_set(h_, weights.empty() ? nullptr : weights.data()));
        proposal_ = weights;
    }
    // the handle borrows the blocks' device copies: made again when either was unpersisted since (FM's fit loop unpersists its dataset)
    fmhip_bpr_t handle() {
        const fmhip_dataset_t c = contexts_.handle(), i = candidates_.handle();
        if (h_ && (c != for_ctx_ || i != for_cand_)) close();
        if (!h_) {
            check(fmhip_bpr_create(contexts_.device(), c, i, (int64_t)inter_ctx_.size(), inter_ctx_.data(), inter_cand_.data(), n_neg_, batch_pairs_,
                                   seed_, &h_));
            if (n_candidates_ > 1) check(fmhip_bpr_set_candidates(h_, n_candidates_));
            if (warp()) check(fmhip_warp_set(h_, 1, margin_));
            if (redraw_ != kEpoch) check(fmhip_redraw_set(h_, redraw_));
            if (!proposal_.empty()) check(fmhip_proposal_set(h_, proposal_.data()));
            if (softmax()) check(fmhip_softmax_set(h_, 1, logq_ ? 1 : 0));
            for_ctx_ = c;
            for_cand_ = i;
        }
        return h_;
    }
    void close() {
        check(fmhip_bpr_destroy(h_));
        h_ = nullptr;
    }
    FMModel &learn(FMModel &fm) {
        const fmhip_bpr_t h = handle();
        if (!ownRule()) check(fmhip_model_set_loss(fm.upload(), loss));
        check(fmhip_model_set_optimizer(fm.upload(), optimizer, adagrad_eps, adagrad_init));
        check(fmhip_bpr_epoch(fm.upload(), h, epoch_, eta, reg0, regw, regv, nullptr, &last_stats));
        if (redraw_ == kBatch) check(fmhip_redraw_epoch_stats(h, &redraw_stats));
        ++epoch_;
        fm.download();
        return fm;
    }
    // one mini-batch step whose pairs are first redrawn at epoch t under the model as it stands (fmhip_redraw_step; either mode)
    const fmhip_stats &step(FMModel &fm, int64_t batch, int64_t t) {
        const fmhip_bpr_t h = handle();
        if (!ownRule()) check(fmhip_model_set_loss(fm.upload(), loss));
        check(fmhip_model_set_optimizer(fm.upload(), optimizer, adagrad_eps, adagrad_init));
        check(fmhip_redraw_step(fm.upload(), h, t, batch, eta, reg0, regw, regv, &last_stats, &redraw_stats));
        fm.download();
        return last_stats;
    }
    FMModel &learn(FMModel &fm, DataSet &) override { return learn(fm); }       // (the fit loop's dataset is not read)
    using FMLearn::learn;
    FMModel fit(int32_t numFactor, int epochs, uint64_t seed = 0) {
        FMModel fm(dimension(), numFactor, 0.0, 0.01, seed, contexts_.device());
        for (int i = 0; i < epochs; ++i) learn(fm);
        return fm;
    }
    const fmhip_bpr_sample_stats &resample(int64_t t) {
        if (warp()) throw Error(FMHIP_ERR_INVALID, "sampler = kWarp: the WARP draw needs a model — resampleWarp(t, fm)");
        if (n_candidates_ > 1) throw Error(FMHIP_ERR_INVALID, "n_candidates > 1: the adaptive draw needs a model — resample(t, fm)");
        check(fmhip_bpr_resample(handle(), t, &sample_stats));
        return sample_stats;
    }
    // the best of n_candidates candidates under the model as it stands (fmhip_bpr_resample_adaptive)
    const fmhip_bpr_adaptive_stats &resample(int64_t t, FMModel &fm) {
        if (warp()) throw Error(FMHIP_ERR_INVALID, "sampler = kWarp: the draw is resampleWarp(t, fm)");
        const fmhip_bpr_t h = handle();
        check(fmhip_bpr_resample_adaptive(fm.upload(), h, t, &adaptive_stats));
        return adaptive_stats;
    }
    // the WARP draw under the model as it stands (fmhip_warp_resample), and what it left per pair
    const fmhip_warp_stats &resampleWarp(int64_t t, FMModel &fm) {
        const fmhip_bpr_t h = handle();
        check(fmhip_warp_resample(fm.upload(), h, t, &warp_stats));
        return warp_stats;
    }
    std::vector<float> pairWeights() {
        std::vector<float> out((size_t)n_pairs());
        check(fmhip_warp_weights(handle(), out.data()));
        return out;
    }
    std::vector<int32_t> trials() {
        std::vector<int32_t> out((size_t)n_pairs());
        check(fmhip_warp_trials(handle(), out.data()));
        return out;
    }
    std::vector<int32_t> negatives() {
        std::vector<int32_t> out((size_t)n_pairs());
        check(fmhip_bpr_negatives(handle(), out.data()));
        return out;
    }
    // the sampled softmax (include/fmhip_softmax.h): the pairs' probabilities of each batch's last step, the log-Q table (empty
    // unless the correction is in force), the mean loss and the share of interactions whose positive is on top
    std::vector<float> softmaxProbs() {
        std::vector<float> out((size_t)n_pairs());
        check(fmhip_softmax_probs(handle(), out.data()));
        return out;
    }
    std::vector<float> logq() {
        if (!softmax() || !logq_ || proposal_.empty()) return {};
        std::vector<float> out((size_t)candidates_.size());
        check(fmhip_softmax_logq(handle(), out.data()));
        return out;
    }
    double computeSoftmaxLoss(FMModel &fm) {
        double loss_ = 0.0;
        check(fmhip_softmax_loss(fm.upload(), handle(), &loss_, nullptr, nullptr));
        return loss_;
    }
    double computeTop1(FMModel &fm) {
        double top = 0.0;
        check(fmhip_softmax_loss(fm.upload(), handle(), nullptr, &top, nullptr));
        return top;
    }
    double computePairLogLoss(FMModel &fm) {
        double ll = 0.0;
        check(fmhip_bpr_pair_logloss(fm.upload(), handle(), &ll, nullptr, nullptr));
        return ll;
    }
    double computePairAccuracy(FMModel &fm) {
        double ll = 0.0, conc = 0.0;
        check(fmhip_bpr_pair_logloss(fm.upload(), handle(), &ll, &conc, nullptr));
        return conc;
    }

  private:
    DataSet &contexts_, &candidates_;
    std::vector<int32_t> inter_ctx_, inter_cand_;
    int32_t n_neg_;
    int64_t batch_pairs_;
    uint64_t seed_;
    int32_t n_candidates_;
    int sampler_;
    double margin_;
    int redraw_;
    bool logq_;
    std::vector<double> proposal_;
    int64_t epoch_ = 0;
    fmhip_bpr_t h_ = nullptr;
    fmhip_dataset_t for_ctx_ = nullptr, for_cand_ = nullptr;
};

// FM(dataset, numFactor, maxIteration).learnWith(learner) — S/fm/FM.scala:25-33 and the fit loop of
// S/fm/impl/FactorizationMachines.scala:30-51: cache; new FMModel(dimension, numFactor); maxIteration x { computeRMSE (logged);
// fm = fml.learn(fm, dataset) }; unpersist
class FM {
  public:
    std::vector<double> rmse_history;
    FM(DataSet &dataset, int32_t numFactor, int maxIteration = 100, uint64_t seed = 0) : dataset_(dataset), numFactor_(numFactor), maxIteration_(maxIteration), seed_(seed) {}
    // S/fm/impl/FactorizationMachines.scala:24-28: appends and returns *this.  With relations learnWith fits
    // RelationalData(labels, relations, plain = the dataset if it has nonzeros), batched as the dataset
    FM &withRelation(Relation &relation) {
        relations_.push_back(&relation);
        return *this;
    }
    FM &withRelation(const std::vector<Relation *> &relations) {
        relations_.insert(relations_.end(), relations.begin(), relations.end());
        return *this;
    }
    // init (optional): called on the fresh model before the first iteration — parity runs inject w0 / w / v here (quirk Q2)
    // With relations the fit ends as the flat one does (:48): the relational handle and the dataset (the plain part) leave the
    // device; the BLOCKS stay cached with their Relation, which other fits and held-out data may share (relation.block().unpersist())
    template <class Init>
    FMModel learnWith(FMLearn &fml, Init init) {
        if (relations_.empty()) return fit(dataset_, fml, init);
        RelationalData rd(dataset_.labels(), relations_, dataset_.nnz() ? &dataset_ : nullptr, dataset_.batch_rows(), dataset_.device());
        FMModel fm = fit(rd, fml, init);       // (its unpersist freed the handle that borrowed the dataset)
        dataset_.unpersist();
        return fm;
    }
    FMModel learnWith(FMLearn &fml) {
        return learnWith(fml, [](FMModel &) {});
    }

  private:
    template <class Data, class Init>
    FMModel fit(Data &data, FMLearn &fml, Init init) {
        Data &ds = data.cache();                                                 // :36
        FMModel fm(std::max<int64_t>(ds.dimension(), fml.dimension()), numFactor_, 0.0, 0.01, seed_, ds.device());   // :39 (+ the learner's own width)
        init(fm);
        for (int i = 1; i <= maxIteration_; ++i) {                               // :42
            rmse_history.push_back(fm.computeRMSE(ds));                          // :43 (logged and discarded in the reference)
            fml.learn(fm, ds);                                                   // :45
        }
        ds.unpersist();                                                          // :48
        return fm;
    }
    DataSet &dataset_;
    std::vector<Relation *> relations_;
    int32_t numFactor_;
    int maxIteration_;
    uint64_t seed_;
};

}  // namespace sparkfm
#endif  // SPARKFM_HPP
