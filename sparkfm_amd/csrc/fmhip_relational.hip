// fmhip_relational.hip — relational data (include/fmhip_relational.h): the handle (create / destroy / info) and the relational
// mini-batch step, a sibling of fmhip_step.hip:
//     fold_scales -> kFwdQ forward of every block (whole) -> kFwdQ forward of the plain part's batch -> k_rel_finish
//     -> per relation: k_rel_gather_sum, then the existing backward + fixups over the block's CSC with (P_b, e_b) for (P, e)
//     -> the plain part's backward with P as it is -> the step's statistics (launch_reduce_blocks) -> the dense launch_apply
// The BPR trainer (fmhip_bpr.hip) runs the same step in its pairs mode: the finish leaves Q_r and yhat_r, launch_pair_finish forms e.
// The scoring calls are in fmhip_score.hip (they work in a ScorePass); the kernels in fm_relational.hip; the host arithmetic
// (mapping check, disjointness of the parts' features, the inverse map's counting sort) in fmhip_host.cpp.
#include "fmhip_internal.h"

#include <algorithm>
#include <cstdio>
#include <memory>
#include <new>
#include <vector>

using namespace fmhip;
using namespace fmhip::host;

static_assert(kRelMax == FMHIP_RELATIONS_MAX && kRelSumCut == FMHIP_RELATIONAL_SUM_CUT, "fm_relational.h and the public header agree");

namespace {

template <typename T>
int upload(DevBuf<T> &dst, const std::vector<T> &src) {
    TRY(dst.alloc(std::max<size_t>(src.size(), 1)));
    if (!src.empty()) HIP_TRY(hipMemcpy(dst.p, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    return FMHIP_OK;
}

const char *part_name(int p, int m, char (&buf)[32]) {
    if (p < m) snprintf(buf, sizeof buf, "relation %d", p);
    else snprintf(buf, sizeof buf, "the plain part");
    return buf;
}

int check_rel_batch(fmhip_relational_t R, int64_t batch) {
    if (batch < 0 || batch >= (int64_t)R->batches.size())
        return fail(FMHIP_ERR_INVALID, "batch %lld out of range [0, %zu)", (long long)batch, R->batches.size());
    return FMHIP_OK;
}

int ensure_rel_workspace(fmhip_model_t m, fmhip_relational_t R) {
    const size_t rows = (size_t)std::max<int64_t>(R->max_rows, 1);
    TRY(m->P.ensure(rows * m->Kp));
    TRY(m->e.ensure(rows));
    TRY(m->yhat.ensure(std::max<size_t>(rows, 2)));
    TRY(m->bsum.ensure((size_t)kMaxFwdBlocks * 4));
    for (auto &rel : R->rels) {
        const size_t J = (size_t)rel->block->n_rows;
        TRY(rel->Q.ensure(J * m->Kp));
        TRY(rel->Pb.ensure(J * m->Kp));
        TRY(rel->yq.ensure(J));
        TRY(rel->eb.ensure(J));
        TRY(rel->part.ensure((size_t)std::max<int32_t>(rel->max_part, 1) * m->Kp));
        TRY(rel->part_e.ensure((size_t)std::max<int32_t>(rel->max_part, 1)));
        TRY(ensure_backward_workspace(m, rel->block));
    }
    if (R->plain) TRY(ensure_backward_workspace(m, R->plain));
    return FMHIP_OK;
}

}  // namespace

namespace fmhip {
namespace host {

// a part's features: the columns of its batches' transposes and the dense hot block's ids
void part_features(fmhip_dataset_t d, std::vector<int32_t> &out) {
    out = d->h_cfeat;
    for (int32_t id : d->hot_ids)
        if (id >= 0) out.push_back(id);
}

int check_rel_model(fmhip_model_t m, fmhip_relational_t R) {
    if (!m || !R) return fail(FMHIP_ERR_INVALID, "model or relational dataset is NULL");
    if (m->device != R->device) return fail(FMHIP_ERR_INVALID, "model on device %d, relational dataset on device %d", m->device, R->device);
    if (R->dimension > m->n)
        return fail(FMHIP_ERR_SHAPE, "relational dataset has feature index %lld but the model has num_attribute = %lld", (long long)R->dimension,
                    (long long)m->n);
    return set_device(m->device);
}

int rel_q_forwards(fmhip_model_t m, fmhip_relational_t R, const RelBufs &w, hipStream_t s) {
    for (size_t i = 0; i < R->rels.size(); ++i) {
        fmhip_dataset_t blk = R->rels[i]->block;
        const FwdArgs a = fwd_args_out(m, blk, blk->batches[0], w.Q[i], nullptr, nullptr, w.yq[i], kLossSquared);
        HIP_TRY(launch_forward(m->Kp, kFwdQ, a, s, nullptr));
    }
    return FMHIP_OK;
}

RelFinishArgs rel_finish_args(fmhip_model_t m, fmhip_relational_t R, const RelBufs &w, const fmhip_relational::Batch &B, int loss) {
    RelFinishArgs fa{};
    fa.m = (int32_t)R->rels.size();
    for (int i = 0; i < fa.m; ++i) {
        fa.Q[i] = w.Q[i];
        fa.yq[i] = w.yq[i];
        fa.map[i] = R->rels[(size_t)i]->map.p + B.row0;
    }
    fa.has_plain = R->plain ? 1 : 0;
    fa.w0 = m->w0.p;
    fa.P = w.P;
    fa.yplain = w.yhat;
    fa.y = R->y.p + B.row0;
    fa.e = w.e;
    fa.yhat = w.yhat;
    fa.bsum = w.bsum;
    fa.n_rows = (int32_t)B.rows;
    fa.pack_k = m->pack_k();
    fa.loss = loss;
    return fa;
}

// a step's buffers: the handle's Q / yq per relation (ensure_rel_workspace has sized them), the model's workspace
static RelBufs rel_step_bufs(fmhip_model_t m, fmhip_relational_t R) {
    RelBufs w{};
    for (size_t i = 0; i < R->rels.size(); ++i) {
        w.Q[i] = R->rels[i]->Q.p;
        w.yq[i] = R->rels[i]->yq.p;
    }
    w.P = m->P.p;
    w.e = m->e.p;
    w.yhat = m->yhat.p;
    w.bsum = m->bsum.p;
    return w;
}

// what a step begins with, on its own: the scales folded, the handle's workspace sized, then every block's kFwdQ forward into the
// relation's Q / yq on the model's stream (behind the last step that used the workspace)
int rel_block_forwards(fmhip_model_t m, fmhip_relational_t R) {
    TRY(fold_scales(m));                     // the dense update only: the tables are at scale 1 from here on
    TRY(ensure_rel_workspace(m, R));
    // the workspace is the handle's: behind the last step that used it, if that one was queued on another stream (another model)
    if (R->busy_set && R->busy_stream != m->stream) HIP_TRY(hipStreamWaitEvent(m->stream, R->busy, 0));
    return rel_q_forwards(m, R, rel_step_bufs(m, R), m->stream);
}

// one relational step of batch b, asynchronous on the model's stream; acc (nullable): the epoch's fp64 accumulators
int rel_step(fmhip_model_t m, fmhip_relational_t R, int64_t b, const Sgd &sgd, double *acc, bool pairs, const PairHinge *hinge,
             const RelStepQueued &queued) {
    const fmhip_relational::Batch &B = R->batches[(size_t)b];
    if (!queued.forwards) TRY(rel_block_forwards(m, R));      // every block's q-mode pass, over the whole block
    TRY(begin_forward(m));                   // (the forwards do not touch the gradient)
    int64_t nnz = R->block_nnz;
    if (R->plain) {
        const BatchMeta &bm = R->plain->batches[(size_t)b];
        const FwdArgs a = fwd_args_out(m, R->plain, bm, m->P.p, nullptr, nullptr, m->yhat.p, kLossSquared);
        HIP_TRY(launch_forward(m->Kp, kFwdQ, a, m->stream, nullptr));
        nnz += bm.nnz_total;
    }
    RelFinishArgs fa = rel_finish_args(m, R, rel_step_bufs(m, R), B, m->rule.loss);
    if (!pairs) fa.yhat = nullptr;           // (only the pairs' finish reads the rows' predictions)
    fa.q_only = pairs ? 1 : 0;
    HIP_TRY(launch_rel_finish(m->Kp, fa, false, m->stream, &m->step.fwd_parts));
    if (pairs) {
        // the BPR trainer: the finish left Q_r in P and yhat_r beside it, as the flat paired step's kFwdQ forward does; the pairs'
        // finish (fm_pairing.hip) turns them into P_r = Q_r e_r, e and the statistics partials (its own block count)
        PairArgs pa = pair_args(m, R->y.p + B.row0, nullptr, B.rows);
        if (hinge && hinge->softmax_n > 0) {  // the softmax step: the pre-pass over yhat, then the probabilities taken as given
            SoftmaxArgs sa{};
            sa.yhat = m->yhat.p;
            sa.map = R->rels[1]->map.p + B.row0;
            sa.lq = hinge->lq;
            sa.pi = hinge->pi + B.row0;
            sa.bsum = hinge->sm_bsum;
            sa.n = hinge->softmax_n;
            sa.n_inter = (int32_t)(B.rows / (2 * (int64_t)hinge->softmax_n));
            HIP_TRY(launch_softmax_pre(sa, m->stream, nullptr));
            pa.c = sa.pi;
            pa.loss = kPairLossGiven;
        } else if (hinge) {                  // the WARP step: the sampler's weights, the hinge in the model's loss's place
            pa.c = hinge->c + B.row0;
            pa.loss = kPairLossHinge;
            pa.margin = hinge->margin;
        }
        HIP_TRY(launch_pair_finish(m->Kp, pa, m->stream, &m->step.fwd_parts));
    }
    m->step.written(nnz, B.rows);            // (no backward window: the parts' whole-batch backwards below are the step's own)
    for (size_t ri = 0; ri < R->rels.size(); ++ri) {
        fmhip_relational::Relation &rel = *R->rels[ri];
        const RelationInverse::Batch &ib = rel.batches[(size_t)b];
        const size_t J = (size_t)rel.block->n_rows;
        HIP_TRY(hipMemsetAsync(rel.Pb.p, 0, J * m->Kp * sizeof(float), m->stream));      // block rows nobody references: exact zeros
        HIP_TRY(hipMemsetAsync(rel.eb.p, 0, J * sizeof(float), m->stream));
        RelGatherArgs ga{};
        ga.P = m->P.p;
        ga.e = m->e.p;
        ga.trow = rel.trow.p + ib.row_off;
        ga.tptr = rel.tptr.p + ib.tptr_off;
        ga.tj = rel.tj.p + ib.t_off;
        ga.wt = rel.wt.p + ib.w_off;
        ga.wbeg = rel.wbeg.p + ib.w_off;
        ga.wdst = rel.wdst.p + ib.w_off;
        ga.n_work = ib.n_work;
        ga.lt = rel.lt.p + ib.l_off;
        ga.lfirst = rel.lfirst.p + ib.l_off;
        ga.lcount = rel.lcount.p + ib.l_off;
        ga.n_long = ib.n_long;
        ga.Pb = rel.Pb.p;
        ga.eb = rel.eb.p;
        ga.part = rel.part.p;
        ga.part_e = rel.part_e.p;
        ga.pack_k = m->pack_k();
        if (queued.dev_counts && queued.dev_counts[ri]) {      // the counts where the inverse build left them: no host copy read
            ga.counts = queued.dev_counts[ri];
            ga.n_work = ga.n_long = 0;
            ga.cap_work = (int32_t)B.rows;
            ga.cap_long = (int32_t)rel_long_cap(B.rows);
            ga.cap_part = 2 * ga.cap_long;
        }
        HIP_TRY(launch_rel_gather_sum(m->Kp, ga, m->stream));
        const BwdSource src{rel.Pb.p, rel.eb.p};
        m->step.arm_hot(rel.block->hot_T > 0);
        TRY(step_backward(m, rel.block, 0, 0, INT64_MAX, false, nullptr, nullptr, kOwnLower, &src));
    }
    if (R->plain) {                          // the plain part: P as the finish left it (the paired path's second half)
        m->step.arm_hot(R->plain->hot_T > 0);
        TRY(step_backward(m, R->plain, b, 0, INT64_MAX, false, nullptr));
    }
    m->step.arm_hot(false);
    HIP_TRY(launch_reduce_blocks(m->bsum.p, m->step.fwd_parts, (int32_t)B.rows, m->scal(), acc, m->stream));
    TRY(step_apply(m, sgd));                 // the dense update (SGD or AdaGrad), which also closes the step
    HIP_TRY(hipEventRecord(R->busy, m->stream));
    R->busy_stream = m->stream;
    R->busy_set = true;
    return FMHIP_OK;
}

}  // namespace host
}  // namespace fmhip

namespace {

int check_train_rel(fmhip_model_t m, fmhip_relational_t R) {
    TRY(check_rel_model(m, R));
    if (const char *why = refusal(Path::kRelational, m->rule)) return fail(FMHIP_ERR_UNSUPPORTED, "%s", why);
    return FMHIP_OK;
}

}  // namespace

extern "C" {

int fmhip_relational_create(int device, int64_t n_rows, const double *y, int32_t n_relations, const fmhip_dataset_t *blocks,
                            const int32_t *const *mappings, fmhip_dataset_t plain, int64_t batch_rows, fmhip_relational_t *out) {
    if (!out) return fail(FMHIP_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (n_rows < 1) return fail(FMHIP_ERR_INVALID, "n_rows = %lld: a relational dataset needs at least one row", (long long)n_rows);
    if (!y) return fail(FMHIP_ERR_INVALID, "y is NULL");
    if (n_relations < 1 || n_relations > FMHIP_RELATIONS_MAX)
        return fail(FMHIP_ERR_INVALID, "n_relations = %d: a relational dataset has 1 .. %d relations", (int)n_relations, FMHIP_RELATIONS_MAX);
    if (!blocks || !mappings) return fail(FMHIP_ERR_INVALID, "blocks or mappings is NULL");
    // ---- the host checks (no HIP call before they have passed)
    int64_t dim = 0;
    for (int i = 0; i < n_relations; ++i) {
        fmhip_dataset_t d = blocks[i];
        if (!d) return fail(FMHIP_ERR_INVALID, "relation %d: the block is NULL", i);
        if (!mappings[i]) return fail(FMHIP_ERR_INVALID, "relation %d: the mapping is NULL", i);
        if (d->device != device) return fail(FMHIP_ERR_INVALID, "relation %d: the block is on device %d, not %d", i, d->device, device);
        if (d->scoring_only)
            return fail(FMHIP_ERR_UNSUPPORTED, "relation %d: the block was created with fmhip_rows_create (scoring only): it has no transposes to train on", i);
        if (d->batches.size() != 1)
            return fail(FMHIP_ERR_INVALID, "relation %d: the block has %zu batches — create it with batch_rows = 0 (one batch of all its %lld rows)", i,
                        d->batches.size(), (long long)d->n_rows);
        if (d->weighted) return fail(FMHIP_ERR_UNSUPPORTED, "relation %d: %s", i, refusal(Path::kRelational, TrainRule{}, true));
        const int64_t bad = relational_bad_mapping(n_rows, mappings[i], d->n_rows);
        if (bad >= 0)
            return fail(FMHIP_ERR_INVALID, "relation %d: mapping[%lld] = %d lies outside the block's rows [0, %lld)", i, (long long)bad,
                        (int)mappings[i][bad], (long long)d->n_rows);
        dim = std::max(dim, d->dimension);
    }
    if (batch_rows <= 0 || batch_rows > n_rows) batch_rows = n_rows;
    const int64_t nb = (n_rows + batch_rows - 1) / batch_rows;
    if (plain) {
        if (plain->device != device) return fail(FMHIP_ERR_INVALID, "the plain part is on device %d, not %d", plain->device, device);
        if (plain->scoring_only)
            return fail(FMHIP_ERR_UNSUPPORTED, "the plain part was created with fmhip_rows_create (scoring only): it has no transposes to train on");
        if (plain->weighted) return fail(FMHIP_ERR_UNSUPPORTED, "the plain part: %s", refusal(Path::kRelational, TrainRule{}, true));
        if (plain->n_rows != n_rows)
            return fail(FMHIP_ERR_INVALID, "the plain part has %lld rows, the relational dataset %lld", (long long)plain->n_rows, (long long)n_rows);
        if (plain->batch_rows != batch_rows || (int64_t)plain->batches.size() != nb)
            return fail(FMHIP_ERR_INVALID, "the plain part is batched by %lld rows (%zu batches), the relational dataset by %lld (%lld batches)",
                        (long long)plain->batch_rows, plain->batches.size(), (long long)batch_rows, (long long)nb);
        dim = std::max(dim, plain->dimension);
    }
    {
        const int n_parts = n_relations + (plain ? 1 : 0);
        std::vector<std::vector<int32_t>> feats((size_t)n_parts);
        std::vector<const int32_t *> fp((size_t)n_parts);
        std::vector<int64_t> fn((size_t)n_parts);
        for (int p = 0; p < n_parts; ++p) {
            part_features(p < n_relations ? blocks[p] : plain, feats[(size_t)p]);
            fp[(size_t)p] = feats[(size_t)p].data();
            fn[(size_t)p] = (int64_t)feats[(size_t)p].size();
        }
        const SharedFeature sh = first_shared_feature(n_parts, fp.data(), fn.data(), dim);
        if (sh.feature >= 0) {
            char na[32], nb_[32];
            return fail(FMHIP_ERR_INVALID, "feature %d occurs in %s and in %s: the parts' feature sets must be disjoint (every part's backward "
                                           "stores its gradient rows)", (int)sh.feature, part_name(sh.a, n_relations, na), part_name(sh.b, n_relations, nb_));
        }
    }
    // ---- the handle
    TRY(set_device(device));
    std::unique_ptr<fmhip_relational> R(new (std::nothrow) fmhip_relational());
    if (!R) return fail(FMHIP_ERR_NOMEM, "out of host memory");
    R->device = device;
    R->n_rows = n_rows;
    R->batch_rows = batch_rows;
    R->dimension = dim;
    R->plain = plain;
    HIP_TRY(hipEventCreateWithFlags(&R->busy, hipEventDisableTiming));
    for (int64_t b = 0; b < nb; ++b) {
        fmhip_relational::Batch B;
        B.row0 = b * batch_rows;
        B.rows = std::min(batch_rows, n_rows - B.row0);
        R->max_rows = std::max(R->max_rows, B.rows);
        R->batches.push_back(B);
    }
    if (plain)
        for (int64_t b = 0; b < nb; ++b)
            if (plain->batches[(size_t)b].row0 != R->batches[(size_t)b].row0 || plain->batches[(size_t)b].rows != R->batches[(size_t)b].rows)
                return fail(FMHIP_ERR_INVALID, "the plain part's batch %lld covers other rows than the relational dataset's", (long long)b);
    {
        std::vector<float> yf((size_t)n_rows);
        for (int64_t r = 0; r < n_rows; ++r) yf[(size_t)r] = (float)y[r];
        TRY(upload(R->y, yf));
        TRY(R->y64.alloc((size_t)n_rows));
        HIP_TRY(hipMemcpy(R->y64.p, y, (size_t)n_rows * sizeof(double), hipMemcpyHostToDevice));
    }
    std::vector<int32_t> count;
    for (int i = 0; i < n_relations; ++i) {
        std::unique_ptr<fmhip_relational::Relation> rel(new (std::nothrow) fmhip_relational::Relation());
        if (!rel) return fail(FMHIP_ERR_NOMEM, "out of host memory");
        rel->block = blocks[i];
        R->block_nnz += blocks[i]->nnz;
        RelationInverse inv;
        count.clear();
        for (const auto &B : R->batches) inv.append_batch(mappings[i] + B.row0, B.rows, blocks[i]->n_rows, kRelSumCut, count);
        rel->batches = inv.batches;
        rel->max_part = inv.max_part;
        TRY(rel->map.alloc((size_t)n_rows));
        HIP_TRY(hipMemcpy(rel->map.p, mappings[i], (size_t)n_rows * sizeof(int32_t), hipMemcpyHostToDevice));
        TRY(upload(rel->trow, inv.trow)); TRY(upload(rel->tj, inv.tj)); TRY(upload(rel->tptr, inv.tptr));
        TRY(upload(rel->wt, inv.wt)); TRY(upload(rel->wbeg, inv.wbeg)); TRY(upload(rel->wdst, inv.wdst));
        TRY(upload(rel->lt, inv.lt)); TRY(upload(rel->lfirst, inv.lfirst)); TRY(upload(rel->lcount, inv.lcount));
        R->rels.push_back(std::move(rel));
    }
    *out = R.release();
    return FMHIP_OK;
}

int fmhip_relational_destroy(fmhip_relational_t r) {
    if (!r) return FMHIP_OK;
    (void)hipSetDevice(r->device);
    std::unique_ptr<fmhip_relational>(r).reset();
    return FMHIP_OK;
}

int fmhip_relational_info(fmhip_relational_t r, int64_t *n_rows, int64_t *dimension, int64_t *batch_rows, int64_t *n_batches,
                          int32_t *n_relations) {
    if (!r) return fail(FMHIP_ERR_INVALID, "relational dataset is NULL");
    if (n_rows) *n_rows = r->n_rows;
    if (dimension) *dimension = r->dimension;
    if (batch_rows) *batch_rows = r->batch_rows;
    if (n_batches) *n_batches = (int64_t)r->batches.size();
    if (n_relations) *n_relations = (int32_t)r->rels.size();
    return FMHIP_OK;
}

int fmhip_relational_sgd_step(fmhip_model_t m, fmhip_relational_t r, int64_t batch, double eta, double reg0, double regw, double regv,
                              fmhip_stats *stats) {
    WriteLock lock(m);
    TRY(check_train_rel(m, r));
    TRY(check_rel_batch(r, batch));
    TRY(rel_step(m, r, batch, Sgd{eta, reg0, regw, regv}, nullptr));
    if (stats) {
        // (the update zeroes the gradient rows it applies, not the head's statistics)
        memset(stats, 0, sizeof *stats);
        TRY(read_scal(m, stats));
        stats->nnz = m->step.last_nnz;
        stats->steps = 1;
    }
    return FMHIP_OK;
}

int fmhip_relational_sgd_epoch(fmhip_model_t m, fmhip_relational_t r, double eta, double reg0, double regw, double regv,
                               const int64_t *order, fmhip_stats *stats) {
    WriteLock lock(m);
    TRY(check_train_rel(m, r));
    const int64_t nb = (int64_t)r->batches.size();
    if (order)
        for (int64_t j = 0; j < nb; ++j) TRY(check_rel_batch(r, order[j]));
    HIP_TRY(hipMemsetAsync(m->acc.p, 0, 4 * sizeof(double), m->stream));
    const Sgd sgd{eta, reg0, regw, regv};
    int64_t nnz = 0;
    for (int64_t j = 0; j < nb; ++j) {
        TRY(rel_step(m, r, order ? order[j] : j, sgd, m->acc.p));
        nnz += m->step.last_nnz;
    }
    if (stats) {
        memset(stats, 0, sizeof *stats);
        TRY(read_acc(m, stats));
        stats->nnz = nnz;
        stats->steps = nb;
    }
    return FMHIP_OK;
}

}  // extern "C"
