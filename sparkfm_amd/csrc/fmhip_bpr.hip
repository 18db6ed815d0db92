// fmhip_bpr.hip — the BPR trainer (include/fmhip_bpr.h): the handle (an owned relational dataset of 2 n_pairs rows over the two
// borrowed blocks), the resample
//     k_bpr_sample (the candidates mapping's odd entries) -> per batch the inverse map on the device (fm_bpr.hip) -> the counts back
// (the scored samplers: the two blocks' kFwdQ forwards on the model's stream first, then k_bpr_sample_walk in k_bpr_sample's place —
// under the best-of-C rule, include/fmhip_bpr_adaptive.h, or under WARP's, include/fmhip_warp.h, which also leaves the pairs' weights
// for the step's hinge) and the training calls, which are the relational step in its pairs mode (rel_step, fmhip_relational.hip).
// A draw is queue_draw() — the sampler over a range of batches, then their inverse maps — and the counts come back by queue_fetch()
// / accept_counts(): resample() is the first over every batch on the handle's stream followed by the second; the per-batch redraw
// (include/fmhip_redraw.h; redraw_batch) queues one batch's draw between its step's forwards and the rest of the step on the
// model's stream and fetches once per epoch.  Every record call goes through record_scores().  The kernels are in fm_bpr.hip; the host arithmetic
// (the positives' lists, the sampler's twin) in fmhip_host.cpp.
#include "fmhip_internal.h"
#include "../../include/fmhip_bpr_adaptive.h"
#include "../../include/fmhip_warp.h"
#include "../../include/fmhip_redraw.h"
#include "../../include/fmhip_proposal.h"
#include "../../include/fmhip_softmax.h"
#include "fm_bpr.h"
#include "fm_relational.h"

#include <algorithm>
#include <cmath>
#include <memory>
#include <new>
#include <vector>

using namespace fmhip;
using namespace fmhip::host;

namespace {

int check_block(int device, fmhip_dataset_t d, const char *what) {
    if (!d) return fail(FMHIP_ERR_INVALID, "the %s block is NULL", what);
    if (d->device != device) return fail(FMHIP_ERR_INVALID, "the %s block is on device %d, not %d", what, d->device, device);
    if (d->scoring_only)
        return fail(FMHIP_ERR_UNSUPPORTED, "the %s block was created with fmhip_rows_create (scoring only): it has no transposes to train on", what);
    if (d->weighted)
        return fail(FMHIP_ERR_UNSUPPORTED, "the %s block carries example weights (fmhip_dataset_create_weighted): the BPR trainer takes unweighted blocks", what);
    if (d->batches.size() != 1)
        return fail(FMHIP_ERR_INVALID, "the %s block has %zu batches — create it with batch_rows = 0 (one batch of all its %lld rows)", what,
                    d->batches.size(), (long long)d->n_rows);
    return FMHIP_OK;
}

int check_bpr(fmhip_model_t m, fmhip_bpr_t h) {
    if (!h) return fail(FMHIP_ERR_INVALID, "the BPR trainer is NULL");
    return check_rel_model(m, h->R);
}

// the pairs of the batches [b0, b1): a batch holds 2 * batch_pairs rows, rows 2p and 2p + 1 one pair
void pair_range(fmhip_bpr_t h, size_t b0, size_t b1, int64_t *p0, int64_t *p1) {
    const fmhip_relational::Batch &first = h->R->batches[b0], &last = h->R->batches[b1 - 1];
    *p0 = first.row0 / 2;
    *p1 = (last.row0 + last.rows) / 2;
}

// a draw of the pairs [p0, p1) at epoch t whose counters' sums go to slot `slot` of h->total
BprSampleArgs sample_args(fmhip_bpr_t h, int64_t t, int64_t p0, int64_t p1, size_t slot) {
    BprSampleArgs sa{};
    sa.seed = h->seed;
    sa.t = (uint32_t)t;
    sa.n_pairs = (int32_t)h->n_pairs;
    sa.n_neg = h->n_neg;
    sa.M = (int32_t)h->M;
    sa.p0 = (int32_t)p0;
    sa.p1 = (int32_t)p1;
    sa.ictx = h->ictx.p;
    sa.pptr = h->pptr.p;
    sa.prow = h->prow.p;
    sa.map = h->R->rels[1]->map.p;
    sa.part = h->part.p;
    sa.total = h->total.p + 3 * slot;
    sa.tab = h->h_ptab.empty() ? nullptr : h->ptab.p;      // (the proposal, include/fmhip_proposal.h: every sampler's draws read it here)
    return sa;
}

// The samplers, and per sampler the counters its kernel sums, in the order of its public stats struct: uniform {attempts, forced}
// (fmhip_bpr_sample_stats), best of C {attempts, forced, replaced} (fmhip_bpr_adaptive_stats), WARP {violated, trials}
// (fmhip_warp_stats, behind `pairs`)
enum Sampler { kUniform, kBestOfC, kWarp };
constexpr int kCounters[] = {2, 3, 2};

// the sampler an epoch draws with
Sampler epoch_sampler(fmhip_bpr_t h) { return h->warp ? kWarp : h->n_cand > 1 ? kBestOfC : kUniform; }

int check_epoch_index(int64_t t) {
    if (t < 0 || t > 0xffffffffll) return fail(FMHIP_ERR_INVALID, "t = %lld: an epoch is in [0, 2^32)", (long long)t);
    return FMHIP_OK;
}

// a scored sampler's walk over the pairs [p0, p1) under m, its arguments alone (nothing queued): the partials sized for `which`
// over the whole set, -> wa->a and WARP's margin
int walk_args(fmhip_model_t m, fmhip_bpr_t h, int64_t t, Sampler which, int64_t p0, int64_t p1, size_t slot, BprWarpArgs *wa) {
    fmhip_relational_t R = h->R;
    TRY(h->part.ensure((size_t)kCounters[which] * (size_t)bpr_adaptive_blocks(m->Kp, h->n_pairs)));
    *wa = BprWarpArgs{};
    wa->a.s = sample_args(h, t, p0, p1, slot);
    wa->a.n_cand = h->n_cand;
    wa->a.k = m->k;
    wa->a.Qu = R->rels[0]->Q.p;
    wa->a.Qi = R->rels[1]->Q.p;
    wa->a.yqi = R->rels[1]->yq.p;
    wa->margin = (float)h->warp_margin;
    return FMHIP_OK;
}

// What a scored sampler's walk on the handle's own stream reads, queued: the two blocks' kFwdQ forwards on the model's stream
// (rel_block_forwards), the handle's stream behind them by an event — and behind the steps queued so far, which read the
// mapping.  -> walk_args
int scored_args(fmhip_model_t m, fmhip_bpr_t h, int64_t t, Sampler which, int64_t p0, int64_t p1, size_t slot, BprWarpArgs *wa) {
    fmhip_relational_t R = h->R;
    TRY(rel_block_forwards(m, R));
    if (!h->fwd_done) HIP_TRY(hipEventCreateWithFlags(&h->fwd_done, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(h->fwd_done, m->stream));
    HIP_TRY(hipStreamWaitEvent(h->stream, h->fwd_done, 0));
    if (R->busy_set) HIP_TRY(hipStreamWaitEvent(h->stream, R->busy, 0));
    return walk_args(m, h, t, which, p0, p1, slot, wa);
}

hipError_t launch_scored(Sampler which, int Kp, const BprWarpArgs &wa, hipStream_t s) {
    return which == kWarp ? launch_bpr_sample_warp(Kp, wa, s) : launch_bpr_sample_adaptive(Kp, wa.a, s);
}

// What a WARP draw reads on top of the walk's arguments, queued on stream s: the weight table (made on the host when the candidate
// count has changed, uploaded), and the room for what it writes: the pairs' weights and trial counts
int warp_table(fmhip_bpr_t h, hipStream_t s) {
    TRY(h->wc.ensure(2 * (size_t)h->n_pairs));
    TRY(h->wtrials.ensure((size_t)h->n_pairs));
    TRY(h->wtab.ensure((size_t)kBprMaxCand + 1));
    if (h->wtab_cand != h->n_cand) {
        h->h_wtab.assign((size_t)h->n_cand + 1, 0.f);
        warp_weight_table(h->M, h->n_cand, h->h_wtab.data());
        h->wtab_cand = h->n_cand;
    }
    HIP_TRY(hipMemcpyAsync(h->wtab.p, h->h_wtab.data(), h->h_wtab.size() * sizeof(float), hipMemcpyHostToDevice, s));
    return FMHIP_OK;
}

void warp_outputs(fmhip_bpr_t h, BprWarpArgs *wa) {
    wa->W = h->wtab.p;
    wa->c = h->wc.p;
    wa->trials = h->wtrials.p;
}

// the WARP draws that stand: batches [b0, b1) drawn (or, `have` false, every batch dropped); all of them: a draw of the whole set
void warp_mark(fmhip_bpr_t h, size_t b0, size_t b1, bool have) {
    const size_t nb = h->R->batches.size();
    if (!have) {
        h->warp_have.assign(nb, 0);
        h->warp_drawn = false;
        return;
    }
    h->warp_have.resize(nb, 0);
    for (size_t b = b0; b < b1; ++b) h->warp_have[b] = 1;
    h->warp_drawn = std::find(h->warp_have.begin(), h->warp_have.end(), (char)0) == h->warp_have.end();
}

// Queues on stream s: sampler `which` at epoch t over the pairs of the batches [b0, b1) (one launch; its counters into slot b0 of
// h->total), then the inverse map of each of those batches, the counts left on the device.  own_stream: s is the handle's stream
// — a scored sampler's forwards are queued on the model's and s put behind them and behind the steps queued so far; else s is the
// model's stream, on which the caller has queued rel_block_forwards for this model state (and, WARP, warp_table).  A scored
// sampler draws under m (the caller has checked the two against each other and holds the model's lock); the uniform one reads none
int queue_draw(fmhip_bpr_t h, int64_t t, Sampler which, fmhip_model_t m, size_t b0, size_t b1, hipStream_t s, bool own_stream) {
    fmhip_relational_t R = h->R;
    fmhip_relational::Relation &rel = *R->rels[1];
    int64_t p0 = 0, p1 = 0;
    pair_range(h, b0, b1, &p0, &p1);
    if (which == kUniform) {
        // the mapping and the inverse map are read by the steps queued so far
        if (own_stream && R->busy_set) HIP_TRY(hipStreamWaitEvent(s, R->busy, 0));
        HIP_TRY(launch_bpr_sample(sample_args(h, t, p0, p1, b0), s));
    } else {
        BprWarpArgs wa{};
        if (own_stream) TRY(scored_args(m, h, t, which, p0, p1, b0, &wa));
        else TRY(walk_args(m, h, t, which, p0, p1, b0, &wa));
        if (which == kWarp) {
            if (own_stream) TRY(warp_table(h, s));
            warp_outputs(h, &wa);
        }
        HIP_TRY(launch_scored(which, m->Kp, wa, s));
    }
    for (size_t b = b0; b < b1; ++b) {
        const RelationInverse::Batch &ib = rel.batches[b];
        BprInverseArgs ia{};
        ia.map = rel.map.p + R->batches[b].row0;
        ia.rows = (int32_t)R->batches[b].rows;
        ia.block_rows = (int32_t)h->M;
        ia.cut = kRelSumCut;
        ia.trow = rel.trow.p + ib.row_off;
        ia.tptr = rel.tptr.p + ib.tptr_off;
        ia.tj = rel.tj.p + ib.t_off;
        ia.wt = rel.wt.p + ib.w_off;
        ia.wbeg = rel.wbeg.p + ib.w_off;
        ia.wdst = rel.wdst.p + ib.w_off;
        ia.lt = rel.lt.p + ib.l_off;
        ia.lfirst = rel.lfirst.p + ib.l_off;
        ia.lcount = rel.lcount.p + ib.l_off;
        ia.counts = h->counts.p + 4 * b;
        HIP_TRY(launch_bpr_inverse(ia, h->work.p, h->work.n, s));
        h->stale[b] = 1;
    }
    h->any_stale = true;
    return FMHIP_OK;
}

// every batch's counts and every slot of the samplers' counters, on their way back on stream s: good once s has been synchronised
struct Fetched {
    std::vector<int32_t> counts;
    std::vector<unsigned long long> total;
};

int queue_fetch(fmhip_bpr_t h, hipStream_t s, Fetched *f) {
    const size_t nb = h->R->batches.size();
    f->counts.assign(4 * nb, 0);
    f->total.assign(3 * nb, 0);
    HIP_TRY(hipMemcpyAsync(f->counts.data(), h->counts.p, f->counts.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(f->total.data(), h->total.p, f->total.size() * sizeof f->total[0], hipMemcpyDeviceToHost, s));
    return FMHIP_OK;
}

// the fetched counts checked against what the slices and the step's partial rows are sized for, then the host's copy refreshed
int accept_counts(fmhip_bpr_t h, const Fetched &f) {
    fmhip_relational_t R = h->R;
    fmhip_relational::Relation &rel = *R->rels[1];
    const size_t nb = R->batches.size();
    for (size_t b = 0; b < nb; ++b) {
        const int32_t *c = f.counts.data() + 4 * b;
        const int64_t rows = R->batches[b].rows;
        if (c[0] < 1 || c[0] > rows || c[1] < c[0] || c[1] > rows || c[2] < 0 || c[2] >= rel_long_cap(rows) || c[3] < 0 || c[3] > 2 * rel_long_cap(rows))
            return fail(FMHIP_ERR_HIP, "the inverse map of batch %zu came back with counts {%d, %d, %d, %d} for %lld rows", b, c[0], c[1], c[2], c[3],
                        (long long)rows);
    }
    for (size_t b = 0; b < nb; ++b) {
        RelationInverse::Batch &ib = rel.batches[b];
        const int32_t *c = f.counts.data() + 4 * b;
        ib.n_touched = c[0];
        ib.n_work = c[1];
        ib.n_long = c[2];
        ib.n_part = c[3];
        h->stale[b] = 0;
    }
    h->any_stale = false;
    return FMHIP_OK;
}

// the host's counts, for a call that reads them — and the draw itself, for a call that reads the mapping or WARP's outputs from
// the host: when a per-batch draw has been queued and not fetched since, one fetch (one synchronisation, the handle's stream
// behind the steps queued so far, hence behind every draw)
int fresh_counts(fmhip_bpr_t h) {
    if (!h->any_stale) return FMHIP_OK;
    TRY(set_device(h->device));
    if (h->R->busy_set) HIP_TRY(hipStreamWaitEvent(h->stream, h->R->busy, 0));
    Fetched f;
    TRY(queue_fetch(h, h->stream, &f));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return accept_counts(h, f);
}

// sampler `which` at epoch t over the whole set, the inverse map of every batch, the batches' counts (one synchronisation); the
// handle's own stream.  total_out: the sampler's kCounters[which] counters
int resample(fmhip_bpr_t h, int64_t t, Sampler which, fmhip_model_t m, int64_t *total_out) {
    TRY(check_epoch_index(t));
    TRY(set_device(h->device));
    if (which == kWarp) warp_mark(h, 0, 0, false);      // (until this draw has come back whole)
    const size_t nb = h->R->batches.size();
    TRY(queue_draw(h, t, which, m, 0, nb, h->stream, true));
    Fetched f;
    TRY(queue_fetch(h, h->stream, &f));
    HIP_TRY(hipStreamSynchronize(h->stream));
    TRY(accept_counts(h, f));
    if (which == kWarp) warp_mark(h, 0, nb, true);
    if (total_out)
        for (int i = 0; i < kCounters[which]; ++i) total_out[i] = (int64_t)f.total[(size_t)i];
    return FMHIP_OK;
}

// a sampler's counters of one draw over `pairs` pairs, added to the public six {pairs, attempts, forced, replaced, violated, trials}
void add_draw(Sampler which, const unsigned long long *tot, int64_t pairs, int64_t (&out)[6]) {
    out[0] += pairs;
    const int at = which == kWarp ? 4 : 1;
    for (int i = 0; i < kCounters[which]; ++i) out[at + i] += (int64_t)tot[i];
}

void put_draw(const int64_t (&v)[6], fmhip_redraw_stats *out) {
    out->pairs = v[0];
    out->attempts = v[1];
    out->forced = v[2];
    out->replaced = v[3];
    out->violated = v[4];
    out->trials = v[5];
}

// ---- the sampled softmax (include/fmhip_softmax.h) ----
// the correction is in force: switch and request on, a weighted proposal
bool logq_in_force(fmhip_bpr_t h) { return h->softmax && h->sm_logq && !h->h_pw.empty(); }

// the log-Q table on both sides as the switch and the proposal now stand (the caller has waited for the steps queued so far)
int refresh_logq(fmhip_bpr_t h) {
    h->h_lq.clear();
    if (!logq_in_force(h)) return FMHIP_OK;
    h->h_lq.resize((size_t)h->M);
    bpr_log_proposal(h->M, h->h_pw.data(), h->h_lq.data());
    TRY(h->lq.ensure(h->h_lq.size()));
    HIP_TRY(hipMemcpy(h->lq.p, h->h_lq.data(), h->h_lq.size() * sizeof(float), hipMemcpyHostToDevice));
    return FMHIP_OK;
}

// every draw and step queued so far has finished (the per-batch ones are on the model's stream, in front of the step that records R->busy)
int wait_queued(fmhip_bpr_t h) {
    TRY(set_device(h->device));
    if (h->R->busy_set) HIP_TRY(hipEventSynchronize(h->R->busy));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return FMHIP_OK;
}

// a batch splits an interaction: its pairs are no multiple of n_neg (one batch never does)
bool splits_interactions(fmhip_bpr_t h) { return h->R->batches.size() > 1 && h->batch_pairs % h->n_neg != 0; }

// batch b has had a softmax step: its probabilities stand
void softmax_mark(fmhip_bpr_t h, int64_t b) {
    if (!h->softmax) return;
    h->sm_have.resize(h->R->batches.size(), 0);
    h->sm_have[(size_t)b] = 1;
}

// What a step of this handle trains in the model's loss's place: the softmax rule (its buffers sized here), or — `warp_drawn`: the
// caller vouches for the WARP draw — the WARP hinge on the standing weights; neither switch on: the model's loss (*out = nullptr)
int step_rule(fmhip_bpr_t h, bool warp_drawn, PairHinge *store, const PairHinge **out) {
    *out = nullptr;
    if (h->softmax) {
        TRY(h->sm_pi.ensure(2 * (size_t)h->n_pairs));
        TRY(h->sm_bsum.ensure(4 * (size_t)softmax_blocks(h->n_neg, h->R->max_rows / (2 * (int64_t)h->n_neg))));
        *store = PairHinge{};
        store->softmax_n = h->n_neg;
        store->pi = h->sm_pi.p;
        store->lq = logq_in_force(h) ? h->lq.p : nullptr;
        store->sm_bsum = h->sm_bsum.p;
        *out = store;
    } else if (h->warp && warp_drawn) {
        *store = PairHinge{h->wc.p, (float)h->warp_margin};
        *out = store;
    }
    return FMHIP_OK;
}

// One batch of the per-batch redraw (include/fmhip_redraw.h), queued on the model's stream: the blocks' forwards under the model
// as it stands, the draw of the batch's pairs, the batch's inverse map, the rest of the step with the counts read on the device.
// WARP: the caller has queued warp_table on the model's stream
int redraw_batch(fmhip_model_t m, fmhip_bpr_t h, int64_t t, Sampler which, int64_t b, const Sgd &sgd, double *acc) {
    fmhip_relational_t R = h->R;
    TRY(rel_block_forwards(m, R));
    TRY(queue_draw(h, t, which, m, (size_t)b, (size_t)b + 1, m->stream, false));
    PairHinge rule_store{};
    const PairHinge *rule = nullptr;
    TRY(step_rule(h, which == kWarp, &rule_store, &rule));
    const int32_t *dev_counts[2] = {nullptr, h->counts.p + 4 * b};
    RelStepQueued queued;
    queued.forwards = true;
    queued.dev_counts = dev_counts;
    TRY(rel_step(m, R, b, sgd, acc, true, rule, queued));
    if (which == kWarp) warp_mark(h, (size_t)b, (size_t)b + 1, true);
    softmax_mark(h, b);
    return FMHIP_OK;
}

// Record mode of a scored sampler's walk for pairs [p0, p1) at epoch t, the mapping left alone: every candidate's row and score
// and, WARP, the positives' scores
int record_scores(fmhip_model_t m, fmhip_bpr_t h, int64_t t, int64_t p0, int64_t p1, Sampler which, int32_t *rows, float *scores, float *pos_scores) {
    TRY(check_bpr(m, h));
    TRY(check_epoch_index(t));
    if (p0 < 0 || p1 > h->n_pairs || p0 >= p1)
        return fail(FMHIP_ERR_INVALID, "pairs [%lld, %lld): a non-empty range inside [0, %lld)", (long long)p0, (long long)p1, (long long)h->n_pairs);
    if (!rows || !scores || (which == kWarp && !pos_scores)) return fail(FMHIP_ERR_INVALID, "an out array is NULL");
    const size_t np = (size_t)(p1 - p0), n = np * (size_t)h->n_cand;
    TRY(h->rec_rows.ensure(n));
    TRY(h->rec_scores.ensure(n));
    if (which == kWarp) TRY(h->rec_pos.ensure(np));
    BprWarpArgs wa{};
    TRY(scored_args(m, h, t, which, p0, p1, 0, &wa));
    wa.a.rec_rows = h->rec_rows.p;
    wa.a.rec_scores = h->rec_scores.p;
    wa.rec_pos = h->rec_pos.p;
    HIP_TRY(launch_scored(which, m->Kp, wa, h->stream));
    HIP_TRY(hipMemcpyAsync(rows, h->rec_rows.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(scores, h->rec_scores.p, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    if (which == kWarp) HIP_TRY(hipMemcpyAsync(pos_scores, h->rec_pos.p, np * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return FMHIP_OK;
}

// a handle whose WARP switch is on takes its draws from fmhip_warp_resample alone
int refuse_under_warp(fmhip_bpr_t h, const char *call) {
    if (h->warp) return fail(FMHIP_ERR_INVALID, "%s: WARP is on for this trainer (fmhip_warp_set) — its draw is fmhip_warp_resample", call);
    return FMHIP_OK;
}

// the rule a step on the STANDING draw trains (step_rule); WARP on without a standing WARP draw: refused
int step_hinge(fmhip_bpr_t h, PairHinge *store, const PairHinge **out) {
    if (h->warp && !h->warp_drawn)
        return fail(FMHIP_ERR_INVALID, "WARP is on and no WARP draw stands since fmhip_warp_set: call fmhip_warp_resample (or fmhip_bpr_epoch) first");
    return step_rule(h, true, store, out);
}

// fmhip_bpr_epoch in the per-batch mode: every batch's forwards, draw, inverse map and step in stream order on the model's stream,
// then ONE synchronisation — the statistics' copy when the caller wants them, the stream's otherwise — that also brings back every
// batch's counts and the sampler's counters per batch (the caller holds the model's lock and has checked m, h and the order)
int redraw_epoch(fmhip_model_t m, fmhip_bpr_t h, int64_t t, const Sgd &sgd, const int64_t *order, fmhip_stats *stats) {
    TRY(check_epoch_index(t));
    const Sampler which = epoch_sampler(h);
    const int64_t nb = (int64_t)h->R->batches.size();
    h->have_epoch_draw = false;
    if (which == kWarp) {
        warp_mark(h, 0, 0, false);
        TRY(warp_table(h, m->stream));
    }
    HIP_TRY(hipMemsetAsync(h->total.p, 0, 3 * (size_t)nb * sizeof(unsigned long long), m->stream));      // (a batch the order leaves out)
    HIP_TRY(hipMemsetAsync(m->acc.p, 0, 4 * sizeof(double), m->stream));
    int64_t nnz = 0;
    std::vector<char> visited((size_t)nb, 0);
    for (int64_t j = 0; j < nb; ++j) {
        const int64_t b = order ? order[j] : j;
        TRY(redraw_batch(m, h, t, which, b, sgd, m->acc.p));
        visited[(size_t)b] = 1;
        nnz += m->step.last_nnz;
    }
    Fetched f;
    TRY(queue_fetch(h, m->stream, &f));
    if (stats) {
        memset(stats, 0, sizeof *stats);
        TRY(read_acc(m, stats));      // (synchronises the model's stream: the fetch has landed)
        stats->nnz = nnz;
        stats->steps = nb;
    } else {
        HIP_TRY(hipStreamSynchronize(m->stream));
    }
    TRY(accept_counts(h, f));
    int64_t sum[6] = {0, 0, 0, 0, 0, 0};
    for (int64_t b = 0; b < nb; ++b)
        if (visited[(size_t)b]) add_draw(which, f.total.data() + 3 * b, h->R->batches[(size_t)b].rows / 2, sum);
    memcpy(h->epoch_draw, sum, sizeof sum);
    h->have_epoch_draw = true;
    return FMHIP_OK;
}

}  // namespace

extern "C" {

int fmhip_bpr_create(int device, fmhip_dataset_t contexts, fmhip_dataset_t candidates, int64_t n_inter, const int32_t *inter_ctx,
                     const int32_t *inter_cand, int32_t n_neg, int64_t batch_pairs, uint64_t seed, fmhip_bpr_t *out) {
    if (!out) return fail(FMHIP_ERR_INVALID, "out is NULL");
    *out = nullptr;
    // ---- the host checks (no HIP call before they have passed)
    if (n_neg < 1) return fail(FMHIP_ERR_INVALID, "n_neg = %d: every interaction needs at least one negative", (int)n_neg);
    TRY(check_block(device, contexts, "contexts"));
    TRY(check_block(device, candidates, "candidates"));
    const int64_t n_ctx = contexts->n_rows, M = candidates->n_rows;
    if (M < 2) return fail(FMHIP_ERR_INVALID, "the candidates block has %lld rows: a pair needs at least 2 candidate rows", (long long)M);
    if (n_inter < 1) return fail(FMHIP_ERR_INVALID, "n_inter = %lld: the trainer needs at least one interaction", (long long)n_inter);
    if (!inter_ctx || !inter_cand) return fail(FMHIP_ERR_INVALID, "inter_ctx or inter_cand is NULL");
    if (2 * (n_inter * (int64_t)n_neg) >= ((int64_t)1 << 31) || n_inter >= ((int64_t)1 << 31))
        return fail(FMHIP_ERR_INVALID, "n_pairs = n_neg * n_inter = %d * %lld: the 2 * n_pairs rows must number less than 2^31", (int)n_neg,
                    (long long)n_inter);
    for (int64_t i = 0; i < n_inter; ++i) {
        if (inter_ctx[i] < 0 || inter_ctx[i] >= n_ctx)
            return fail(FMHIP_ERR_INVALID, "interaction %lld names context row %d, outside the contexts block's rows [0, %lld)", (long long)i,
                        (int)inter_ctx[i], (long long)n_ctx);
        if (inter_cand[i] < 0 || inter_cand[i] >= M)
            return fail(FMHIP_ERR_INVALID, "interaction %lld names candidate row %d, outside the candidates block's rows [0, %lld)", (long long)i,
                        (int)inter_cand[i], (long long)M);
    }
    std::vector<int64_t> pptr;
    std::vector<int32_t> prow;
    bpr_positive_lists(n_ctx, n_inter, inter_ctx, inter_cand, pptr, prow);
    for (int64_t u = 0; u < n_ctx; ++u)
        if (pptr[(size_t)u + 1] - pptr[(size_t)u] >= M)
            return fail(FMHIP_ERR_INVALID, "context %lld has all %lld candidate rows as positives: no negative exists for it", (long long)u, (long long)M);
    {
        std::vector<int32_t> feats[2];
        part_features(contexts, feats[0]);
        part_features(candidates, feats[1]);
        const int32_t *fp[2] = {feats[0].data(), feats[1].data()};
        const int64_t fn[2] = {(int64_t)feats[0].size(), (int64_t)feats[1].size()};
        const SharedFeature sh = first_shared_feature(2, fp, fn, std::max(contexts->dimension, candidates->dimension));
        if (sh.feature >= 0)
            return fail(FMHIP_ERR_INVALID, "feature %d occurs in the contexts block and in the candidates block: the blocks' feature sets must be "
                                           "disjoint (every block's backward stores its gradient rows)", (int)sh.feature);
    }
    // ---- the relational dataset it stands for (the negatives' entries hold the positive until the first draw)
    const int64_t n_pairs = n_inter * n_neg, N = 2 * n_pairs;
    if (batch_pairs <= 0 || batch_pairs > n_pairs) batch_pairs = n_pairs;
    std::unique_ptr<fmhip_bpr> H(new (std::nothrow) fmhip_bpr());
    if (!H) return fail(FMHIP_ERR_NOMEM, "out of host memory");
    H->device = device;
    H->n_inter = n_inter;
    H->n_pairs = n_pairs;
    H->batch_pairs = batch_pairs;
    H->n_ctx = n_ctx;
    H->M = M;
    H->n_neg = n_neg;
    H->seed = seed;
    {
        std::vector<double> y((size_t)N);
        std::vector<int32_t> mc((size_t)N), mi((size_t)N);
        for (int64_t p = 0; p < n_pairs; ++p) {
            const int64_t i = p / n_neg;
            y[(size_t)(2 * p)] = 1.0;
            y[(size_t)(2 * p + 1)] = 0.0;
            mc[(size_t)(2 * p)] = mc[(size_t)(2 * p + 1)] = inter_ctx[i];
            mi[(size_t)(2 * p)] = mi[(size_t)(2 * p + 1)] = inter_cand[i];
        }
        const fmhip_dataset_t blocks[2] = {contexts, candidates};
        const int32_t *maps[2] = {mc.data(), mi.data()};
        TRY(fmhip_relational_create(device, N, y.data(), 2, blocks, maps, nullptr, 2 * batch_pairs, &H->R));
    }
    TRY(set_device(device));
    fmhip_relational_t R = H->R;
    fmhip_relational::Relation &rel = *R->rels[1];
    // the candidates relation's inverse map: buffers at their worst case, O(rows + rows / cut) in all, filled by the device
    const size_t nb = R->batches.size();
    int64_t l_total = 0;
    for (size_t b = 0; b < nb; ++b) {
        RelationInverse::Batch &ib = rel.batches[b];
        ib = RelationInverse::Batch{};
        ib.row_off = ib.t_off = ib.w_off = R->batches[b].row0;
        ib.tptr_off = R->batches[b].row0 + (int64_t)b;
        ib.l_off = l_total;
        l_total += rel_long_cap(R->batches[b].rows);
    }
    // the partial rows of the long lists, at their worst case too (a few KB per 1000 rows): whatever a draw gives fits, so the step
    // never waits for a count to size its workspace
    rel.max_part = (int32_t)(2 * rel_long_cap(R->max_rows));
    H->stale.assign(nb, 0);
    TRY(rel.trow.alloc((size_t)N)); TRY(rel.tj.alloc((size_t)N)); TRY(rel.tptr.alloc((size_t)N + nb));
    TRY(rel.wt.alloc((size_t)N)); TRY(rel.wbeg.alloc((size_t)N)); TRY(rel.wdst.alloc((size_t)N));
    TRY(rel.lt.alloc((size_t)l_total)); TRY(rel.lfirst.alloc((size_t)l_total)); TRY(rel.lcount.alloc((size_t)l_total));
    TRY(H->counts.alloc(4 * nb));
    TRY(H->ictx.alloc((size_t)n_inter));
    HIP_TRY(hipMemcpy(H->ictx.p, inter_ctx, (size_t)n_inter * sizeof(int32_t), hipMemcpyHostToDevice));
    TRY(H->pptr.alloc(pptr.size()));
    HIP_TRY(hipMemcpy(H->pptr.p, pptr.data(), pptr.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    TRY(H->prow.alloc(std::max<size_t>(prow.size(), 1)));
    if (!prow.empty()) HIP_TRY(hipMemcpy(H->prow.p, prow.data(), prow.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    TRY(H->part.alloc(2 * (size_t)bpr_sample_blocks(n_pairs)));      // (the uniform sampler's need; the scored ones grow it)
    TRY(H->total.alloc(3 * nb));
    size_t work = 0;
    HIP_TRY(bpr_inverse_workspace((int32_t)R->max_rows, (int32_t)M, &work));
    TRY(H->work.alloc(work));
    HIP_TRY(hipStreamCreateWithFlags(&H->stream, hipStreamNonBlocking));
    TRY(resample(H.get(), 0, kUniform, nullptr, nullptr));
    *out = H.release();
    return FMHIP_OK;
}

int fmhip_bpr_destroy(fmhip_bpr_t h) {
    if (!h) return FMHIP_OK;
    (void)hipSetDevice(h->device);
    std::unique_ptr<fmhip_bpr>(h).reset();
    return FMHIP_OK;
}

int fmhip_bpr_info(fmhip_bpr_t h, int64_t *n_pairs, int64_t *dimension, int64_t *batch_pairs, int64_t *n_batches, int32_t *n_neg) {
    if (!h) return fail(FMHIP_ERR_INVALID, "the BPR trainer is NULL");
    if (n_pairs) *n_pairs = h->n_pairs;
    if (dimension) *dimension = h->R->dimension;
    if (batch_pairs) *batch_pairs = h->batch_pairs;
    if (n_batches) *n_batches = (int64_t)h->R->batches.size();
    if (n_neg) *n_neg = h->n_neg;
    return FMHIP_OK;
}

int fmhip_bpr_resample(fmhip_bpr_t h, int64_t t, fmhip_bpr_sample_stats *stats) {
    if (!h) return fail(FMHIP_ERR_INVALID, "the BPR trainer is NULL");
    TRY(refuse_under_warp(h, "fmhip_bpr_resample"));
    int64_t total[3];
    TRY(resample(h, t, kUniform, nullptr, total));
    if (stats) {
        stats->attempts = total[0];
        stats->forced = total[1];
    }
    return FMHIP_OK;
}

int fmhip_bpr_set_candidates(fmhip_bpr_t h, int32_t n_cand) {
    if (!h) return fail(FMHIP_ERR_INVALID, "the BPR trainer is NULL");
    if (n_cand < 1 || n_cand > FMHIP_BPR_MAX_CANDIDATES)
        return fail(FMHIP_ERR_INVALID, "n_cand = %d: a pair has 1 .. %d candidates", (int)n_cand, FMHIP_BPR_MAX_CANDIDATES);
    h->n_cand = n_cand;
    return FMHIP_OK;
}

int fmhip_bpr_get_candidates(fmhip_bpr_t h, int32_t *n_cand) {
    if (!h) return fail(FMHIP_ERR_INVALID, "the BPR trainer is NULL");
    if (!n_cand) return fail(FMHIP_ERR_INVALID, "n_cand is NULL");
    *n_cand = h->n_cand;
    return FMHIP_OK;
}

int fmhip_bpr_resample_adaptive(fmhip_model_t m, fmhip_bpr_t h, int64_t t, fmhip_bpr_adaptive_stats *stats) {
    WriteLock lock(m);
    TRY(check_bpr(m, h));
    TRY(refuse_under_warp(h, "fmhip_bpr_resample_adaptive"));
    int64_t total[3];
    TRY(resample(h, t, kBestOfC, m, total));
    if (stats) {
        stats->attempts = total[0];
        stats->forced = total[1];
        stats->replaced = total[2];
    }
    return FMHIP_OK;
}

int fmhip_bpr_debug_adaptive(fmhip_model_t m, struct fmhip_bpr *h, int64_t t, int64_t p0, int64_t p1, int32_t *rows, float *scores) {
    WriteLock lock(m);
    return record_scores(m, h, t, p0, p1, kBestOfC, rows, scores, nullptr);
}

// ---- WARP (include/fmhip_warp.h) ----------------------------------------------------------------------------------------------------

int fmhip_warp_set(fmhip_bpr_t h, int enabled, double margin) {
    if (!h) return fail(FMHIP_ERR_INVALID, "the BPR trainer is NULL");
    if (!(margin >= 0.0) || !std::isfinite(margin) || !std::isfinite((float)margin))
        return fail(FMHIP_ERR_INVALID, "margin = %g: the WARP margin is a finite number >= 0", margin);
    if (enabled && h->softmax)
        return fail(FMHIP_ERR_INVALID, "fmhip_warp_set: the softmax switch is on for this trainer (fmhip_softmax_set) — WARP trains its own hinge; turn the softmax off first");
    h->warp = enabled != 0;
    h->warp_margin = margin;
    warp_mark(h, 0, 0, false);
    return FMHIP_OK;
}

int fmhip_warp_get(fmhip_bpr_t h, int *enabled, double *margin) {
    if (!h) return fail(FMHIP_ERR_INVALID, "the BPR trainer is NULL");
    if (enabled) *enabled = h->warp ? 1 : 0;
    if (margin) *margin = h->warp_margin;
    return FMHIP_OK;
}

int fmhip_warp_resample(fmhip_model_t m, fmhip_bpr_t h, int64_t t, fmhip_warp_stats *stats) {
    WriteLock lock(m);
    TRY(check_bpr(m, h));
    if (!h->warp) return fail(FMHIP_ERR_INVALID, "WARP is off for this trainer: turn it on with fmhip_warp_set");
    int64_t total[3];
    TRY(resample(h, t, kWarp, m, total));
    if (stats) {
        stats->pairs = h->n_pairs;
        stats->violated = total[0];
        stats->trials = total[1];
    }
    return FMHIP_OK;
}

int fmhip_warp_weights(fmhip_bpr_t h, float *out) {
    if (!h) return fail(FMHIP_ERR_INVALID, "the BPR trainer is NULL");
    if (!out) return fail(FMHIP_ERR_INVALID, "out is NULL");
    if (!h->warp_drawn) return fail(FMHIP_ERR_INVALID, "no WARP draw stands: call fmhip_warp_resample first");
    TRY(set_device(h->device));
    TRY(fresh_counts(h));      // (behind the per-batch draws queued so far)
    std::vector<float> c((size_t)(2 * h->n_pairs));
    HIP_TRY(hipMemcpy(c.data(), h->wc.p, c.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (int64_t p = 0; p < h->n_pairs; ++p) out[p] = c[(size_t)(2 * p)];
    return FMHIP_OK;
}

int fmhip_warp_trials(fmhip_bpr_t h, int32_t *out) {
    if (!h) return fail(FMHIP_ERR_INVALID, "the BPR trainer is NULL");
    if (!out) return fail(FMHIP_ERR_INVALID, "out is NULL");
    if (!h->warp_drawn) return fail(FMHIP_ERR_INVALID, "no WARP draw stands: call fmhip_warp_resample first");
    TRY(set_device(h->device));
    TRY(fresh_counts(h));
    HIP_TRY(hipMemcpy(out, h->wtrials.p, (size_t)h->n_pairs * sizeof(int32_t), hipMemcpyDeviceToHost));
    return FMHIP_OK;
}

int fmhip_warp_debug(fmhip_model_t m, struct fmhip_bpr *h, int64_t t, int64_t p0, int64_t p1, int32_t *rows, float *scores, float *pos_scores) {
    WriteLock lock(m);
    return record_scores(m, h, t, p0, p1, kWarp, rows, scores, pos_scores);
}

int fmhip_bpr_negatives(fmhip_bpr_t h, int32_t *out) {
    if (!h) return fail(FMHIP_ERR_INVALID, "the BPR trainer is NULL");
    if (!out) return fail(FMHIP_ERR_INVALID, "out is NULL");
    TRY(set_device(h->device));
    TRY(fresh_counts(h));      // (a per-batch draw queued without a synchronisation writes the mapping: behind it)
    std::vector<int32_t> map((size_t)(2 * h->n_pairs));
    HIP_TRY(hipMemcpy(map.data(), h->R->rels[1]->map.p, map.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (int64_t p = 0; p < h->n_pairs; ++p) out[p] = map[(size_t)(2 * p + 1)];
    return FMHIP_OK;
}

int fmhip_bpr_step(fmhip_model_t m, fmhip_bpr_t h, int64_t batch, double eta, double reg0, double regw, double regv, fmhip_stats *stats) {
    WriteLock lock(m);
    TRY(check_bpr(m, h));
    if (batch < 0 || batch >= (int64_t)h->R->batches.size())
        return fail(FMHIP_ERR_INVALID, "batch %lld out of range [0, %zu)", (long long)batch, h->R->batches.size());
    PairHinge hinge_store{};
    const PairHinge *hinge = nullptr;
    TRY(step_hinge(h, &hinge_store, &hinge));
    TRY(fresh_counts(h));      // (the step sizes its gather from the host's counts)
    TRY(rel_step(m, h->R, batch, Sgd{eta, reg0, regw, regv}, nullptr, true, hinge));
    softmax_mark(h, batch);
    if (stats) {
        memset(stats, 0, sizeof *stats);
        TRY(read_scal(m, stats));
        stats->nnz = m->step.last_nnz;
        stats->steps = 1;
    }
    return FMHIP_OK;
}

int fmhip_bpr_epoch(fmhip_model_t m, fmhip_bpr_t h, int64_t t, double eta, double reg0, double regw, double regv, const int64_t *order,
                    fmhip_stats *stats) {
    WriteLock lock(m);
    TRY(check_bpr(m, h));
    const int64_t nb = (int64_t)h->R->batches.size();
    if (order)
        for (int64_t j = 0; j < nb; ++j)
            if (order[j] < 0 || order[j] >= nb) return fail(FMHIP_ERR_INVALID, "batch %lld out of range [0, %lld)", (long long)order[j], (long long)nb);
    if (h->redraw == FMHIP_REDRAW_BATCH) return redraw_epoch(m, h, t, Sgd{eta, reg0, regw, regv}, order, stats);
    TRY(resample(h, t, epoch_sampler(h), m, nullptr));
    PairHinge hinge_store{};
    const PairHinge *hinge = nullptr;
    TRY(step_hinge(h, &hinge_store, &hinge));
    HIP_TRY(hipMemsetAsync(m->acc.p, 0, 4 * sizeof(double), m->stream));
    const Sgd sgd{eta, reg0, regw, regv};
    int64_t nnz = 0;
    for (int64_t j = 0; j < nb; ++j) {
        TRY(rel_step(m, h->R, order ? order[j] : j, sgd, m->acc.p, true, hinge));
        softmax_mark(h, order ? order[j] : j);
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

// ---- the redraw mode (include/fmhip_redraw.h) -------------------------------------------------------------------------------------------

int fmhip_redraw_set(fmhip_bpr_t h, int mode) {
    if (!h) return fail(FMHIP_ERR_INVALID, "the BPR trainer is NULL");
    if (mode != FMHIP_REDRAW_EPOCH && mode != FMHIP_REDRAW_BATCH)
        return fail(FMHIP_ERR_INVALID, "mode = %d: the redraw mode is FMHIP_REDRAW_EPOCH (%d) or FMHIP_REDRAW_BATCH (%d)", mode, FMHIP_REDRAW_EPOCH,
                    FMHIP_REDRAW_BATCH);
    h->redraw = mode;
    return FMHIP_OK;
}

int fmhip_redraw_get(fmhip_bpr_t h, int *mode) {
    if (!h) return fail(FMHIP_ERR_INVALID, "the BPR trainer is NULL");
    if (!mode) return fail(FMHIP_ERR_INVALID, "mode is NULL");
    *mode = h->redraw;
    return FMHIP_OK;
}

int fmhip_redraw_step(fmhip_model_t m, fmhip_bpr_t h, int64_t t, int64_t batch, double eta, double reg0, double regw, double regv,
                      fmhip_stats *stats, fmhip_redraw_stats *draw) {
    WriteLock lock(m);
    TRY(check_bpr(m, h));
    if (batch < 0 || batch >= (int64_t)h->R->batches.size())
        return fail(FMHIP_ERR_INVALID, "batch %lld out of range [0, %zu)", (long long)batch, h->R->batches.size());
    TRY(check_epoch_index(t));
    const Sampler which = epoch_sampler(h);
    if (which == kWarp) TRY(warp_table(h, m->stream));
    TRY(redraw_batch(m, h, t, which, batch, Sgd{eta, reg0, regw, regv}, nullptr));
    if (!stats && !draw) return FMHIP_OK;
    Fetched f;
    TRY(queue_fetch(h, m->stream, &f));
    if (stats) {
        memset(stats, 0, sizeof *stats);
        TRY(read_scal(m, stats));      // (synchronises the model's stream: the fetch has landed)
        stats->nnz = m->step.last_nnz;
        stats->steps = 1;
    } else {
        HIP_TRY(hipStreamSynchronize(m->stream));
    }
    TRY(accept_counts(h, f));
    if (draw) {
        int64_t v[6] = {0, 0, 0, 0, 0, 0};
        add_draw(which, f.total.data() + 3 * batch, h->R->batches[(size_t)batch].rows / 2, v);
        put_draw(v, draw);
    }
    return FMHIP_OK;
}

int fmhip_redraw_epoch_stats(fmhip_bpr_t h, fmhip_redraw_stats *out) {
    if (!h) return fail(FMHIP_ERR_INVALID, "the BPR trainer is NULL");
    if (!out) return fail(FMHIP_ERR_INVALID, "out is NULL");
    if (!h->have_epoch_draw)
        return fail(FMHIP_ERR_INVALID, "no per-batch epoch has run: fmhip_redraw_set(h, FMHIP_REDRAW_BATCH), then fmhip_bpr_epoch");
    put_draw(h->epoch_draw, out);
    return FMHIP_OK;
}

// ---- the proposal (include/fmhip_proposal.h) --------------------------------------------------------------------------------------------

int fmhip_proposal_set(fmhip_bpr_t h, const double *weights) {
    if (!h) return fail(FMHIP_ERR_INVALID, "the BPR trainer is NULL");
    std::vector<rng::AliasEntry> tab;
    if (weights) {
        tab.resize((size_t)h->M);
        const int64_t bad = bpr_alias_table(h->M, weights, tab.data());
        if (bad == -2) return fail(FMHIP_ERR_INVALID, "the sum of the %lld weights is not finite", (long long)h->M);
        if (bad >= 0) return fail(FMHIP_ERR_INVALID, "weights[%lld] = %g: a proposal weight is finite and > 0", (long long)bad, weights[bad]);
    }
    // the draws queued so far read the table that stands: behind them (the per-batch ones are on the model's stream, in front of
    // the step that records R->busy)
    TRY(wait_queued(h));
    if (!tab.empty()) {
        TRY(h->ptab.ensure(tab.size()));
        HIP_TRY(hipMemcpy(h->ptab.p, tab.data(), tab.size() * sizeof tab[0], hipMemcpyHostToDevice));
    }
    h->h_ptab.swap(tab);
    if (weights) h->h_pw.assign(weights, weights + h->M);
    else h->h_pw.clear();
    return refresh_logq(h);      // (the softmax's log-Q table follows the proposal, include/fmhip_softmax.h)
}

int fmhip_proposal_get(fmhip_bpr_t h, int *weighted) {
    if (!h) return fail(FMHIP_ERR_INVALID, "the BPR trainer is NULL");
    if (!weighted) return fail(FMHIP_ERR_INVALID, "weighted is NULL");
    *weighted = h->h_ptab.empty() ? 0 : 1;
    return FMHIP_OK;
}

int fmhip_proposal_table(fmhip_bpr_t h, uint32_t *thresh, int32_t *alias) {
    if (!h) return fail(FMHIP_ERR_INVALID, "the BPR trainer is NULL");
    if (h->h_ptab.empty()) return fail(FMHIP_ERR_INVALID, "the proposal is uniform: it has no table (fmhip_proposal_set)");
    for (size_t i = 0; i < h->h_ptab.size(); ++i) {
        if (thresh) thresh[i] = h->h_ptab[i].thresh;
        if (alias) alias[i] = h->h_ptab[i].alias;
    }
    return FMHIP_OK;
}

// ---- the sampled softmax (include/fmhip_softmax.h) -------------------------------------------------------------------------------------

int fmhip_softmax_set(fmhip_bpr_t h, int enabled, int logq) {
    if (!h) return fail(FMHIP_ERR_INVALID, "the BPR trainer is NULL");
    if (enabled && h->warp)
        return fail(FMHIP_ERR_INVALID, "fmhip_softmax_set: WARP is on for this trainer (fmhip_warp_set) — its hinge is the step's rule; turn WARP off first");
    if (enabled && splits_interactions(h))
        return fail(FMHIP_ERR_INVALID, "fmhip_softmax_set: batch_pairs = %lld is no multiple of n_neg = %d — a batch would split an interaction's negatives",
                    (long long)h->batch_pairs, (int)h->n_neg);
    TRY(wait_queued(h));      // (the steps queued so far read the table and the probabilities that stand)
    h->softmax = enabled != 0;
    h->sm_logq = logq != 0;
    h->sm_have.assign(h->R->batches.size(), 0);
    return refresh_logq(h);
}

int fmhip_softmax_get(fmhip_bpr_t h, int *enabled, int *logq) {
    if (!h) return fail(FMHIP_ERR_INVALID, "the BPR trainer is NULL");
    if (enabled) *enabled = h->softmax ? 1 : 0;
    if (logq) *logq = h->sm_logq ? 1 : 0;
    return FMHIP_OK;
}

int fmhip_softmax_loss(fmhip_model_t m, fmhip_bpr_t h, double *loss, double *top1, fmhip_stats *stats) {
    ReadLock lock(m);
    if (!h) return fail(FMHIP_ERR_INVALID, "the BPR trainer is NULL");
    if (splits_interactions(h))
        return fail(FMHIP_ERR_INVALID, "fmhip_softmax_loss: batch_pairs = %lld is no multiple of n_neg = %d — a batch splits an interaction's negatives",
                    (long long)h->batch_pairs, (int)h->n_neg);
    double sums[2] = {0.0, 0.0};
    TRY(rel_softmax_score(m, h->R, h->n_neg, logq_in_force(h) ? h->lq.p : nullptr, sums, stats));
    const double inter = (double)h->n_inter;
    if (top1) *top1 = sums[0] / inter;
    if (loss) *loss = sums[1] / inter;
    return FMHIP_OK;
}

int fmhip_softmax_probs(fmhip_bpr_t h, float *out) {
    if (!h) return fail(FMHIP_ERR_INVALID, "the BPR trainer is NULL");
    if (!out) return fail(FMHIP_ERR_INVALID, "out is NULL");
    if (!h->softmax || h->sm_have.empty() || std::find(h->sm_have.begin(), h->sm_have.end(), (char)0) != h->sm_have.end())
        return fail(FMHIP_ERR_INVALID, "fmhip_softmax_probs: no softmax probabilities stand — every batch needs a step since fmhip_softmax_set(h, 1, ..)");
    TRY(wait_queued(h));
    std::vector<float> c((size_t)(2 * h->n_pairs));
    HIP_TRY(hipMemcpy(c.data(), h->sm_pi.p, c.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (int64_t p = 0; p < h->n_pairs; ++p) out[p] = c[(size_t)(2 * p)];
    return FMHIP_OK;
}

int fmhip_softmax_logq(fmhip_bpr_t h, float *out) {
    if (!h) return fail(FMHIP_ERR_INVALID, "the BPR trainer is NULL");
    if (!out) return fail(FMHIP_ERR_INVALID, "out is NULL");
    if (!logq_in_force(h))
        return fail(FMHIP_ERR_INVALID, "fmhip_softmax_logq: the log-Q correction is not in force (it needs the softmax switch, logq and a weighted proposal)");
    std::copy(h->h_lq.begin(), h->h_lq.end(), out);
    return FMHIP_OK;
}

int fmhip_bpr_pair_logloss(fmhip_model_t m, fmhip_bpr_t h, double *logloss, double *concordance, fmhip_stats *stats) {
    ReadLock lock(m);
    if (!h) return fail(FMHIP_ERR_INVALID, "the BPR trainer is NULL");
    if (!logloss) return fail(FMHIP_ERR_INVALID, "logloss is NULL");
    return rel_pair_score(m, h->R, logloss, concordance, stats);
}

int fmhip_bpr_debug_inverse(struct fmhip_bpr *h, int64_t batch, int32_t *trow, int32_t *tptr, int32_t *tj, int32_t *wt, int32_t *wbeg,
                            int32_t *wdst, int32_t *lt, int32_t *lfirst, int32_t *lcount, int32_t *counts) {
    if (!h) return fail(FMHIP_ERR_INVALID, "the BPR trainer is NULL");
    if (batch < 0 || batch >= (int64_t)h->R->batches.size())
        return fail(FMHIP_ERR_INVALID, "batch %lld out of range [0, %zu)", (long long)batch, h->R->batches.size());
    if (!trow || !tptr || !tj || !wt || !wbeg || !wdst || !lt || !lfirst || !lcount || !counts) return fail(FMHIP_ERR_INVALID, "an out array is NULL");
    TRY(set_device(h->device));
    TRY(fresh_counts(h));
    const fmhip_relational::Relation &rel = *h->R->rels[1];
    const RelationInverse::Batch &ib = rel.batches[(size_t)batch];
    const auto back = [](int32_t *dst, const int32_t *src, int64_t n) {
        return n > 0 ? hipMemcpy(dst, src, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost) : hipSuccess;
    };
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(back(trow, rel.trow.p + ib.row_off, h->R->batches[(size_t)batch].rows));
    HIP_TRY(back(tptr, rel.tptr.p + ib.tptr_off, (int64_t)ib.n_touched + 1));
    HIP_TRY(back(tj, rel.tj.p + ib.t_off, ib.n_touched));
    HIP_TRY(back(wt, rel.wt.p + ib.w_off, ib.n_work));
    HIP_TRY(back(wbeg, rel.wbeg.p + ib.w_off, ib.n_work));
    HIP_TRY(back(wdst, rel.wdst.p + ib.w_off, ib.n_work));
    HIP_TRY(back(lt, rel.lt.p + ib.l_off, ib.n_long));
    HIP_TRY(back(lfirst, rel.lfirst.p + ib.l_off, ib.n_long));
    HIP_TRY(back(lcount, rel.lcount.p + ib.l_off, ib.n_long));
    HIP_TRY(back(counts, h->counts.p + 4 * batch, 4));
    return FMHIP_OK;
}

}  // extern "C"
