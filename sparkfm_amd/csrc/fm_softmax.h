// fm_softmax.h — launcher of the sampled-softmax pre-pass (fm_softmax.hip; internal to libfmhip.so; the rule: include/fmhip_softmax.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fmhip {

// One batch of the BPR trainer's pair layout: interaction j holds the n adjacent pairs p = j n + q, rows 2p (the positive, the same
// block rows in all n) and 2p + 1 (negative q).  The pre-pass reads the rows' predictions and leaves, per pair, the softmax
// probability of its negative among {the positive, the interaction's n negatives}; the pairs' finish (fm_pairing.h,
// kPairLossGiven) takes g = -pi from there, so P is still read and written once.
struct SoftmaxArgs {
    const float *yhat;   // [2 * n * n_inter] the rows' predictions
    const int32_t *map;  // [2 * n * n_inter] the candidates relation's mapping of these rows (the log-Q correction: lq != NULL)
    const float *lq;     // [M] log of the proposal's probabilities, or NULL: no correction, map is not read
    float *pi;           // [2 * n * n_inter] out: pi[2p] the pair's probability, a PairArgs::c (pi[2p + 1] is not written); NULL: the
                         // scoring form, which writes the partials alone
    double *bsum;        // [softmax_blocks(n, n_inter)][4] per-block {interactions whose positive is strictly on top, 2 sum pi^2,
                         // rows with a non-finite prediction, sum of the interactions' losses}: the layout of launch_pair_score
    int32_t n_inter;
    int32_t n;           // negatives per interaction, >= 1
};

// the launch's grid = the number of partials it writes (<= kMaxFwdBlocks)
int softmax_blocks(int32_t n, int64_t n_inter);
hipError_t launch_softmax_pre(const SoftmaxArgs &a, hipStream_t s, int *n_partials);

}  // namespace fmhip
