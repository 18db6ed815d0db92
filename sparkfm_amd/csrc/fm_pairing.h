// fm_pairing.h — launchers of the pairwise-ranking kernels (fm_pairing.hip; internal to libfmhip.so).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fmhip {

// Pairing ADJACENT (enum fmhip_pairing, include/fmhip.h): rows 2j and 2j+1 of a batch are one example and the model's loss is
// applied to their difference — margin d = yhat_2j - yhat_2j+1, target dy = y_2j - y_2j+1,
//     squared  g = d - dy            logistic  g = sigma(d) - [dy > 0]
// and the two rows' residuals are e_2j = g, e_2j+1 = -g.  Everything after the residual is linear in it and stays as it is.
//
// The training forward of a paired model is the kFwdQ forward (P = sv*q, yhat beside it) followed by launch_pair_finish, which
// turns the q rows into the P rows the backward reads: P_r = (sv*q_r) * e_r, with e_r riding in the row the way row_finish
// (fm_forward.hip) leaves it — slot pack_k of a packed row, else the low mantissa bits of the first 32 floats — and e[] beside it.
struct PairArgs {
    float *P;            // [2 * n_pairs][Kp]: in, sv*q; out, (sv*q)*e
    const float *yhat;   // [2 * n_pairs] the rows' predictions
    const float *y;      // [2 * n_pairs] the batch's labels (an even row0: 8-byte aligned)
    float *e;            // [2 * n_pairs] out
    double *bsum;        // [slot_blocks(Kp, n_pairs)][4] per-block {sum e = 0 exactly, sum e^2, rows with a non-finite yhat, 0}
    int32_t n_pairs;
    int32_t pack_k;      // >= 0: packed rows (FwdArgs::pack_k)
    int32_t loss;        // Loss (fm_kernels.h)
    const float *c;      // weighted dataset (fm_weights.h): [2 * n_pairs] the batch's row weights, pair j's = c[2j]; NULL: none
                         // (kPairLossHinge, kPairLossGiven: the pairs' weights / probabilities in the same layout)
    float margin;        // loss == kPairLossHinge: m
};

// A third value of PairArgs::loss, internal to the library (fmhip_model_set_loss does not know it): the WARP step's hinge
// (include/fmhip_warp.h), g = (d < margin) ? -1 : 0 times the pair's weight c[2j] — c is then required.  A NaN d gives g = 0.
constexpr int32_t kPairLossHinge = 2;
// A fourth, as internal: the residual is GIVEN, g = -c[2j] (0 where c[2j] is not > 0, the pair's P rows then exact zeros) — the
// sampled softmax's step (include/fmhip_softmax.h), whose pre-pass (fm_softmax.h) leaves the pairs' probabilities in c.  c is
// required; y and the margin are not read.
constexpr int32_t kPairLossGiven = 3;

// n_partials: the launch's grid (slot_blocks, fm_finish.h) = the number of per-block statistic partials it writes (<= kMaxFwdBlocks)
hipError_t launch_pair_finish(int Kp, const PairArgs &a, hipStream_t s, int *n_partials);

// Scoring of held-out pairs (fmhip_pair_logloss): per-block partials in the layout launch_reduce_blocks(with_logloss) sums,
//     {concordance (1, or 0.5 at d == 0), sum e^2 over both rows with e = +-(sigma(d) - [dy > 0]), rows with a non-finite yhat, log-loss}
// the log-loss of a pair being softplus(-d) if dy > 0, else softplus(d).
hipError_t launch_pair_score(const float *yhat, const float *y, int32_t n_pairs, double *bsum, hipStream_t s, int *n_partials);

}  // namespace fmhip
