// fm_weights.h — launchers of the per-row example-weight kernels (fm_weights.hip; internal to libfmhip.so).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fmhip {

// THE RULE (include/fmhip_weights.h).  A dataset may carry one weight c_r >= 0 per row.  For a weighted
// dataset every training path forms
//     e_r <- c_r * e_r(loss)      g_theta = sum_{r in batch} e_r h_r(theta)      theta <- theta - eta (g_theta / |batch| + lambda theta)
// the gradient of (1 / |batch|) sum_r c_r l_r.  |batch| stays the ROW count (not sum c): c == 1 is the unweighted rule and a
// data-parallel step needs no new collective.  Under pairing ADJACENT the pair's weight is row 2j's (k_pair_finish, fm_pairing.hip).
// A weight changes the residual and nothing else: everything after the forward sees only e.
//
// The training forward of a weighted dataset is the kFwdQ forward (P = sv*q, yhat beside it) followed by launch_weight_finish
// (single rows) or launch_pair_finish with PairArgs::c (pairs); the single-launch forward instances are not touched, and a
// dataset without weights takes exactly the path it always took.
struct WeightArgs {
    float *P;            // [n_rows][Kp]: in, sv*q; out, (sv*q) * (c e) with e riding in the row as row_finish leaves it
    const float *yhat;   // [n_rows] the rows' predictions
    const float *y;      // [n_rows] the batch's labels
    const float *c;      // [n_rows] the batch's weights (finite, >= 0: validated when the dataset was built)
    float *e;            // [n_rows] out: c_r * e_r(loss); +0 for a row of weight 0
    double *bsum;        // [slot_blocks(Kp, n_rows)][4] per-block {sum e, sum e^2, rows with a non-finite yhat, 0}
    int32_t n_rows;
    int32_t pack_k;      // >= 0: packed rows (FwdArgs::pack_k)
    int32_t loss;        // Loss (fm_kernels.h)
};

// n_partials: the launch's grid (slot_blocks, fm_finish.h) = the number of per-block statistic partials it writes (<= kMaxFwdBlocks)
hipError_t launch_weight_finish(int Kp, const WeightArgs &a, hipStream_t s, int *n_partials);

// Weighted scores (fmhip_weighted_scores) behind a residual-mode forward that left the predictions in yhat: per-block partials in
// the layout launch_reduce_blocks(with_logloss) sums,
//     {sum c, sum c (yhat - y)^2, sum c |yhat - y|, sum c l}     l = softplus(yhat) - [y > 0] yhat, the log-loss of fmhip_logloss
// every term in fp64; a row of weight 0 adds nothing, whatever its prediction.
int weighted_score_blocks(int64_t n_rows);
hipError_t launch_weighted_score(const float *yhat, const float *y, const float *c, int32_t n_rows, double *bsum, hipStream_t s, int *n_partials);

}  // namespace fmhip
