// fm_autoint.h — the kernels of AutoInt, multi-head self-attention over the field sums (include/fmhip_autoint.h; fm_autoint.hip): what
// a launch is given, and the launchers.
// Device layout: V, w, w0 and their accumulators as fm_fwfm.h's (V here is the feature table v).  The dense part is ONE fp32 array D of
// `total` floats, with A = H d the layers' width:
//   WT_0 [4A][16] | WT_1 [4A][A] | WT_2 [4A][A] | u [F][A]                    (row-major, only the L layers the model has)
// WT_l is the header's W_l = [W_Q | W_K | W_V | W_R] TRANSPOSED: row n of it is column n of W_l, so the projection X_l W_l reads its B
// operand along a stored row (one global_load_dwordx4 a lane) and the backward product [dQ|dK|dV|Gz] W_l^T reads the same array across
// rows.  WT_0's rows are padded from k to kAutoIntD0 = 16 floats, whatever Kp is: one 16-wide reduction slice serves every Kp.  The
// columns d >= k of WT_0 are 0 and stay 0: their gradient is 0 because X_0 is 0 there.  u needs no pad: A is a multiple of 16 and only
// the F real tokens reach yhat.  ND: AdaGrad's accumulators, and a workgroup's partial of the gradient, in the same shape.  Every element
// of D is regularised (regd).
// v, w, w0 and the statistics are stepped by fm_fwfm.h's backward and update launches: `b` is what they are given (train_r = 0,
// n_blocks = this forward's block count).
//
// WORKSPACE of a training step beside yhat, e, dz, bsum and part of fm_fwfm.h, NONE of it with a slot per batch row (floats; G = the
// forward's workgroups for the dataset's largest batch):
//   scratch: G (L - 1) Fp 3A   a workgroup's own Q, K, V of the layers 0 .. L - 2 of the ONE row it is at (the last layer's stay in LDS)
//   gpart:   G total           a workgroup's partial of the dense gradient, written once
#pragma once
#include "fm_fwfm.h"

namespace fmhip {

constexpr int kAutoIntRowsPerBlock = 128;   // data rows per workgroup of k_autoint_forward: one partial of the dense gradient and of the statistics each
constexpr int kAutoIntPad = 4;              // floats behind a row of an LDS tile, as fm_dcn.h's kDcnPad
constexpr int kAutoIntD0 = 16;              // the width X_0 and WT_0 are padded to
constexpr int kAutoIntMaxLayers = 3;        // FMHIP_AUTOINT_MAX_LAYERS
constexpr int kAutoIntMaxHeads = 4;         // FMHIP_AUTOINT_MAX_HEADS
constexpr int kAutoIntMaxHeadDim = 32;      // FMHIP_AUTOINT_MAX_HEAD_DIM
constexpr int kAutoIntMaxWidth = 64;        // FMHIP_AUTOINT_MAX_WIDTH
constexpr int kAutoIntMaxFactors = 16;      // FMHIP_AUTOINT_MAX_FACTORS
constexpr int kAutoIntSmall = 16;           // floats behind the tiles: the waves' partials of <vec(X_L), u>, the linear term, e

struct AutoIntArgs {
    FwfmArgs b;                   // the model's vectors, the batch, yhat / e / dz / bsum / part / stats and the rule
    float *D, *ND;                // [total]; ND AdaGrad only
    int32_t k, L, H, d, A;
    int32_t woff[kAutoIntMaxLayers];          // WT_l at D + woff[l]
    int32_t hoff, total;          // u at D + hoff
    float *scratch;               // [forward blocks][(L - 1) Fp 3A] (a training launch of a model of two or three layers)
    float *gpart;                 // [forward blocks][total]
    int32_t n_splits, train_d;    // n_splits: the forward's block count
    float regd;
};

// dynamic LDS of a forward workgroup, the ONE row it is at: X_0 [Fp][16 + pad], X_1 .. X_L [Fp][A + pad] each, the projections
// [Q | K | V | R] [Fp][4A + pad] (backwards: [dQ | dK | dV | Gz]), the probabilities of ONE head P [Fp][Fp + pad] and, backwards, their
// score gradients dSc in a second tile of the same shape, then kAutoIntSmall floats.  W_l is NOT held in LDS: it is streamed from L2.
// A scoring launch (train = false) needs neither dSc nor every X_l: it keeps X_l, l >= 1, in two tiles by turns.
constexpr int autoint_x_tiles(int L, bool train) { return train || L < 2 ? L : 2; }
constexpr size_t autoint_forward_lds(int Fp, int A, int L, bool train) {
    return 4 * ((size_t)Fp * (kAutoIntD0 + kAutoIntPad) + (size_t)autoint_x_tiles(L, train) * Fp * (A + kAutoIntPad) +
                (size_t)Fp * (4 * A + kAutoIntPad) + (train ? 2 : 1) * (size_t)Fp * (Fp + kAutoIntPad) + kAutoIntSmall);
}
// floats of one workgroup's scratch
constexpr size_t autoint_scratch(int Fp, int A, int L) { return (size_t)(L - 1) * Fp * 3 * A; }

inline int autoint_forward_blocks(int64_t rows) { return (int)((rows + kAutoIntRowsPerBlock - 1) / kAutoIntRowsPerBlock); }
// train: also e, dz, the statistics' block partials and, with train_d, gpart (a.b.y given)
hipError_t launch_autoint_forward(const AutoIntArgs &a, bool train, hipStream_t s);
hipError_t launch_autoint_dupdate(const AutoIntArgs &a, bool adagrad, hipStream_t s);

}  // namespace fmhip
