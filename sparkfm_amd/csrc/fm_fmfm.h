// fm_fmfm.h — the kernels of the field-matrixed FM (include/fmhip_fmfm.h; fm_fmfm.hip): what a launch is given, and the launchers.
// Device layout: V, w, w0 and their accumulators as fm_fwfm.h's.  M is ONE symmetric fp32 matrix MM[Pp][Pp], P = F Kp, Pp = P rounded
// up to 16: MM[f Kp + d][g Kp + d'] = M[f][g][d][d'], mirrored; the diagonal blocks and every pad slot are 0 and stay 0.  NM: AdaGrad's
// accumulators in the same shape.  v, w, w0 and the statistics are stepped by fm_fwfm.h's backward and update launches: `b` is what
// they are given (train_r = 0, n_blocks = this forward's block count).
#pragma once
#include "fm_fwfm.h"

namespace fmhip {

constexpr int kFmfmRowsPerBlock = 128;   // data rows per workgroup of k_fmfm_forward: one partial of the statistics each
constexpr int kFmfmPad = 4;              // floats behind a row of S in LDS: lane (g, c) of an MFMA operand read sits at c (Pp + 4) + 4 g
constexpr int kFmfmMaxWidth = 768;       // FMHIP_FMFM_MAX_WIDTH
constexpr int kFmfmGradRows = 256;       // data rows per row split of k_fmfm_mgrad: one partial of M's gradient each
constexpr int kFmfmGradTile = 64;        // its output tile: 64 x 64 elements of MM a workgroup, 32 x 32 a wave
constexpr int kFmfmGradStage = 32;       // ... and the rows it stages through LDS at a time

// The forward's row tile: the largest of 64, 32, 16 rows whose S[rows][Pp] stays inside 48 KB
constexpr int fmfm_row_tile(int pp) { return 64 * pp * 4 <= 49152 ? 64 : (32 * pp * 4 <= 49152 ? 32 : 16); }
constexpr int fmfm_max_pp(int rt) { return 49152 / (4 * rt) > kFmfmMaxWidth ? kFmfmMaxWidth : 49152 / (4 * rt); }
// dynamic LDS of a forward workgroup: S [rt][pp + pad], the waves' pair partials [4][rt], the rows' linear terms [rt], the tile's row
// offsets [rt + 1], then per (row, field) its run's head (the entry's index in the tile, 16 bits) and length (8 bits)
constexpr size_t fmfm_forward_lds(int rt, int pp, int f) { return ((size_t)rt * (pp + kFmfmPad) + 4 * rt + rt + (rt + 1)) * 4 + (size_t)rt * f * 3; }

struct FmfmArgs {
    FwfmArgs b;                   // the model's vectors, the batch, yhat / e / dz / bsum / part / stats and the rule
    float *MM, *NM;               // [Pp][Pp]; NM AdaGrad only
    int32_t k, Pp;
    float *sw;                    // [rows][Pp]: the rows' field sums (written when M is trained)
    float *mpart;                 // [row splits][Pp][Pp]: the tiles on and above the diagonal written, f < g read
    int32_t n_splits, train_m;
    float regm;
};

inline int fmfm_forward_blocks(int64_t rows) { return (int)((rows + kFmfmRowsPerBlock - 1) / kFmfmRowsPerBlock); }
inline int fmfm_grad_splits(int64_t rows) { return (int)((rows + kFmfmGradRows - 1) / kFmfmGradRows); }
// train: also e, dz, the statistics' block partials and, with train_m, sw (a.b.y given)
hipError_t launch_fmfm_forward(const FmfmArgs &a, bool train, hipStream_t s);
hipError_t launch_fmfm_mgrad(const FmfmArgs &a, hipStream_t s);
hipError_t launch_fmfm_mupdate(const FmfmArgs &a, bool adagrad, hipStream_t s);

}  // namespace fmhip
