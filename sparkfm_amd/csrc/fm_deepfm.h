// fm_deepfm.h — the kernels of DeepFM (include/fmhip_deepfm.h; fm_deepfm.hip): what a launch is given, and the launchers.
// Device layout: V, w, w0 and their accumulators as fm_fwfm.h's.  The dense part is ONE fp32 array D of `total` floats:
//   W_1 [Pp][n_1] | W_2 [n_1][n_2] | W_3 [n_2][n_3] | u [n_L] | b_1 [n_1] | b_2 | b_3          (row-major, only the L layers the model has)
// P = F Kp, Pp = P rounded up to 16; row f Kp + d of W_1 belongs to slot d of field f, the rows of the pad slots d >= k and the rows
// P .. Pp - 1 are 0 and stay 0 (their gradient is 0: the field sums' pad slots are).  ND: AdaGrad's accumulators, and a row split's
// partial of the gradient, in the same shape.  Everything before b_1 is regularised (regd), the biases are not.
// v, w, w0 and the statistics are stepped by fm_fwfm.h's backward and update launches: `b` is what they are given (train_r = 0,
// n_blocks = this forward's block count).
#pragma once
#include "fm_fwfm.h"

namespace fmhip {

constexpr int kDeepRowsPerBlock = 128;   // data rows per workgroup of k_deepfm_forward: one partial of the statistics each
constexpr int kDeepPad = 4;              // floats behind a row of an LDS tile: lane (g, c) of an MFMA operand read sits at c (width + 4) + 4 g
constexpr int kDeepMaxWidth = 768;       // FMHIP_DEEPFM_MAX_WIDTH
constexpr int kDeepMaxLayers = 3;        // FMHIP_DEEPFM_MAX_LAYERS
constexpr int kDeepMaxUnits = 256;       // FMHIP_DEEPFM_MAX_UNITS
constexpr int kDeepGradRows = 512;       // data rows per row split of k_deepfm_wgrad: one partial of the dense gradient each
constexpr int kDeepGradTile = 64;        // its output tile: 64 x 64 elements of a W_l a workgroup, 32 x 32 a wave
constexpr int kDeepGradStage = 32;       // ... and the rows it stages through LDS at a time
constexpr int kDeepLdsBudget = 65536;    // the forward's row tile is the largest whose LDS stays inside this; 16 rows otherwise

struct DeepfmArgs {
    FwfmArgs b;                   // the model's vectors, the batch, yhat / e / dz / bsum / part / stats and the rule
    float *D, *ND;                // [total]; ND AdaGrad only
    int32_t k, Pp, L;
    int32_t n[kDeepMaxLayers + 1];            // n[0] = Pp, n[l] = the width of layer l
    int32_t woff[kDeepMaxLayers];             // W_l at D + woff[l - 1]
    int32_t boff[kDeepMaxLayers];             // b_l at D + boff[l - 1]
    int32_t uoff, total;
    float *sw;                    // [rows][Pp]: the rows' field sums h_0 (written when the dense part is trained)
    float *hw[kDeepMaxLayers];    // [rows][n_l]: h_l (written by every training launch: the backward half reads its masks from it)
    float *dw[kDeepMaxLayers];    // [rows][n_l]: delta_l = d yhat / d (layer l's pre-activation) (written when the dense part is trained)
    float *gpart;                 // [row splits][total]
    int32_t n_splits, train_d;
    float regd;
};

constexpr int deepfm_max(int a, int b) { return a > b ? a : b; }
// The forward's two LDS tiles: X holds h_0 (the field sums), h_2, delta_2 and J, Y holds h_1, h_3, delta_3 and delta_1
inline int deepfm_wx(const DeepfmArgs &a) { return deepfm_max(a.Pp, a.L >= 2 ? a.n[2] : 0); }
inline int deepfm_wy(const DeepfmArgs &a) { return deepfm_max(a.n[1], a.L >= 3 ? a.n[3] : 0); }
// dynamic LDS of a forward workgroup: X [rt][wx + pad], Y [rt][wy + pad], T [rt][kp] (the rows' sums over all entries), the rows'
// linear, pair and deep terms 3 [rt], the tile's row offsets [rt + 1]
constexpr size_t deepfm_forward_lds(int rt, int wx, int wy, int kp) { return ((size_t)rt * (wx + wy + 2 * kDeepPad + kp + 3) + rt + 1 + 3) / 4 * 16; }
// the largest of 64, 32, 16 rows inside the budget (the kernel's own three doubles a row included); 16 rows when none is: F Kp above
// ~680 under a layer of 256 units takes up to 66 KB, which the device's LDS (160 KB a CU on gfx950) holds twice over
inline int deepfm_row_tile(int wx, int wy, int kp) {
    for (int rt = 64; rt > 16; rt >>= 1)
        if (deepfm_forward_lds(rt, wx, wy, kp) + (size_t)rt * 3 * sizeof(double) <= (size_t)kDeepLdsBudget) return rt;
    return 16;
}

inline int deepfm_forward_blocks(int64_t rows) { return (int)((rows + kDeepRowsPerBlock - 1) / kDeepRowsPerBlock); }
inline int deepfm_grad_splits(int64_t rows) { return (int)((rows + kDeepGradRows - 1) / kDeepGradRows); }
// train: also e, dz, the statistics' block partials, hw and, with train_d, sw and dw (a.b.y given)
hipError_t launch_deepfm_forward(const DeepfmArgs &a, bool train, hipStream_t s);
hipError_t launch_deepfm_wgrad(const DeepfmArgs &a, hipStream_t s);
hipError_t launch_deepfm_dupdate(const DeepfmArgs &a, bool adagrad, hipStream_t s);

}  // namespace fmhip
