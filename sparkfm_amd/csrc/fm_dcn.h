// fm_dcn.h — the kernels of the low-rank cross network, DCN-V2 (include/fmhip_dcn.h; fm_dcn.hip): what a launch is given, and the
// launchers.
// Device layout: V, w, w0 and their accumulators as fm_fwfm.h's (V here is the feature table v).  The dense part is ONE fp32 array D
// of `total` floats, with P = F Kp, Pp = P rounded up to 16, r the rank:
//   VT_0 [r][Pp] | UT_0 [Pp][r] | VT_1 | UT_1 | VT_2 | UT_2 | u [Pp] | c_0 [Pp] | c_1 | c_2          (row-major, only the L layers the model has)
// VT_l is the header's V_l TRANSPOSED and UT_l its U_l transposed: both products of the forward half, x_l V_l and t_l U_l, then read
// their B operand along a stored row (one global_load_dwordx4 a lane); the backward half reads the same arrays across rows.  Slot
// f Kp + d of Pp belongs to slot d of field f; the columns of VT_l, the rows of UT_l and the elements of c_l and u that belong to pad
// slots (d >= k, and P .. Pp - 1) are 0 and stay 0: their gradient is 0 because x_0, hence every x_l and q_l, is 0 there.  ND: AdaGrad's
// accumulators, and a row split's partial of the gradient, in the same shape.  Everything before c_0 is regularised (regd), c_l is not.
// v, w, w0 and the statistics are stepped by fm_fwfm.h's backward and update launches: `b` is what they are given (train_r = 0,
// n_blocks = this forward's block count).
//
// WORKSPACE of a training step, for the dataset's largest batch of R rows, allocated at the first training step (floats):
//   always:                       pw: L R Pp (p_l)   jw: R Pp when L >= 2 (the running second sum of J)
//   when the dense part trains:   sw: R Pp (x_0)   xw: L R Pp (x_1 .. x_L)   qw: L R Pp (q_l)   tw, mw: L R r each (t_l, m_l)
//                                 gpart: ceil(R / kDcnGradRows) total
//   bytes = 4 (R (L (3 Pp + 2 r) + 2 Pp) + ceil(R / 512) total) at most, beside yhat, e, dz, bsum and part of fm_fwfm.h.
#pragma once
#include "fm_fwfm.h"

namespace fmhip {

constexpr int kDcnRowsPerBlock = 128;    // data rows per workgroup of k_dcn_forward: one partial of the statistics each
constexpr int kDcnPad = 4;               // floats behind a row of an LDS tile: lane (g, c) of an MFMA operand read sits at c (width + 4) + 4 g
constexpr int kDcnMaxWidth = 768;        // FMHIP_DCN_MAX_WIDTH
constexpr int kDcnMaxLayers = 3;         // FMHIP_DCN_MAX_LAYERS
constexpr int kDcnMaxRank = 256;         // FMHIP_DCN_MAX_RANK
constexpr int kDcnGradRows = 512;        // data rows per row split of k_dcn_wgrad: one partial of the dense gradient each
constexpr int kDcnGradTile = 64;         // its output tile: 64 x 64 elements a workgroup, 32 x 32 a wave
constexpr int kDcnGradStage = 32;        // ... and the rows it stages through LDS at a time

struct DcnArgs {
    FwfmArgs b;                   // the model's vectors, the batch, yhat / e / dz / bsum / part / stats and the rule
    float *D, *ND;                // [total]; ND AdaGrad only
    int32_t k, Pp, L, r;
    int32_t voff[kDcnMaxLayers];  // VT_l at D + voff[l]
    int32_t uoff[kDcnMaxLayers];  // UT_l at D + uoff[l]
    int32_t coff[kDcnMaxLayers];  // c_l at D + coff[l]
    int32_t hoff, total;          // u at D + hoff
    float *sw;                    // [rows][Pp]: x_0, the rows' field sums (written when the dense part is trained)
    float *xw[kDcnMaxLayers];     // [rows][Pp]: x_{l+1} (likewise)
    float *qw[kDcnMaxLayers];     // [rows][Pp]: q_l = g_{l+1} o x_0 (likewise)
    float *tw[kDcnMaxLayers];     // [rows][r]: t_l = x_l V_l (likewise)
    float *mw[kDcnMaxLayers];     // [rows][r]: m_l = q_l U_l^T (likewise)
    float *pw[kDcnMaxLayers];     // [rows][Pp]: p_l (written by every training launch: the backward half reads it back)
    float *jw;                    // [rows][Pp]: sum_{l' > l} g_{l'+1} o p_l', carried from layer to layer (L >= 2)
    float *gpart;                 // [row splits][total]
    int32_t n_splits, train_d;
    int32_t lds_limit;            // the device's LDS bytes a workgroup may ask for (hipDeviceAttributeMaxSharedMemoryPerBlock)
    float regd;
};

// dynamic LDS of a forward workgroup: X0 and X [rt][Pp + pad], Tt [rt][r + pad], the rows' linear and cross terms 2 [rt], the tile's
// row offsets [rt + 1]; the kernel's own three doubles a row come on top (dcn_forward_static)
constexpr size_t dcn_forward_lds(int rt, int Pp, int r) { return ((size_t)rt * (2 * (Pp + kDcnPad) + r + kDcnPad + 2) + rt + 1 + 3) / 4 * 16; }
constexpr size_t dcn_forward_static(int rt) { return (size_t)rt * 3 * sizeof(double); }
// the largest of 64, 32, 16 rows whose LDS the device gives one workgroup; 0: not even 16 rows fit (the launch is refused)
inline int dcn_row_tile(int Pp, int r, int lds_limit) {
    for (int rt = 64; rt >= 16; rt >>= 1)
        if (dcn_forward_lds(rt, Pp, r) + dcn_forward_static(rt) <= (size_t)lds_limit) return rt;
    return 0;
}

inline int dcn_forward_blocks(int64_t rows) { return (int)((rows + kDcnRowsPerBlock - 1) / kDcnRowsPerBlock); }
inline int dcn_grad_splits(int64_t rows) { return (int)((rows + kDcnGradRows - 1) / kDcnGradRows); }
// train: also e, dz, the statistics' block partials, pw (and jw) and, with train_d, sw, xw, qw, tw and mw (a.b.y given)
hipError_t launch_dcn_forward(const DcnArgs &a, bool train, hipStream_t s);
hipError_t launch_dcn_wgrad(const DcnArgs &a, hipStream_t s);
hipError_t launch_dcn_dupdate(const DcnArgs &a, bool adagrad, hipStream_t s);

}  // namespace fmhip
