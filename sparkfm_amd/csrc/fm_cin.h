// fm_cin.h — the kernels of xDeepFM's Compressed Interaction Network (include/fmhip_cin.h; fm_cin.hip): what a launch is given, and the
// launchers.
// Device layout: V, w, w0 and their accumulators as fm_fwfm.h's (V here is the feature table v).  The model's own part is ONE fp32
// array D of `total` floats, with Fp = F rounded up to 16, H_0 = F and hp_l the stored H_{l-1} (Fp for l = 1, H_{l-1} above):
//   W_1 [H_1][Fp][Fp] | W_2 [H_2][H_1][Fp] | W_3 [H_3][H_2][Fp] | u [H_1 + .. + H_L]          (row-major, only the L layers the model has)
// W_l[h][i][.] keeps its Fp floats in MFMA order: position 16 t + 4 g + s holds field j = 16 t + 4 s + g, so that lane group g of a
// matrix instruction reads the B operand of four consecutive steps (s = 0 .. 3, fields 16 t + 4 s + {0 .. 3}) as one dwordx4 along
// a stored row, and a step covers four CONSECUTIVE fields: the steps at or above F are skipped, whatever Fp is.  The elements of W_1
// with i >= F and of every W_l at a position whose field is >= F are 0 and stay 0: X^0 is 0 there, and so is their gradient.  ND:
// AdaGrad's accumulators, and a row split's partial of the gradient, in the same shape.  All of D is regularised (regd).
// v, w, w0 and the statistics are stepped by fm_fwfm.h's backward and update launches: `b` is what they are given (train_r = 0,
// n_blocks = this forward's block count).
//
// An M-ROW is a pair (data row, factor d < k): row r's are r k .. r k + k - 1 — no M-row is spent on a pad factor.
//
// WORKSPACE of a training step, for the dataset's largest batch of R rows, allocated at the first training step (floats), all of it
// only when the CIN part trains:
//   xw[0]: R k Fp (X^0, fields in natural order)   xw[l]: R k H_l (X^l, l = 1 .. L-1)   gw[l-1]: R k H_l (G^l, l = 1 .. L)
//   pw: R (H_1 + .. + H_L) (p^l)   gpart: ceil(R / kCinGradRows) total
//   bytes = 4 (R (k (Fp + 2 sum H - H_L) + sum H) + ceil(R / 512) total), beside yhat, e, dz, bsum and part of fm_fwfm.h.
#pragma once
#include "fm_fwfm.h"

namespace fmhip {

constexpr int kCinBlock = 512;           // threads of a forward workgroup: eight waves, two a SIMD
constexpr int kCinWaves = kCinBlock / 64;
constexpr int kCinRowsPerBlock = 128;    // data rows per workgroup of k_cin_forward: one partial of the statistics each
constexpr int kCinMaxTile = 64;          // the largest row tile
constexpr int kCinPad = 4;               // floats behind a row of an LDS tile
constexpr int kCinMaxFactors = 16;       // FMHIP_CIN_MAX_FACTORS
constexpr int kCinMaxLayers = 3;         // FMHIP_CIN_MAX_LAYERS
constexpr int kCinMaxMaps = 128;         // FMHIP_CIN_MAX_MAPS
constexpr int kCinGradRows = 512;        // data rows per row split of k_cin_wgrad: one partial of the dense gradient each
constexpr int kCinGradStage = 32;        // M-rows it stages through LDS at a time

struct CinArgs {
    FwfmArgs b;                   // the model's vectors, the batch, yhat / e / dz / bsum / part / stats and the rule
    float *D, *ND;                // [total]; ND AdaGrad only
    int32_t k, Fp, L;
    int32_t H[kCinMaxLayers + 1]; // H[l] = H_l, l = 1 .. L (H[0] = F)
    int32_t woff[kCinMaxLayers];  // W_l at D + woff[l - 1]
    int32_t uoff, total;          // u at D + uoff
    float *xw[kCinMaxLayers];     // [rows k][Fp], then [rows k][H_l]: X^0 .. X^{L-1} (written when the CIN part is trained)
    float *gw[kCinMaxLayers];     // [rows k][H_l]: G^1 .. G^L (likewise)
    float *pw;                    // [rows][sum H]: p^1 .. p^L (likewise)
    float *gpart;                 // [row splits][total]
    int32_t n_splits, train_d;
    int32_t lds_limit;            // the device's LDS bytes a workgroup may ask for (hipDeviceAttributeMaxSharedMemoryPerBlock)
    int32_t rt;                   // the row tile (the launcher's)
    float regd;
};

constexpr int cin_round16(int x) { return (x + 15) / 16 * 16; }
// the stored H_{l-1} of W_l, and the i the products walk (X^0's rows up to F rounded up to 4: the loop goes four i at a time)
inline __host__ __device__ int cin_hp(const CinArgs &a, int l) { return l == 1 ? a.Fp : a.H[l - 1]; }
inline __host__ __device__ int cin_ni(const CinArgs &a, int l) { return l == 1 ? (a.b.F + 3) / 4 * 4 : a.H[l - 1]; }
inline __host__ __device__ int cin_hsum(const CinArgs &a) { return a.total - a.uoff; }
// the i splits of the backward half: with fewer M tiles than waves, S waves share an M tile and leave S partials of J
constexpr int cin_splits(int tm) { return tm < kCinWaves ? kCinWaves / tm : 1; }

// dynamic LDS of a forward workgroup at a tile of rt rows, Mp = rt k rounded up to 16 M-rows: X^0 [Mp][Fp + pad], X^l [Mp][H_l + pad]
// for l = 1 .. L-1, one buffer [Mp][hmax + pad] for X^L (hmax: the widest of Fp and the H_l), the rows' linear and CIN terms 2 [rt],
// the tile's row offsets [rt + 1]; a training launch adds the second buffer of the G^l and the S partials of J [S][Mp][Fp + pad].
// The kernel's own three doubles a row come on top (cin_forward_static)
inline size_t cin_forward_lds(int rt, int k, int Fp, int L, const int32_t *H, bool train) {
    const size_t Mp = (size_t)cin_round16(rt * k);
    int hmax = Fp;
    size_t per = (size_t)Fp + kCinPad;
    for (int l = 1; l <= L; ++l) {
        hmax = H[l] > hmax ? H[l] : hmax;
        if (l < L) per += (size_t)H[l] + kCinPad;
    }
    per += (size_t)(train ? 2 : 1) * (hmax + kCinPad);
    if (train) per += (size_t)cin_splits((int)Mp / 16) * (Fp + kCinPad);
    return (Mp * per + 3 * (size_t)rt + 1 + 3) / 4 * 16;
}
constexpr size_t cin_forward_static() { return (size_t)kCinMaxTile * 3 * sizeof(double); }
// the largest of 64, 32, .. 1 rows whose LDS the device gives one workgroup; 0: not even one row fits (the launch is refused)
inline int cin_row_tile(int k, int Fp, int L, const int32_t *H, bool train, int lds_limit) {
    for (int rt = kCinMaxTile; rt >= 1; rt >>= 1)
        if (cin_forward_lds(rt, k, Fp, L, H, train) + cin_forward_static() <= (size_t)lds_limit) return rt;
    return 0;
}

inline int cin_forward_blocks(int64_t rows) { return (int)((rows + kCinRowsPerBlock - 1) / kCinRowsPerBlock); }
inline int cin_grad_splits(int64_t rows) { return (int)((rows + kCinGradRows - 1) / kCinGradRows); }
// train: also e, dz, the statistics' block partials and, with train_d, xw, gw and pw (a.b.y given)
hipError_t launch_cin_forward(const CinArgs &a, bool train, hipStream_t s);
hipError_t launch_cin_wgrad(const CinArgs &a, hipStream_t s);
hipError_t launch_cin_dupdate(const CinArgs &a, bool adagrad, hipStream_t s);

}  // namespace fmhip
