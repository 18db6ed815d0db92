// fm_pnn.h — the kernels of the product-based neural network (include/fmhip_pnn.h; fm_pnn.hip): what a launch is given, the Gram
// tiles' table, the forward's LDS budget, and the launchers.
// Device layout: V, w, w0 and their accumulators as fm_fwfm.h's.  The dense part is ONE fp32 array D of `total` floats, in
// fm_deepfm.h's order with a taller W_1:
//   W_1 [n0p][n_1] | W_2 [n_1][n_2] | W_3 [n_2][n_3] | u [n_L] | b_1 [n_1] | b_2 | b_3
// W_1's rows: first the Pp = round16(F Kp) rows of the field sums (row f Kp + d: slot d of field f, as DeepFM's), then the pairs' rows
// GRAM TILE by Gram tile.  The fields come in Fp / 16 blocks of 16; a tile (mt, nt), mt <= nt, is the 16 x 16 block of S S^T of the
// field blocks mt and nt, and its slot il * 16 + jl is the pair (i, j) = (16 mt + il, 16 nt + jl).  A slot with i >= j or j >= F is a
// PAD: its row of W_1 is 0 and stays 0 (h_0 is 0 there, and so is the row's gradient).  A tile stores only its first ns rows il — the
// SLICES of 16 slots that hold a pair at all: 16 off the diagonal, min(F - 16 mt, 16) - 1 on it —, a tile without one is not in the
// table, and the tiles follow one another in ascending (mt, nt).  n0p = Pp + 16 (the slices of all tiles): h_0's width on the device.
// v, w, w0 and the statistics are stepped by fm_fwfm.h's backward and update launches over this forward's dz, e and bsum; the dense
// part's update is fm_deepfm.h's launch_deepfm_dupdate over `d` (it reads D, ND, gpart, total, boff[0], n_splits and the rates).
#pragma once
#include "fm_deepfm.h"

namespace fmhip {

constexpr int kPnnRowsPerBlock = 128;    // data rows per workgroup of k_pnn_forward: one partial of the statistics each
constexpr int kPnnMaxWidth = 1408;       // FMHIP_PNN_MAX_WIDTH: round16(F Kp) + round16(F (F - 1) / 2)
constexpr int kPnnMaxTiles = 10;         // Gram tiles of four field blocks (F <= 49 under the width)
constexpr int kPnnStage = 256;           // slots of a Gram tile: the staging tile's width
constexpr int kPnnStaticLds = 64 * 3 * 8;          // the forward's own __shared__ doubles (the statistics' tree)

struct PnnTiles {
    int32_t n = 0, rows = 0;             // tiles; 16 x their slices together
    int8_t mt[kPnnMaxTiles] = {}, nt[kPnnMaxTiles] = {}, ns[kPnnMaxTiles] = {};
    int16_t off[kPnnMaxTiles] = {};      // the tile's first row behind W_1's Pp field rows
};

// false: more than kPnnMaxTiles tiles (the width refuses such a model long before)
inline bool pnn_tiles(int F, PnnTiles &t) {
    t = PnnTiles();
    const int nb = (F + 15) / 16;
    for (int m = 0; m < nb; ++m)
        for (int n = m; n < nb; ++n) {
            const int left = F - 16 * m < 16 ? F - 16 * m : 16, ns = m == n ? left - 1 : 16;
            if (ns <= 0) continue;
            if (t.n == kPnnMaxTiles) return false;
            t.mt[t.n] = (int8_t)m;
            t.nt[t.n] = (int8_t)n;
            t.ns[t.n] = (int8_t)ns;
            t.off[t.n] = (int16_t)t.rows;
            t.rows += 16 * ns;
            ++t.n;
        }
    return true;
}

struct PnnArgs {
    DeepfmArgs d;                 // DeepFM's, with n[0] = n0p (W_1's height on the device), Pp = the field sums' width and sw [rows][n0p]
    PnnTiles t;
    int32_t lds_limit;            // the device's LDS per workgroup
};

// The forward's LDS tiles, floats per row: X0 [Pp + 4] the field sums; Y [max(n_1, n_3) + 4] h_1, h_3, delta_3, delta_1; Z
// [max(256, n_2) + 4] the staging tile of a Gram tile's products (forward) and of their derivatives (backward), between them h_2 and
// delta_2; a training launch also Jt [Pp + 4].  Then the rows' linear and deep terms 2 [rt] and the tile's row offsets [rt + 1].
inline int pnn_wy(const DeepfmArgs &a) { return deepfm_max(a.n[1], a.L >= 3 ? a.n[3] : 0); }
inline int pnn_wz(const DeepfmArgs &a) { return deepfm_max(kPnnStage, a.L >= 2 ? a.n[2] : 0); }
constexpr size_t pnn_forward_lds(int rt, int pp, int wy, int wz, bool train) {
    return ((size_t)rt * ((train ? 2 : 1) * (pp + kDeepPad) + wy + wz + 2 * kDeepPad + 2) + rt + 1 + 3) / 4 * 16;
}
// the largest of 64, 32, 16 rows whose tiles (and the kernel's own doubles) the device gives a workgroup; 0: not even 16
inline int pnn_row_tile(int pp, int wy, int wz, bool train, int lds_limit) {
    for (int rt = 64; rt >= 16; rt >>= 1)
        if (pnn_forward_lds(rt, pp, wy, wz, train) + kPnnStaticLds <= (size_t)lds_limit) return rt;
    return 0;
}

inline int pnn_forward_blocks(int64_t rows) { return (int)((rows + kPnnRowsPerBlock - 1) / kPnnRowsPerBlock); }
// train: also e, dz, the statistics' block partials, hw and, with train_d, sw and dw (a.d.b.y given)
hipError_t launch_pnn_forward(const PnnArgs &a, bool train, hipStream_t s);
hipError_t launch_pnn_wgrad(const PnnArgs &a, hipStream_t s);

}  // namespace fmhip
