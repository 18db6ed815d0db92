// fm_fwfm.h — the kernels of the field-weighted FM (include/fmhip_fwfm.h; fm_fwfm.hip): what a launch is given, and the launchers.
// Device layout: V[i][Kp] fp32 (the slots k .. Kp - 1 stay 0), w [n + 1], w0 [1], r [F][F] symmetric fp32; AdaGrad's accumulators
// NV, Nw, N0, Nr in the same shapes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fmhip {

constexpr int kFwfmRowsPerBlock = 128;   // data rows per workgroup of k_fwfm_forward: one partial of r's gradient and of the statistics each
constexpr int kFwfmChunkLen = 256;       // == host::kFfmChunk: the dataset's chunks (fmhip_fwfm.hip asserts it)
constexpr int kFwfmPartTail = 4;         // floats behind a chunk's Kp partial sums: {the w term, 0, 0, 0}

// The forward's row tile: Fp = 16 * mt fields (the M tiles of the MFMA), `cols` = rows * Kp columns of S and Z0 in LDS.
constexpr int fwfm_cols(int mt) { return mt == 1 ? 256 : (mt == 2 ? 128 : 64); }
constexpr int fwfm_ld(int mt) { return fwfm_cols(mt) + 16; }          // floats per field row of S and Z0 (the pad: see DESIGN.md)
// dynamic LDS of a forward workgroup: S and Z0 [Fp][ld], three [rows][Fp + 1] per-(row, field) sums, e [rows], the tile's row offsets
// [rows + 1], the row of every entry of the tile [rows * 64] bytes
constexpr size_t fwfm_forward_lds(int mt, int kp) {
    const size_t fp = 16 * (size_t)mt, rt = (size_t)fwfm_cols(mt) / kp;
    return (2 * fp * fwfm_ld(mt) + 3 * rt * (fp + 1) + rt + (rt + 1) + 3) / 4 * 16 + rt * 64;
}
// floats of one workgroup's partial of r's gradient: [Fp][Fp] (the tiles on and above the diagonal written, f < g read), then the
// diagonal's own [Fp]
constexpr int fwfm_rpart(int fp) { return fp * fp + fp; }

struct FwfmArgs {
    // the model
    float *V, *w, *w0, *r;
    float *NV, *Nw, *N0, *Nr;     // AdaGrad only
    int32_t F, Fp, Kp;
    // the batch's rows (row_ptr, y, yhat, e: the batch's own slices; row_ptr's values index the dataset's entry arrays, the batch's
    // first entry is nnz0) ...
    const int64_t *row_ptr;
    const int32_t *col;
    const uint8_t *fld, *run;
    const float *val;
    const float *y;               // NULL: a scoring launch of a dataset without labels
    int64_t nnz0;
    int32_t rows;
    // ... and its transpose (the batch's own slices)
    const int32_t *cfeat, *cptr, *chunk0, *chunk_col, *occ_row;
    const uint8_t *occ_pos;
    int32_t n_cols, n_chunks;
    // workspace
    float *yhat, *e;              // [rows]
    float *dz;                    // [batch entries][Kp]: x_a D_a at the entry's place
    double *bsum;                 // [forward blocks][4] {sum e, sum e^2, rows with a non-finite margin, 0}
    float *rpart;                 // [forward blocks][fwfm_rpart(Fp)]
    int32_t n_blocks;
    float *part;                  // [n_chunks][Kp + kFwfmPartTail]: the chunks of the columns that have more than one
    double *stats, *acc;          // as FfmArgs'
    // the rule
    int32_t acc_reset, loss, linear, train_r;
    float eta, reg0, regw, regv, regr, eps, invb;
};

inline int fwfm_forward_blocks(int64_t rows) { return (int)((rows + kFwfmRowsPerBlock - 1) / kFwfmRowsPerBlock); }
// train: also e, dz and the block partials (a.y given)
hipError_t launch_fwfm_forward(const FwfmArgs &a, bool train, hipStream_t s);
hipError_t launch_fwfm_backward(const FwfmArgs &a, bool adagrad, hipStream_t s);
hipError_t launch_fwfm_update(const FwfmArgs &a, bool adagrad, hipStream_t s);

}  // namespace fmhip
