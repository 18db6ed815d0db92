// fm_ffm.h — the kernels of the field-aware FM (include/fmhip_ffm.h; fm_ffm.hip): what a launch is given, and the launchers.
// Device layout: V[i][f][Kp] fp32 — a feature's row is F * Kp contiguous floats, the slots k .. Kp - 1 of a vector stay 0 — and
// AdaGrad's accumulators NV in the same shape; w [n + 1], w0 [1] with Nw, N0.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fmhip {

constexpr int kFfmRowsPerBlock = 32;     // data rows per workgroup of k_ffm_forward (one block partial of the statistics each)
constexpr int kFfmPartTail = 4;          // floats behind a chunk's F * Kp partial sums: {mask bits 0-31, mask bits 32-63, the w term, 0}
constexpr int kFfmChunkLen = 256;        // == host::kFfmChunk (fmhip_ffm.hip asserts it)

struct FfmArgs {
    // the model
    float *V, *w, *w0;
    float *NV, *Nw, *N0;          // AdaGrad only
    int32_t F, Kp;
    // the batch: its rows (row_ptr, y, yhat, e are the batch's own slices: row 0 is the batch's first row; row_ptr's values index the
    // dataset's entry arrays) ...
    const int64_t *row_ptr;
    const int32_t *col;
    const uint8_t *fld, *run;
    const float *val;
    const float *y;               // NULL: a scoring launch of a dataset without labels
    int32_t rows, max_len;
    // ... and its transpose (the batch's own slices)
    const int32_t *cfeat, *cptr, *chunk0, *chunk_col, *occ_row;
    const uint8_t *occ_pos;
    int32_t n_cols, n_chunks;
    // workspace
    float *yhat, *e;              // [rows]
    double *bsum;                 // [forward blocks][4] {sum e, sum e^2, rows with a non-finite margin, 0}
    int32_t n_blocks;
    float *part;                  // [n_chunks][F * Kp + kFfmPartTail]
    double *stats, *acc;          // [4] {sum e, sum e^2, rows, nonfinite}: the step's, and the epoch's running sums (nullable)
    // the rule
    int32_t acc_reset;            // acc = the step's sums instead of acc += (an epoch's first step)
    int32_t loss, linear;
    float eta, reg0, regw, regv, eps, invb;
};

// blocks of the forward over `rows` rows (also the statistic partials it writes)
inline int ffm_forward_blocks(int64_t rows) { return (int)((rows + kFfmRowsPerBlock - 1) / kFfmRowsPerBlock); }
// train: also e and the block partials (a.y given)
hipError_t launch_ffm_forward(const FfmArgs &a, bool train, hipStream_t s);
hipError_t launch_ffm_backward(const FfmArgs &a, hipStream_t s);
hipError_t launch_ffm_update(const FfmArgs &a, bool adagrad, hipStream_t s);

}  // namespace fmhip
