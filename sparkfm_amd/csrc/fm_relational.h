// fm_relational.h — launchers of the relational-data kernels (fm_relational.hip; internal to libfmhip.so).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fmhip {

// THE RULE (include/fmhip_relational.h).  Data row r points at block row j_b(r) of every relation b.  After one kFwdQ
// forward per block (q_b rows, yhat_b beside them) and one of the plain part's batch (its q rows in P),
//     Q_r = sum_b q_b[j_b(r)]     yhat_r = w0 + sum_b (yhat_b[j_b(r)] - w0) + sum_{b < b'} <q_b, q_b'>          (k_rel_finish)
//     P_b[j] = sum_{r: j_b(r) = j} e_r Q_r     e_b[j] = sum_{r: j_b(r) = j} e_r                                   (k_rel_gather_sum)
// and the existing backward + fixups over the block's CSC with (P_b, e_b) in place of (P, e) give the block's gradient rows.
constexpr int kRelMax = 8;          // == FMHIP_RELATIONS_MAX
constexpr int kRelSumCut = 256;     // == FMHIP_RELATIONAL_SUM_CUT: a list of more rows is summed in chunks of this many

struct RelFinishArgs {
    const float *Q[kRelMax];       // per relation: [J_b][Kp] q rows (packed slot and padding 0, scales applied)
    const float *yq[kRelMax];      // per relation: [J_b] predictions of the block rows
    const int32_t *map[kRelMax];   // per relation: the mapping, at the batch's first row
    int32_t m;                     // relations
    int32_t has_plain;             // 1: row r of P holds the plain part's q row, yplain[r] its prediction
    const float *w0;
    float *P;                      // [n_rows][Kp]: in, the plain part's q rows; out (training), e*Q with e riding in the row as row_finish leaves it
    const float *yplain;           // [n_rows]
    const float *y;                // [n_rows] the batch's labels
    float *e;                      // [n_rows] out: the residuals (nullable in residual mode)
    float *yhat;                   // [n_rows] out, nullable: the predictions
    double *bsum;                  // [slot_blocks(Kp, n_rows)][4] per-block {sum e, sum e^2, rows with a non-finite yhat, sum of log-losses (residual mode, logistic) else 0}
    int32_t n_rows;
    int32_t pack_k;                // >= 0: packed rows (FwdArgs::pack_k)
    int32_t loss;                  // Loss (fm_kernels.h)
    int32_t q_only;                // 1 (training form only; the BPR trainer): P = Q_r as it is and yhat beside it — no residual, no e, no
                                   // statistics: launch_pair_finish (fm_pairing.h) follows and forms the pairs' from them
};

// n_partials: the launch's grid (slot_blocks, fm_finish.h) = the number of per-block statistic partials it writes (<= kMaxFwdBlocks)
// residual_only: the scoring form — P is read (plain part) and never written
hipError_t launch_rel_finish(int Kp, const RelFinishArgs &a, bool residual_only, hipStream_t s, int *n_partials);

// The segmented sum of one (batch, relation): the slices of fmhip::host::RelationInverse on the device.
struct RelGatherArgs {
    const float *P;                // [rows][Kp] the batch's P rows
    const float *e;                // [rows]
    const int32_t *trow, *tptr, *tj;             // the inverse map
    const int32_t *wt, *wbeg, *wdst;             // work items: touched index, first position in trow, destination (>= 0: block row; < 0: partial row -1-dst)
    int32_t n_work;
    const int32_t *lt, *lfirst, *lcount;         // long lists: touched index, first partial row, partial rows
    int32_t n_long;
    float *Pb;                     // [J_b][Kp] out: touched rows written (the caller zeroed the table), e_b in the packed slot or embedded
    float *eb;                     // [J_b] out
    float *part;                   // [n_part][Kp] chunk sums of the long lists
    float *part_e;                 // [n_part]
    int32_t pack_k;
    // Device-counted form (the BPR trainer's per-batch redraw, include/fmhip_redraw.h): counts = the batch's {n_touched, n_work,
    // n_long, n_part} where the inverse build left them, read by the kernels in n_work's and n_long's place, each clamped to the
    // capacity of the slices the host knows (cap_work, cap_long; cap_part partial rows), so that no count indexes outside a slice.
    // nullptr: n_work and n_long by value, as above
    const int32_t *counts;
    int32_t cap_work, cap_long, cap_part;
};
// two launches: every work item (a slot each, ascending rows, fp32), then the long lists' chunk sums in chunk order.  With counts
// set both kernels are always launched, on the grids of cap_work and cap_long: a zero count leaves at the loop's head
hipError_t launch_rel_gather_sum(int Kp, const RelGatherArgs &a, hipStream_t s);

}  // namespace fmhip
