// fm_constants.h — layout constants shared by the kernels (fm_kernels.h) and the library's pure host arithmetic
// (fmhip_host.h), among them the dense hot block's page geometry.  No HIP include: fmhip_host.cpp also compiles with plain g++ under AddressSanitizer / UBSan (CPU tests).
#pragma once
#include <stdint.h>

namespace fmhip {

constexpr int kRangeLen = 64;      // == FMHIP_RANGE_LEN
constexpr int kXcds = 8;           // L2 domains of an MI355X (workgroups are dispatched round-robin over them)
constexpr int kXSegs = 9;          // runs of one XCD's range list: up to 8 row bands + the share of the unplaced ranges
constexpr int kRowBands = 16;      // row bands of the band-affine placement: two per XCD, 2 MB of P each at 250k-row batches of Kp = 32
constexpr int kExtend = 16;        // a slot finishes a column that ends this close behind its range
constexpr int kHotT = 16;          // slots of one page of the dense hot block (fp32 per row: one 64-B half line)
// Pages of the dense hot block.  Page 0 (the 16 most frequent features) is dense on BOTH sides: its entries leave the
// CSR and the CSC streams.  Pages 1.. (the next most frequent ones that still pass the density test) are dense on the
// GRADIENT side only: their entries stay in the CSR stream the forward walks (a longer dense prologue costs the forward
// its occupancy — profiles/r02_experiments.md §18) but leave the CSC stream, where every entry costs the backward a P-row
// gather; the MFMA block product (fm_kernels.h) forms their gradient rows in the same pass over P as page 0's.
constexpr int kHotPages = 8;
static_assert(kHotPages * kHotT <= 128, "a slot mask holds 128 bits");
typedef unsigned __int128 slotmask_t;      // one bit per slot of the dense hot block
// The priority a wave of the forward's row walk issues a step's requests at (s_setprio; fm_forward.hip, forward_rows: 1 gains half
// as much at C3, 3 no more than 2: profiles/fwd_phase.md), and the bit of tuning key 0 (FMHIP_TUNE_FORWARD_KERNEL) that turns it off
constexpr int kFwdIssuePrio = 2;
constexpr int kFwdNoIssuePrio = 1;

}  // namespace fmhip
