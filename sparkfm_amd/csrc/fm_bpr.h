// fm_bpr.h — launchers of the BPR trainer's device work (fm_bpr.hip; internal to libfmhip.so): the negative sampler and the
// inverse map of the candidates relation, rebuilt on the device after every resample.  The rule: include/fmhip_bpr.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mcmc_rng.h"

namespace fmhip {

// One thread per pair p of [p0, p1): the context of interaction p / n_neg, a row of [0, M) outside the context's positives
// (rng::negative_row, mcmc_rng.h) into map[2p + 1] — the candidates relation's mapping; map[2p] (the positive) is not touched, and
// nothing of a pair outside the range.  A whole-set draw passes [0, n_pairs); the grid and the partials are sized by the range.
// With `tab` set the row comes from the weighted proposal instead (rng::proposal_row): the kernels take the proposal as a
// compile-time parameter, and the uniform instantiations are the code they were.  The scored samplers' walk draws the same way.
struct BprSampleArgs {
    uint64_t seed;
    uint32_t t;
    int32_t n_pairs, n_neg, M;
    int32_t p0, p1;            // the pairs drawn (a scored sampler's record mode: the pairs written)
    const int32_t *ictx;       // [n_inter] the interactions' contexts, in training order
    const int64_t *pptr;       // [n_ctx + 1]
    const int32_t *prow;       // the contexts' positives, ascending and distinct inside a list
    int32_t *map;              // [2 * n_pairs]
    unsigned long long *part;  // [bpr_sample_blocks(p1 - p0)][2] per-block {attempts, forced pairs}
    unsigned long long *total; // [2] their sums (a second, one-block launch): the caller's slot, one per draw in flight
    const rng::AliasEntry *tab; // [M] the weighted proposal's alias table (include/fmhip_proposal.h), every alias in [0, M); nullptr: uniform
};
int bpr_sample_blocks(int64_t n_pairs);
hipError_t launch_bpr_sample(const BprSampleArgs &a, hipStream_t s);

// The scored samplers' candidate walk (k_bpr_sample_walk).  A group of G = Kp / 4 lanes (8 .. 64) per pair: lane l keeps floats
// 4l .. 4l+3 of the context's q row in registers, the group's lanes draw the pair's n_cand candidate rows side by side (lane l
// candidates l, l + G, ...; rng::negative_row with group0 = c << 4), then candidate by candidate the group gathers the row's q
// slice, multiplies and sums over the group by an xor-shuffle tree — an order Kp alone fixes — and hands row and score to the
// sampler's choice rule, whose lane 0 writes the kept row into map[2p + 1].  Qu / Qi / yqi are what the kFwdQ forwards of the two
// blocks left (rel.Q, rel.yq); floats k .. Kp-1 of the context's slice (the packed slot and the padding) are cleared in registers,
// so the score does not rest on what the tables hold there.  Both modes walk the pairs [s.p0, s.p1) and touch nothing of a pair
// outside them.  Record mode (rec_rows set): every candidate's row and score out, nothing else written, no early stop.
//
// Best of C (the rule: include/fmhip_bpr_adaptive.h) adds nothing to the walk's arguments: it keeps the first strict maximum.
struct BprAdaptiveArgs {
    BprSampleArgs s;           // part: [bpr_adaptive_blocks][3] {attempts, forced, replaced pairs}; total: [3]
    int32_t n_cand;            // 1 .. kBprMaxCand
    int32_t k;                 // the model's factors: floats [k, Kp) of a q row are no factors
    const float *Qu, *Qi;      // [n_ctx][Kp], [M][Kp]
    const float *yqi;          // [M]
    int32_t *rec_rows;         // [(s.p1 - s.p0) * n_cand] or nullptr
    float *rec_scores;         // [(s.p1 - s.p0) * n_cand]
};
constexpr int kBprMaxCand = 64;
int bpr_adaptive_blocks(int Kp, int64_t n_pairs);
hipError_t launch_bpr_sample_adaptive(int Kp, const BprAdaptiveArgs &a, hipStream_t s);

// WARP (the rule: include/fmhip_warp.h) adds the pair's positive (map[2p]), gathered and scored before the walk by the walk's
// code; the kept row is the FIRST candidate whose score is strictly above thr = s+ - margin, N = 1 + its index (0: none,
// candidate 0's row kept).  Lane 0 also writes the pair's weight W[N] to c[2p] and c[2p + 1], and N to trials[p].  A group stops
// scoring at the end of the chunk that holds its first violator.  Record mode: s+ out as well.
struct BprWarpArgs {
    BprAdaptiveArgs a;         // a.s.part: [bpr_adaptive_blocks][2] {violated pairs, sum of N over them}; a.s.total: [2]
    float margin;
    const float *W;            // [n_cand + 1] W[0] = 0, W[n] the weight of a pair whose first violator is candidate n - 1
    float *c;                  // [2 * n_pairs] the pairs' weights, a valid PairArgs::c (fm_pairing.h)
    int32_t *trials;           // [n_pairs] N
    float *rec_pos;            // record mode: [a.s.p1 - a.s.p0] s+
};
hipError_t launch_bpr_sample_warp(int Kp, const BprWarpArgs &a, hipStream_t s);

// The inverse map of ONE batch (fmhip::host::RelationInverse::append_batch, array for array) from the batch's slice of the mapping:
// one radix sort of (block row, batch-local row) words over the bits the two need, the lists read off the sorted words, the work
// list at the cut by scans.  Every output array has the capacity its worst case needs: trow / tj / wt / wbeg / wdst `rows`, tptr
// rows + 1, lt / lfirst / lcount rows / cut + 1; counts[4] = {n_touched, n_work, n_long, n_part}.
struct BprInverseArgs {
    const int32_t *map;        // the batch's `rows` entries, all in [0, block_rows)
    int32_t rows, block_rows, cut;
    int32_t *trow, *tptr, *tj, *wt, *wbeg, *wdst, *lt, *lfirst, *lcount, *counts;
};
// bytes of workspace a batch of up to `rows` rows needs (0 on success in *bytes)
hipError_t bpr_inverse_workspace(int32_t rows, int32_t block_rows, size_t *bytes);
hipError_t launch_bpr_inverse(const BprInverseArgs &a, void *workspace, size_t bytes, hipStream_t s);

}  // namespace fmhip
