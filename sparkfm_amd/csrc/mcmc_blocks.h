// mcmc_blocks.h — launchers of the MCMC learner's block-structure sweep (include/fmhip_mcmc_relational.h; internal to libfmhip.so).
// The kernels sit in als_kernels.hip beside the flat column walk, whose step (DrawMcmc), sums (wave_sum, block_sum2, theta_sums),
// walk choice and per-group pass (group_pass: the plain part) they share; the existing instantiations keep their arguments and
// their code.  The parts' noise and the test rows' accumulation are als_kernels.h's launch_mcmc_noise / launch_mcmc_accumulate_link.
#pragma once
#include "als_kernels.h"

namespace fmhip {

constexpr int kBlockPartsMax = 9;       // FMHIP_RELATIONS_MAX relations + the plain part
constexpr int kBlockCaches = 6;         // E, A, B, C, S1, S2 (the w pass: E and, in S2's place, D)

// One relation of the train set on the device.  a: the BLOCK's rows and columns with a.e = yhat_p [J] (k_als_residual over labels
// of zero), a.q = q_p [k][J] (k_als_q_all), a.y = J zeros.
struct BlockPart {
    AlsArgs a;
    int64_t J;                           // block rows
    int64_t n_rows;                      // data rows
    const int32_t *map;                  // [n_rows] j_p(r)
    const int32_t *trained;              // [a.n_cols] 1: the column is in T (id < num_attribute, an entry in a referenced block row)
    const double *n;                     // [J] n_p[j], the data rows that map to block row j
    // the handle's inverse map (fmhip::host::RelationInverse) of the one batch
    const int32_t *trow, *tptr, *tj, *wt, *wbeg, *wdst;
    int32_t n_work;
    const int32_t *lt, *lfirst, *lcount;
    int32_t n_long;
    double *cache;                       // [kBlockCaches][J]
    double *part;                        // [n_part][4] chunk sums of the long lists
    double *qrest;                       // [n_rows] q_r = Q_f[r] - q_p[j_p(r)] of the factor in hand
};

// The fp64 relational residual of every data row: parts p = 0 .. n_parts - 1 in the order GIVEN (relations, then the plain part)
struct BlockCombine {
    int32_t n_parts, k;
    int64_t n_rows;
    const double *yhat[kBlockPartsMax];  // [J_p]
    const double *q[kBlockPartsMax];     // [k][J_p]
    const int32_t *map[kBlockPartsMax];  // [n_rows]; NULL: the identity (the plain part)
    int64_t J[kBlockPartsMax];
    const double *w0;
    const double *y;                     // [n_rows] targets (the probit form: written through McmcProbit.ystar, which this points at)
    double *e;                           // [n_rows] out
    double *Q;                           // [k][n_rows] out, nullable
};

// The host's view of a block's columns: what the walk's launch plan follows, and a copy of BlockPart.trained
struct BlockPlan : ColumnPlan {
    const int32_t *h_trained;
};

// yhat_p of every block row (a.e) and, with_q, q_p (a.q: it depends on v alone, so the pass behind the bias step leaves it out)
hipError_t launch_block_forward(const AlsArgs &a, bool with_q, hipStream_t s);
hipError_t launch_block_combine(const BlockCombine &c, const McmcProbit *probit, uint64_t seed, uint32_t t, hipStream_t s);
// sums[2 * c] (c < kMcmcSumParts): partial sums of e^2 over rows.n_rows data rows
hipError_t launch_block_sse(const AlsArgs &rows, double *sums, hipStream_t s);
// out[2 * (g * kMcmcSumParts + c)], + 1: chunk c's {sum theta, sum (theta - mu_g)^2} over the part's trained columns, g = 0 .. k
hipError_t launch_block_theta_sums(const AlsArgs &a, const int32_t *trained, const double *hyp, double *out, hipStream_t s);
// the bias draw over rows.e (rows: k, n_rows, e, w0, reg0 and n_cols = 0; m.z: the bias's noise)
hipError_t launch_block_bias(const AlsArgs &rows, const McmcDev &m, hipStream_t s);
// One part's pass of parameter group g (0: w; 1 + f: factor f): cache build, the column walk, the scatter into e and Q_f
hipError_t launch_block_pass(const BlockPart &b, const BlockPlan &plan, int g, double *e, double *Q, const McmcDev &m, hipStream_t s);
// ... and the plain part's: the flat walk's per-group pass over e and Q_f directly (a.e = e, a.q = Q)
hipError_t launch_plain_pass(const AlsArgs &a, int g, const McmcDev &m, const ColumnPlan &plan, hipStream_t s);

}  // namespace fmhip
