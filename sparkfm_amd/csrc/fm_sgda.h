// fm_sgda.h — launchers of the SGDA learner's kernels (fm_sgda.hip; include/fmhip_sgda.h states the rule): the dense SGD update with
// a regulariser per (feature group, factor) that keeps the parameters it replaces, and the step of those regularisers from the
// validation batch's packed gradient.  Internal to libfmhip.so.
#pragma once
#include "fm_kernels.h"

namespace fmhip {

constexpr int kSgdaPartPad = 4;     // a chunk's partial row = Kp floats + {the w sum of unpacked rows, pad, pad, pad}
constexpr int kSgdaSlots = 1;       // a group's row of S = Kp doubles + this many (the w sum of unpacked rows)

struct SgdaArgs {
    float *V, *w, *w0;           // the parameter tables, at scale 1
    float *GV, *Gw, *Gb;         // the packed gradient's rows
    float *scal;                 // ... and its head {sum e, sum e^2, rows, nonfinite}
    int64_t n1;
    int32_t pack_k;              // >= 0: packed rows — slot pack_k of a V row is w_i
    float eta, reg0;
    const int32_t *group;        // [n1] the feature's group
    float *L;                    // [G][Kp] lambda_v of (group, factor); packed rows: slot pack_k holds lambda_w; other pad slots 0
    float *Lw;                   // [G] lambda_w (packed rows too: the copy the w table's update reads)
    float *SV, *Sw;              // shadow tables [n1p][Kp], [n1p]: the parameters before the last update
    // the lambda step: the plan (fmhip_host.h: sgda_group_plan) and what it leaves
    const int32_t *order, *chunk_ptr, *group_chunks;
    int32_t n_chunks, n_groups;
    float *part;                 // [n_chunks][Kp + kSgdaPartPad]
    double *S;                   // [G][Kp + kSgdaSlots]: the sums of the last step, already divided by |C|
    double rate;                 // eta_lambda * eta
};

// theta' = theta - eta*(g/|B| + lambda[group, slot]*theta) over [0, n1) and w0, the old theta into SV / Sw, the gradient rows zeroed
hipError_t launch_sgda_apply(int Kp, const SgdaArgs &a, hipStream_t s);
// one workgroup per chunk of the plan: part[chunk] = sum over its rows, in row order, of theta_old * h (h: the gradient in the
// buffer at the CURRENT parameters, not yet divided by |C|); the rows it reads are zeroed.  n_chunks == 0: nothing is launched
hipError_t launch_sgda_lambda_partials(int Kp, const SgdaArgs &a, hipStream_t s);
// per (group, slot): S = (the group's partials added in chunk order, fp64) / |C|, lambda <- max(0, lambda + rate*S)
hipError_t launch_sgda_lambda_step(int Kp, const SgdaArgs &a, hipStream_t s);

}  // namespace fmhip
