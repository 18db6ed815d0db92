// fm_afm.h — the kernels of the Attentional Factorization Machine (include/fmhip_afm.h; fm_afm.hip): what a launch is given, and the
// launchers.
// Device layout: V, w, w0 and their accumulators as fm_fwfm.h's (V here is the feature table v).  The model's own part is ONE fp32
// array D of `total` = t Kp + 2 t + Kp floats, t the attention factor:
//   W [t][Kp] | b [t] | h [t] | p [Kp]          (row-major; the slots k .. Kp - 1 of a row of W and of p are 0 and stay 0: S is 0
//                                                there, and so is their gradient)
// A lane of the forward reads its B operand as Kp / 4 consecutive floats of a stored row of W (one dwordx4 at Kp = 16).  ND: AdaGrad's
// accumulators, and a workgroup's partial of the gradient, in the same shape.  All of D is regularised (regd).
// v, w, w0 and the statistics are stepped by fm_fwfm.h's backward and update launches: `b` is what they are given (train_r = 0,
// n_blocks = this forward's block count).
//
// WORKSPACE of a training step beside yhat, e, dz, bsum and part of fm_fwfm.h: gpart [forward blocks][total] floats.
#pragma once
#include "fm_fwfm.h"

namespace fmhip {

constexpr int kAfmBlock = 256;           // threads of a forward workgroup: four waves, one a SIMD, each with rows of its own
constexpr int kAfmWaves = kAfmBlock / 64;
constexpr int kAfmRowsPerBlock = 128;    // data rows per workgroup of k_afm_forward: one partial of the statistics and of D's gradient each
constexpr int kAfmPad = 4;               // floats behind a field's row of S and J in LDS
constexpr int kAfmMaxFactors = 16;       // FMHIP_AFM_MAX_FACTORS
constexpr int kAfmMaxAttention = 64;     // FMHIP_AFM_MAX_ATTENTION

struct AfmArgs {
    FwfmArgs b;                   // the model's vectors, the batch, yhat / e / dz / bsum / part / stats and the rule
    float *D, *ND;                // [total]; ND AdaGrad only
    int32_t k, t, total;          // the factors, the attention factor, t Kp + 2 t + Kp
    float *gpart;                 // [forward blocks][total]
    int32_t n_splits, train_d;    // the forward's block count; 0: the attention part is read and never stepped (gpart is not written)
    int32_t lds_limit;            // the device's LDS bytes a workgroup may ask for (hipDeviceAttributeMaxSharedMemoryPerBlock)
    float regd;
};

constexpr int afm_total(int t, int kp) { return t * kp + 2 * t + kp; }
// the tiles (field i, 16-block jt of j) a row of F fields walks: every jt with 16 jt + 15 > i, for i = 0 .. F - 2
constexpr int afm_tiles(int F) {
    int n = 0;
    for (int i = 0; i + 1 < F; ++i) n += (F - 1) / 16 - (i + 1) / 16 + 1;
    return n;
}
// floats of a wave's LDS region: S [Fp][Kp + pad], a training launch's J in the same shape, one score per M-row of every tile; a
// training launch's region also holds the wave's partial of D's gradient at the end (at most afm_total(64, Kp) floats)
constexpr size_t afm_wave_floats(int Fp, int KP, bool train) {
    const size_t own = (size_t)(train ? 2 : 1) * Fp * (KP + kAfmPad) + 16 * (size_t)afm_tiles(Fp);
    const size_t part = train ? (size_t)afm_total(kAfmMaxAttention, KP) : 0;
    return ((own > part ? own : part) + 3) & ~(size_t)3;
}
// dynamic LDS of a forward workgroup, bytes: 64 fields at Kp = 16 take 20,224 a wave and 80,896 a workgroup when training (15,104
// and 60,416 when scoring); 48 fields (39 rounded up) 13,632 and 54,528.  The kernel's own statics come on top (afm_forward_static)
constexpr size_t afm_forward_lds(int Fp, int KP, bool train) { return kAfmWaves * afm_wave_floats(Fp, KP, train) * sizeof(float); }
constexpr size_t afm_forward_static() { return 2 * kAfmMaxAttention * sizeof(float) + kAfmWaves * 4 * sizeof(double); }

inline int afm_forward_blocks(int64_t rows) { return (int)((rows + kAfmRowsPerBlock - 1) / kAfmRowsPerBlock); }
// train: also e, dz, the statistics' block partials and, with train_d, gpart (a.b.y given)
hipError_t launch_afm_forward(const AfmArgs &a, bool train, hipStream_t s);
hipError_t launch_afm_dupdate(const AfmArgs &a, bool adagrad, hipStream_t s);

}  // namespace fmhip
