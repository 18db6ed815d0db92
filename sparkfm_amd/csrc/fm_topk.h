// fm_topk.h — launchers of the pair-score / top-K kernels (fm_topk.hip; internal to libfmhip.so).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fmhip {

constexpr int kTopkTileC = 64;        // contexts a workgroup keeps resident (16 per wave)
constexpr int kTopkTileD = 64;        // candidates per LDS tile
constexpr int kTopkMaxSplits = 512;   // candidate splits a context's partial lists may come from (k_topk_merge: 8 heads per lane)

// What every pair kernel reads.  Q tables are what the kFwdQ forward writes ([rows][Kp], packed slot and padding zero, scales
// folded in), y the predictions it writes beside them.
struct PairTables {
    const float *Qc, *yc;       // contexts of the chunk: [B][Kp], [B]
    const float *Qd, *yd;       // candidates: [M][Kp], [M]
    const float *w0;            // [1]
};

// One (context chunk) x (all candidates) product.
struct TopkArgs {
    PairTables t;
    int32_t B, M, K;
    int32_t split_len;          // candidates per split (a multiple of kTopkTileD); grid.y = ceil(M / split_len)
    const int64_t *excl_ptr;    // [B + 1] of the chunk's contexts (offsets into excl), NULL = no exclusions
    const int32_t *excl;
    unsigned long long *part;   // top-K: [B][splits][K] partial lists, best first (key << 32 | ~row; 0 = empty slot)
    float *out;                 // pair scores: out[c * M + d]
};

// splits a launch over `B` contexts and `M` candidates uses (>= 1, <= kTopkMaxSplits) and the candidates per split
int topk_splits(int64_t B, int64_t M, int32_t *split_len);
// the running best-K of every (context, split) -> a.part
hipError_t launch_pair_topk(int Kp, const TopkArgs &a, hipStream_t s);
// every score -> a.out
hipError_t launch_pair_scores(int Kp, const TopkArgs &a, hipStream_t s);
// part [B][splits][K] -> idx [B][K] (candidate rows, -1 = none), score [B][K] (-Inf beside -1)
hipError_t launch_topk_merge(const unsigned long long *part, int32_t B, int32_t splits, int32_t K, int32_t *idx, float *score,
                             hipStream_t s);

}  // namespace fmhip
