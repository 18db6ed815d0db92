// fm_score_key.h — the order-preserving 32-bit key of an fp32 score, shared by the kernels that RANK predictions
// (fm_topk.hip: the best-K lists; fm_auc.hip: the sort behind ROC AUC), so that both order scores by one rule.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fmhip {

// order-preserving key: NaN -> 0, then -Inf < ... < -0 < +0 < ... < +Inf (a caller that wants -0 and +0 to tie adds 0.f first)
__device__ __forceinline__ uint32_t score_key(float s) {
    const uint32_t u = __float_as_uint(s);
    return s != s ? 0u : ((u & 0x80000000u) ? ~u : (u | 0x80000000u));
}

}  // namespace fmhip
