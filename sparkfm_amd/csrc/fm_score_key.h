// fm_score_key.h — the order-preserving 32-bit key of an fp32 score, shared by the kernels that RANK predictions
// (fm_topk.hip: the best-K lists; fm_rank.hip: the counts; fm_auc.hip: the sort behind ROC AUC), so that all order scores by
// one rule; and, for the pair kernels, the one expression a pair's score is and the 64-bit order word of (score, candidate row).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fmhip {

// order-preserving key: NaN -> 0, then -Inf < ... < -0 < +0 < ... < +Inf (a caller that wants -0 and +0 to tie adds 0.f first)
__device__ __forceinline__ uint32_t score_key(float s) {
    const uint32_t u = __float_as_uint(s);
    return s != s ? 0u : ((u & 0x80000000u) ? ~u : (u | 0x80000000u));
}
// the score of a key (score_key's inverse on canonical scores; key 0 = NaN)
__device__ __forceinline__ float key_score(uint32_t key) {
    return key == 0u ? __uint_as_float(0x7fc00000u) : __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
}

// the one expression a pair's score is; -0 becomes +0 and every NaN the canonical one, so that key <-> score is a bijection
__device__ __forceinline__ float pair_score(float yc, float bd, float dot) {
    float s = (yc + bd) + dot;
    s += 0.f;
    return s != s ? __uint_as_float(0x7fc00000u) : s;
}
// the order word of (score, candidate row): larger = better — higher score first, lower row first among equals, NaN (key 0)
// below -Inf, the empty slot (0) below everything
__device__ __forceinline__ unsigned long long order_word(float score, uint32_t row) {
    return ((unsigned long long)score_key(score) << 32) | (unsigned long long)(0xffffffffu - row);
}

}  // namespace fmhip
