// fm_auc.h — launchers of the ROC AUC / per-group AUC kernels (fm_auc.hip; internal to libfmhip.so).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fmhip {

// AUC is a rank statistic, an exact integer count (include/fmhip_metrics.h):
//     2 U = sum over (positive, negative) pairs of one group of 2 [yhat_p > yhat_n] + [yhat_p == yhat_n]
// Row r becomes ONE 64-bit word, group << 33 | score_key(yhat + 0.f) << 1 | t with t = [y > 0] (31 + 32 + 1 bits), the words
// are sorted, and everything else is read off the sorted words: a RUN is a stretch of equal (group, score) — its negatives
// come first — and a GROUP a stretch of equal group ids.  With cneg(p) = the negatives before position p,
//     run r = [s, e):     neg_r = cneg(e) - cneg(s), pos_r = (e - s) - neg_r, A_r = pos_r * (2 cneg(s) + neg_r)
//     group g = [s, e):   pos_g, neg_g likewise, 2 U_g = sum of A_r over its runs - 2 cneg(s) pos_g
// in uint64 arithmetic (sums wrap harmlessly; every reported value fits for n < 2^31).

constexpr int kAucScoreShift = 1, kAucGroupShift = 33;

// words[r] = group[r] << 33 | key << 1 | t for r < rows (group NULL: 0); plain pointers, so a batch of a dataset (score = the
// forward's yhat, y = the batch's labels, group = the call's ids + row0, words = the call's array + row0) and a caller's own
// arrays take the same launch
hipError_t launch_auc_keys(const float *score, const float *y, const int32_t *group, int64_t rows, unsigned long long *words,
                           hipStream_t s);

struct AucSums {
    uint64_t u2, pairs;                 // over the scored groups (both classes present)
    uint64_t groups, groups_scored;
    uint64_t rows_scored;               // rows of the scored groups
    uint64_t negatives;                 // over all rows
    double gauc_num;                    // sum over scored groups of rows_g * (2 U_g / (2 pos_g neg_g)), in a fixed order
};

// Sort + runs + groups + sums of the n words (n >= 1; clobbered).  Bits [0, end_bit) of the words are sorted: 33 + the bits
// the largest group id needs.  Allocates its workspace (20 B per row beside the words, plus rocPRIM's temporary storage) for the call, synchronises `s` and frees it.
hipError_t auc_from_words(unsigned long long *words, int64_t n, int end_bit, hipStream_t s, AucSums *out);

}  // namespace fmhip
