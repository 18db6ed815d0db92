// fm_rank.h — launchers of the ranking-evaluation kernels (fm_rank.hip; internal to libfmhip.so).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fm_topk.h"

namespace fmhip {

// The score of n explicit (context row, candidate row) pairs: pc[p] a row of t.Qc / t.yc, pd[p] a row of t.Qd / t.yd.
//   key [n]    (order-preserving key of the score) << 32 | ~pd[p] — the order word of the top-K lists (fm_topk.hip)
//   score [n]  nullable: the score itself, the bits of the pair-score kernel
struct PairListArgs {
    PairTables t;
    const int32_t *pc, *pd;     // [n]
    int64_t n;
    unsigned long long *key;
    float *score;
};
hipError_t launch_pair_list(int Kp, const PairListArgs &a, hipStream_t s);

// One (chunk's queries) x (all candidates) counting sweep.  A QUERY is one (context, relevant row) pair: qctx[q] is its
// context's row in t.Qc / t.yc, tk[q] the order word of its target (launch_pair_list).
struct RankArgs {
    PairTables t;
    const int32_t *qctx;        // [nq]
    const unsigned long long *tk;   // [nq]
    int32_t nq, M;
    int32_t split_len, splits;  // candidates per split (a multiple of kTopkTileD) and their number, as topk_splits(nq, M) says
    int32_t *part;              // [nq][splits]: the candidates of the split whose order word is above tk[q]
};
hipError_t launch_pair_rank(int Kp, const RankArgs &a, hipStream_t s);

// rank[q] = sum over the splits of part[q][.] - #{e in [eptr[qctx[q]], eptr[qctx[q] + 1]) : ekey[e - ebase] > tk[q]}
// (eptr NULL: no exclusions; ekey: the order words of the chunk's (context, excluded row) pairs, launch_pair_list)
hipError_t launch_rank_finish(const int32_t *part, int32_t nq, int32_t splits, const unsigned long long *tk, const int32_t *qctx,
                              const int64_t *eptr, int64_t ebase, const unsigned long long *ekey, int32_t *rank, hipStream_t s);

}  // namespace fmhip
