// fm_rank.hip — ranking evaluation: the exact position of given candidate rows in their contexts' complete rankings.
//
// fm_topk.hip forms the [B x Kp] . [Kp x M] product of the pair identity on the exact-f32 MFMA and keeps the best K per context.
// Counting how many candidates beat ONE target is the same sweep with a compare-and-count in place of the list insertion
// (include/fmhip_ranking.h).  The unit of work is a QUERY, one (context, relevant row) pair of the chunk:
//   - k_pair_list scores an explicit list of (context row, candidate row) pairs, 16 per wave: the A rows of the MFMA are the
//     pairs' context q rows, the B columns the pairs' candidate q rows, the steps those of k_pair_topk in the same order, and the
//     pair's dot product is the DIAGONAL of the 16 x 16 block — an element of the block depends on its own A row and B column
//     only, so the bits are those k_pair_topk forms for the pair wherever it meets it.  It runs twice: over the queries'
//     targets (their 64-bit order words tk) and over the chunk's (context, excluded row) pairs;
//   - k_pair_rank walks the candidates as k_pair_topk does, by the same lines (PairTiles, fm_pair_tiles.h: the tile streamed
//     through LDS, the prefetch, the k-permuted layout, the four accumulators): a workgroup of 4 waves owns 64 queries — the A
//     operands gathered through the query -> context index — and one split of the candidates.  Per score the common
//     path is one float compare against the query's target score, held in registers: strictly greater counts, strictly less
//     does not.  Only an equal or NaN score makes its lane form the 64-bit order word and compare it with tk — the target itself
//     (word == tk) is never counted and ties order by row exactly as top-K orders them.  Counts are per-lane int32, summed
//     over the 16 lanes that share a query group at the end and written to part[nq][splits]: no atomics;
//   - k_rank_finish: rank = sum of the splits' counts - #{excluded rows of the query's context whose word is above tk}.
// Exclusions therefore cost one pair score per (context, excluded row) and one compare per (query, excluded row): nothing is
// looked up inside the sweep.  pair_score, key_score and order_word are fm_score_key.h's: one definition for this file and
// fm_topk.hip.
#include "fm_rank.h"
#include "fm_pair_tiles.h"
#include "fm_score_key.h"

namespace fmhip {

namespace {

typedef unsigned long long u64;

constexpr int kThreads = kPairThreads;
constexpr int TC = kTopkTileC, TD = kTopkTileD;

template <int KP>
__global__ __launch_bounds__(kThreads) void k_pair_list(const PairListArgs a) {
    constexpr int S = KP / 4;
    const int l = threadIdx.x & 63, wv = threadIdx.x >> 6, g = l >> 4, c15 = l & 15;
    const int64_t p = ((int64_t)blockIdx.x * (kThreads / 64) + wv) * 16 + c15;       // lane (g, c15) feeds slot 4s + g of pair p
    const bool ok = p < a.n;
    const int32_t c = ok ? a.pc[p] : 0, d = ok ? a.pd[p] : 0;
    const float *qa = a.t.Qc + (size_t)c * KP + g, *qb = a.t.Qd + (size_t)d * KP + g;
    f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < S; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ok ? qa[4 * s] : 0.f, ok ? qb[4 * s] : 0.f, acc, 0, 0, 0);
    // lane (g, c15) holds in acc[i] the block's element (row 4g + i, column c15): the diagonal is on the lanes with c15 / 4 == g
    if (ok && (c15 >> 2) == g) {
        const int i = c15 & 3;
        const float dot = i == 0 ? acc[0] : i == 1 ? acc[1] : i == 2 ? acc[2] : acc[3];
        const float s = pair_score(a.t.yc[c], a.t.yd[d] - *a.t.w0, dot);
        a.key[p] = order_word(s, (uint32_t)d);
        if (a.score) a.score[p] = s;
    }
}

template <int KP>
__global__ __launch_bounds__(kThreads) void k_pair_rank(const RankArgs a) {
    constexpr int S = PairTiles<KP>::S;      // MFMA steps
    constexpr PairTileLds lds = pair_tile_lds(KP);
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x, l = tid & 63, wv = tid >> 6, g = l >> 4, c15 = l & 15;
    const int qw = blockIdx.x * TC + wv * 16;                 // the wave's first query
    const int split = blockIdx.y;
    const int64_t d_lo = (int64_t)split * a.split_len, d_hi = min((int64_t)a.M, d_lo + a.split_len);

    // A operand of step s: Qc[context of query c15 of the wave][4s + g]; queries past the chunk's are zero rows
    float A[S];
    {
        const bool ok = qw + c15 < a.nq;
        const float *q = a.t.Qc + (size_t)(ok ? a.qctx[qw + c15] : 0) * KP + g;
#pragma unroll
        for (int s = 0; s < S; ++s) A[s] = ok ? q[4 * s] : 0.f;
    }
    // the accumulators' rows: queries 4g + i of the wave.  A query past the chunk's counts against a target of 0 and is
    // never written
    float yc[4], ts[4];
    u64 tk[4];
    int32_t cnt[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const bool v = qw + 4 * g + i < a.nq;
        yc[i] = v ? a.t.yc[a.qctx[qw + 4 * g + i]] : 0.f;
        tk[i] = v ? a.tk[qw + 4 * g + i] : 0ull;
        ts[i] = v ? key_score((uint32_t)(tk[i] >> 32)) : 0.f;
        cnt[i] = 0;
    }

    PairTiles<KP> pt{reinterpret_cast<float *>(smem), reinterpret_cast<float *>(smem + lds.tile_bytes), a.t.Qd, a.t.yd, *a.t.w0, d_lo, d_hi,
                     tid, g, c15};
    if (d_lo < d_hi) pt.fetch(d_lo);
    for (int64_t d0 = d_lo; d0 < d_hi; d0 += TD) {
        f32x4 acc[4];
        pt.product(d0, A, acc);

        // lane (g, c15) holds, in acc[j][i], the pair (query 4g + i of the wave, candidate d0 + 16j + c15)
        float bdv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) bdv[j] = pt.bd[16 * j + c15];
        if (d0 + TD <= d_hi) {
            // the common path: one compare per score counts it (the raw sum orders like the canonical score), one more tells
            // whether any score of the lane is equal to its target or NaN; one branch per tile
            bool any = false;
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float r = (yc[i] + bdv[j]) + acc[j][i];
                    cnt[i] += r > ts[i] ? 1 : 0;
                    any |= !(r > ts[i] || r < ts[i]);
                }
            if (!any) continue;
        }
        // rare — a tie with the target, the target itself, a NaN on either side — or the split's last, partial tile: the lane
        // settles what the float compare left open by the order words
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (d0 + 16 * j + c15 >= d_hi) continue;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float r = (yc[i] + bdv[j]) + acc[j][i];
                if (d0 + TD <= d_hi) {
                    if (r > ts[i] || r < ts[i]) continue;      // counted (or not) above
                } else if (r > ts[i]) {
                    ++cnt[i];
                    continue;
                } else if (r < ts[i]) {
                    continue;
                }
                cnt[i] += order_word(pair_score(yc[i], bdv[j], acc[j][i]), (uint32_t)(d0 + 16 * j + c15)) > tk[i] ? 1 : 0;
            }
        }
    }
    // a query's count: the sum over the 16 lanes of its group
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) cnt[i] += __shfl_xor(cnt[i], off, 64);
        const int q = qw + 4 * g + i;
        if (c15 == 0 && q < a.nq) a.part[(size_t)q * a.splits + split] = cnt[i];
    }
}

// one wave per query
__global__ __launch_bounds__(kThreads) void k_rank_finish(const int32_t *part, int32_t nq, int32_t splits, const u64 *tk, const int32_t *qctx,
                                                         const int64_t *eptr, int64_t ebase, const u64 *ekey, int32_t *rank) {
    const int l = threadIdx.x & 63, q = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (q >= nq) return;
    int32_t sum = 0;
    for (int s = l; s < splits; s += 64) sum += part[(size_t)q * splits + s];
    if (eptr) {
        const u64 t = tk[q];
        const int64_t lo = eptr[qctx[q]] - ebase, hi = eptr[qctx[q] + 1] - ebase;
        for (int64_t e = lo + l; e < hi; e += 64) sum -= ekey[e] > t ? 1 : 0;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off, 64);
    if (l == 0) rank[q] = sum;
}

template <int KP>
hipError_t launch_list(const PairListArgs &a, hipStream_t s) {
    const int64_t per = (kThreads / 64) * 16;
    hipLaunchKernelGGL((k_pair_list<KP>), dim3((unsigned)((a.n + per - 1) / per)), dim3(kThreads), 0, s, a);
    return hipGetLastError();
}

template <int KP>
hipError_t launch_rank(const RankArgs &a, hipStream_t s) {
    constexpr size_t lds = pair_tile_lds(KP).tile_bytes + pair_tile_lds(KP).bd_bytes;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_pair_rank<KP>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_pair_rank<KP>), dim3((unsigned)((a.nq + TC - 1) / TC), (unsigned)a.splits), dim3(kThreads), lds, s, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_pair_list(int Kp, const PairListArgs &a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    if (a.n > 0x7fffffffll) return hipErrorInvalidValue;
    switch (Kp) {
        case 32: return launch_list<32>(a, s);
        case 64: return launch_list<64>(a, s);
        case 128: return launch_list<128>(a, s);
        case 256: return launch_list<256>(a, s);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_pair_rank(int Kp, const RankArgs &a, hipStream_t s) {
    if (a.nq <= 0 || a.M <= 0) return hipSuccess;
    if (a.splits < 1 || a.splits > kTopkMaxSplits || a.split_len < TD || a.split_len % TD != 0 ||
        (int64_t)a.splits * a.split_len < a.M)
        return hipErrorInvalidValue;
    switch (Kp) {
        case 32: return launch_rank<32>(a, s);
        case 64: return launch_rank<64>(a, s);
        case 128: return launch_rank<128>(a, s);
        case 256: return launch_rank<256>(a, s);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_rank_finish(const int32_t *part, int32_t nq, int32_t splits, const unsigned long long *tk, const int32_t *qctx,
                              const int64_t *eptr, int64_t ebase, const unsigned long long *ekey, int32_t *rank, hipStream_t s) {
    if (nq <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_rank_finish, dim3((unsigned)((nq + kThreads / 64 - 1) / (kThreads / 64))), dim3(kThreads), 0, s, part, nq, splits, tk,
                       qctx, eptr, ebase, ekey, rank);
    return hipGetLastError();
}

}  // namespace fmhip
