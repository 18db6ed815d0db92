// fm_topk.hip — top-K recommendation: the scores of (context row) x (candidate row) pairs and the best K per context.
//
// The FM score of the joined row "c's entries, then d's" splits exactly (include/fmhip_topk.h):
//     score(c, d) = (yhat(c) + (yhat(d) - w0)) + sum_f q_f(c) q_f(d)
// so after one kFwdQ forward over each row set (fm_forward.hip: q into a [rows][Kp] table, yhat beside it) the job is a
// [B x Kp] . [Kp x M] product plus two bias vectors.  k_pair_topk forms it on the exact-f32 MFMA (v_mfma_f32_16x16x4_f32: a
// k-ordered fmaf chain from 0, the numerics of every other kernel here) and selects while it goes, so the B x M scores never
// reach memory:
//   - a workgroup (4 waves) owns kTopkTileC = 64 contexts — each wave keeps the q rows of 16 of them in registers as the A
//     operand of all Kp/4 steps — and one SPLIT of the candidates, which it streams through LDS kTopkTileD = 64 rows at a time:
//     the tile walk (prefetch, k-permuted layout, MFMA steps) is PairTiles, fm_pair_tiles.h, shared with fm_rank.hip;
//   - a wave forms four 16 x 16 blocks per tile (four independent accumulators: the MFMA's issue rate), adds the biases and
//     offers a score to its context's running best-K list only if it is not below the list's K-th score: one float compare
//     per score and one branch per tile on the common path, against thresholds held in registers.  What passes is inserted by the whole wave (the list
//     is sorted, 1 or 2 entries per lane: compare, ballot, shift by one, store); exclusions are looked up (binary search) only
//     then.  A context belongs to ONE wave, so lists need no atomics and no workgroup barrier;
//   - a list entry is one 64-bit word, (order-preserving key of the score) << 32 | ~(candidate row): larger = better, i.e.
//     higher score first, lower row first among equals, NaN (key 0) below -Inf, the empty slot (0) below everything.
// k_topk_merge then merges the splits' lists of a context.  k_pair_scores is the same product, every score stored.
// The score of a pair is one fixed expression whatever tile, split or chunk it falls into: results are bit-identical run
// to run and batch to batch.
#include "fm_topk.h"
#include "fm_pair_tiles.h"
#include "fm_score_key.h"

#include <algorithm>

namespace fmhip {

namespace {

typedef unsigned long long u64;

constexpr int kThreads = kPairThreads;
constexpr int TC = kTopkTileC, TD = kTopkTileD;

// what a score must not be below to be worth offering to a list whose last entry is `last` (a list that is not full, or whose
// K-th score is NaN, takes anything)
__device__ __forceinline__ float list_threshold(u64 last) {
    const uint32_t key = (uint32_t)(last >> 32);
    return key == 0u ? -__builtin_inff() : key_score(key);
}

__device__ __forceinline__ u64 readlane64(u64 v, int lane) {
    const uint32_t lo = __builtin_amdgcn_readlane((int)(uint32_t)v, lane), hi = __builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
    return ((u64)hi << 32) | lo;
}

// is candidate row d in the ascending list excl[lo, hi)?  (wave-uniform arguments: every lane walks the same path)
__device__ __forceinline__ bool excluded(const int32_t *excl, int64_t lo, int64_t hi, int32_t d) {
    const int64_t end = hi;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (excl[mid] < d) lo = mid + 1;
        else hi = mid;
    }
    return lo < end && excl[lo] == d;
}

// The whole wave inserts c (wave-uniform, larger than L[K - 1], distinct from every entry) into the descending list L[0, K),
// K <= 128: lane l holds entries l and l + 64; the entries below c move down one slot, the last one falls off.
__device__ __forceinline__ void list_insert(u64 *L, int K, u64 c, int l) {
    const bool in0 = l < K, in1 = l + 64 < K;
    const u64 e0 = in0 ? L[l] : 0ull, e1 = in1 ? L[l + 64] : 0ull;
    const bool g0 = in0 && e0 > c, g1 = in1 && e1 > c;
    const int pos = __popcll(__ballot(g0)) + __popcll(__ballot(g1));
    if (in0 && !g0 && l + 1 < K) L[l + 1] = e0;
    if (in1 && !g1 && l + 65 < K) L[l + 65] = e1;
    if (l == 0) L[pos] = c;
}

template <int KP, bool SELECT>
__global__ __launch_bounds__(kThreads) void k_pair_topk(const TopkArgs a) {
    constexpr int S = PairTiles<KP>::S;      // MFMA steps
    constexpr PairTileLds lds = pair_tile_lds(KP);
    extern __shared__ __align__(16) unsigned char smem[];
    u64 *lists = reinterpret_cast<u64 *>(smem + lds.tile_bytes + lds.bd_bytes);      // SELECT: [TC][K]
    const int tid = threadIdx.x, l = tid & 63, wv = tid >> 6, g = l >> 4, c15 = l & 15;
    const int K = a.K;
    const int cw = blockIdx.x * TC + wv * 16;                 // the wave's first context
    const int n_splits = gridDim.y, split = blockIdx.y;
    const int64_t d_lo = (int64_t)split * a.split_len, d_hi = min((int64_t)a.M, d_lo + a.split_len);

    // A operand of step s: Qc[context c15 of the wave][4s + g]; rows past the chunk are zero
    float A[S];
    {
        const bool ok = cw + c15 < a.B;
        const float *q = a.t.Qc + (size_t)(ok ? cw + c15 : 0) * KP + g;
#pragma unroll
        for (int s = 0; s < S; ++s) A[s] = ok ? q[4 * s] : 0.f;
    }
    // the accumulators' rows: contexts 4g + i of the wave
    float yc[4], thr[4];
    bool vc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        vc[i] = cw + 4 * g + i < a.B;
        yc[i] = vc[i] ? a.t.yc[cw + 4 * g + i] : 0.f;
        thr[i] = -__builtin_inff();
    }
    u64 *wl = lists + (size_t)(wv * 16) * K;                  // the wave's 16 lists
    if (SELECT)
        for (int t = l; t < 16 * K; t += 64) wl[t] = 0ull;

    PairTiles<KP> pt{reinterpret_cast<float *>(smem), reinterpret_cast<float *>(smem + lds.tile_bytes), a.t.Qd, a.t.yd, *a.t.w0, d_lo, d_hi,
                     tid, g, c15};
    if (d_lo < d_hi) pt.fetch(d_lo);
    for (int64_t d0 = d_lo; d0 < d_hi; d0 += TD) {
        f32x4 acc[4];
        pt.product(d0, A, acc);

        // lane (g, c15) holds, in acc[j][i], the pair (context 4g + i of the wave, candidate d0 + 16j + c15)
        float bdv[4];
        bool vd[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            bdv[j] = pt.bd[16 * j + c15];
            vd[j] = d0 + 16 * j + c15 < d_hi;
        }
        if constexpr (!SELECT) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (vd[j] && vc[i]) a.out[(size_t)(cw + 4 * g + i) * a.M + (size_t)(d0 + 16 * j + c15)] = pair_score(yc[i], bdv[j], acc[j][i]);
        } else {
            // the common path: one compare per score (the raw sum orders like the canonical score; a NaN passes), one branch per tile
            bool any = false;
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int i = 0; i < 4; ++i) any |= vd[j] && vc[i] && !((yc[i] + bdv[j]) + acc[j][i] < thr[i]);
            if (__ballot(any) != 0ull) {
                // rare: some lanes hold a score that may enter its context's list — the wave takes them one at a time
#pragma unroll
                for (int j = 0; j < 4; ++j) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        u64 mask = __ballot(vd[j] && vc[i] && !((yc[i] + bdv[j]) + acc[j][i] < thr[i]));
                        if (mask == 0ull) continue;
                        const u64 mine = order_word(pair_score(yc[i], bdv[j], acc[j][i]), (uint32_t)(d0 + 16 * j + c15));
                        while (mask) {
                            const int src = __builtin_amdgcn_readfirstlane(__ffsll((unsigned long long)mask) - 1);
                            mask &= mask - 1;
                            const u64 c = readlane64(mine, src);
                            const int row = (src >> 4) * 4 + i;
                            u64 *L = wl + (size_t)row * K;
                            if (c <= L[K - 1]) continue;
                            if (a.excl_ptr &&
                                excluded(a.excl, a.excl_ptr[cw + row], a.excl_ptr[cw + row + 1], (int32_t)(0xffffffffu - (uint32_t)c)))
                                continue;
                            list_insert(L, K, c, l);
                        }
#pragma unroll
                        for (int i2 = 0; i2 < 4; ++i2) thr[i2] = list_threshold(wl[(size_t)(4 * g + i2) * K + K - 1]);
                    }
                }
            }
        }
    }
    if (SELECT)
        for (int t = l; t < 16 * K; t += 64) {
            const int c = cw + t / K;
            if (c < a.B) a.part[((size_t)c * n_splits + split) * K + t % K] = wl[t];
        }
}

// One wave per context: the K best of its `splits` sorted lists, by repeated selection of the best head (a lane holds the
// heads of lists l, l + 64, ...; entries are distinct, so exactly one lane owns the winner).
__global__ __launch_bounds__(kThreads) void k_topk_merge(const u64 *part, int B, int splits, int K, int32_t *idx, float *score) {
    constexpr int H = kTopkMaxSplits / 64;
    const int l = threadIdx.x & 63, c = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (c >= B) return;
    const u64 *P = part + (size_t)c * splits * K;
    int head[H];
    u64 hv[H];
#pragma unroll
    for (int m = 0; m < H; ++m) {
        head[m] = 0;
        hv[m] = l + 64 * m < splits ? P[(size_t)(l + 64 * m) * K] : 0ull;
    }
    for (int r = 0; r < K; ++r) {
        u64 best = 0ull;
#pragma unroll
        for (int m = 0; m < H; ++m) best = hv[m] > best ? hv[m] : best;
        u64 top = best;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const u64 o = __shfl_xor(top, off, 64);
            top = o > top ? o : top;
        }
        if (l == 0) {
            // an empty slot: no candidate left
            idx[(size_t)c * K + r] = top ? (int32_t)(0xffffffffu - (uint32_t)top) : -1;
            score[(size_t)c * K + r] = top ? key_score((uint32_t)(top >> 32)) : -__builtin_inff();
        }
        if (top != 0ull && best == top) {
#pragma unroll
            for (int m = 0; m < H; ++m)
                if (hv[m] == top) {
                    ++head[m];
                    hv[m] = head[m] < K ? P[(size_t)(l + 64 * m) * K + head[m]] : 0ull;
                }
        }
    }
}

size_t topk_lds_bytes(int Kp, int K, bool select) {
    const PairTileLds lds = pair_tile_lds(Kp);
    return lds.tile_bytes + lds.bd_bytes + (select ? (size_t)TC * K * sizeof(u64) : 0);
}

template <int KP, bool SELECT>
hipError_t launch_pair(const TopkArgs &a, hipStream_t s) {
    if (a.B <= 0 || a.M <= 0) return hipSuccess;
    const size_t lds = topk_lds_bytes(KP, a.K, SELECT);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_pair_topk<KP, SELECT>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)((a.B + TC - 1) / TC), (unsigned)((a.M + a.split_len - 1) / a.split_len));
    hipLaunchKernelGGL((k_pair_topk<KP, SELECT>), grid, dim3(kThreads), lds, s, a);
    return hipGetLastError();
}

template <bool SELECT>
hipError_t launch_pair_kp(int Kp, const TopkArgs &a, hipStream_t s) {
    switch (Kp) {
        case 32: return launch_pair<32, SELECT>(a, s);
        case 64: return launch_pair<64, SELECT>(a, s);
        case 128: return launch_pair<128, SELECT>(a, s);
        case 256: return launch_pair<256, SELECT>(a, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace

// How many splits?  Every (context, split) list starts empty and pays its first K ln(M_split / K) insertions again, so as few
// as fill the machine: at least kTopkBlocks workgroups (a few per CU), and — the workgroups of a launch all run equally long —
// the fewest more that leave the last round of ~kTopkSlots concurrent workgroups at least 85 % full.
constexpr int kTopkBlocks = 1024, kTopkSlots = 768;
int topk_splits(int64_t B, int64_t M, int32_t *split_len) {
    const int64_t ctx_tiles = std::max<int64_t>((B + TC - 1) / TC, 1), tiles = std::max<int64_t>((M + TD - 1) / TD, 1);
    const int64_t cap = std::min<int64_t>(kTopkMaxSplits, tiles);
    int64_t want = std::min<int64_t>((kTopkBlocks + ctx_tiles - 1) / ctx_tiles, cap);
    for (int64_t s = want; s <= std::min<int64_t>(cap, want + 7); ++s) {
        const int64_t blocks = ctx_tiles * s, rounds = (blocks + kTopkSlots - 1) / kTopkSlots;
        if (blocks * 100 >= rounds * kTopkSlots * 85) { want = s; break; }
    }
    const int64_t per = (tiles + want - 1) / want;      // tiles per split
    *split_len = (int32_t)std::min<int64_t>(per * TD, 0x7fffffc0);
    return (int)((tiles + per - 1) / per);
}

hipError_t launch_pair_topk(int Kp, const TopkArgs &a, hipStream_t s) { return launch_pair_kp<true>(Kp, a, s); }
hipError_t launch_pair_scores(int Kp, const TopkArgs &a, hipStream_t s) { return launch_pair_kp<false>(Kp, a, s); }

hipError_t launch_topk_merge(const unsigned long long *part, int32_t B, int32_t splits, int32_t K, int32_t *idx, float *score,
                             hipStream_t s) {
    if (B <= 0) return hipSuccess;
    if (splits < 1 || splits > kTopkMaxSplits) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_topk_merge, dim3((unsigned)((B + kThreads / 64 - 1) / (kThreads / 64))), dim3(kThreads), 0, s, part, B, splits, K,
                       idx, score);
    return hipGetLastError();
}

}  // namespace fmhip
