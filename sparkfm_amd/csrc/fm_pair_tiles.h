// fm_pair_tiles.h — the candidate-tile walk of the pair kernels (k_pair_topk in fm_topk.hip, k_pair_rank in fm_rank.hip), owned
// once.  Both form a [64 rows x Kp] . [Kp x candidates] product on the exact-f32 MFMA (v_mfma_f32_16x16x4_f32: a k-ordered fmaf
// chain from 0): each wave holds the q rows of 16 contexts (or queries) in registers as the A operand of all Kp/4 steps, and
// the workgroup streams its split of the candidates through LDS kTopkTileD = 64 rows at a time:
//   - the NEXT tile's rows are fetched into registers before the current tile's product starts (their latency hides behind
//     it) and stored to LDS after it, behind two workgroup barriers;
//   - the tile is stored k-permuted (slot 4s + g of a row at g * Kp/4 + s) so that lane group g reads the B operands of four
//     consecutive steps with one ds_read_b128;
//   - a wave forms four 16 x 16 blocks per tile in four independent accumulators (the MFMA's issue rate).
// What a kernel does with a tile's product — insert into a list, store, compare and count — stays in the kernel, and so does its
// loop over the tiles:
//     PairTiles<KP> pt{...};
//     if (d_lo < d_hi) pt.fetch(d_lo);
//     for (int64_t d0 = d_lo; d0 < d_hi; d0 += kTopkTileD) { f32x4 acc[4]; pt.product(d0, A, acc); ... }
// The bits of a pair's dot product are the same in both kernels because they are these lines.
#pragma once
#include "fm_topk.h"

namespace fmhip {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kPairThreads = 256;     // a workgroup of the pair kernels: 4 waves

// the LDS of a tile walk: the tile [kTopkTileD][ld] (the pad of 4 floats spreads the 16 rows of a read over the banks), then
// bd [kTopkTileD] = yhat(d) - w0; a kernel's own LDS starts at tile_bytes + bd_bytes
struct PairTileLds {
    int ld;
    size_t tile_bytes, bd_bytes;
};
constexpr PairTileLds pair_tile_lds(int Kp) {
    return {Kp + 4, (size_t)kTopkTileD * (Kp + 4) * sizeof(float), (size_t)kTopkTileD * sizeof(float)};
}

template <int KP>
struct PairTiles {
    static constexpr int TD = kTopkTileD;
    static constexpr int S = KP / 4;                 // MFMA steps; also the floats of one lane group's region of a tile row
    static constexpr int LD = pair_tile_lds(KP).ld;  // floats per tile row
    // A thread moves UN units of a tile, a unit = 16 consecutive slots of a candidate row: four float4 in, regrouped by lane
    // group, four float4 out.
    static constexpr int UNITS = TD * (KP / 16), UN = (UNITS + kPairThreads - 1) / kPairThreads;

    float *tile;                // [TD][LD], slot 4s + g of a row at g * S + s
    float *bd;                  // [TD] yhat(d) - w0
    const float *Qd, *yd;
    float w0;
    int64_t d_lo, d_hi;         // the workgroup's split of the candidates
    int tid, g, c15;            // the thread; its lane group and lane within the group
    float4 pre[UN][4];          // the prefetched units
    float pre_y;

    // (a constructor, so that the prefetch registers start undefined: value-initialised with the rest, their loads are waited
    // for where they are issued and the prefetch hides nothing)
    __device__ __forceinline__ PairTiles(float *tile_, float *bd_, const float *Qd_, const float *yd_, float w0_, int64_t d_lo_, int64_t d_hi_,
                                         int tid_, int g_, int c15_)
        : tile(tile_), bd(bd_), Qd(Qd_), yd(yd_), w0(w0_), d_lo(d_lo_), d_hi(d_hi_), tid(tid_), g(g_), c15(c15_) {}

    // request the rows [d0, d0 + TD) of the split (past d_hi: zero rows with bd = 0) into the prefetch registers
    __device__ __forceinline__ void fetch(int64_t d0) {
#pragma unroll
        for (int n = 0; n < UN; ++n) {
            const int u = tid + n * kPairThreads, row = u / (KP / 16), t = u % (KP / 16);
            const bool ok = u < UNITS && d0 + row < d_hi;
            const float4 *src = reinterpret_cast<const float4 *>(Qd + (size_t)(ok ? d0 + row : d_lo) * KP) + 4 * t;
#pragma unroll
            for (int i = 0; i < 4; ++i) pre[n][i] = ok ? src[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        if (tid < TD) pre_y = d0 + tid < d_hi ? yd[d0 + tid] : w0;
    }
    // the prefetch registers -> LDS, k-permuted
    __device__ __forceinline__ void stash() {
#pragma unroll
        for (int n = 0; n < UN; ++n) {
            const int u = tid + n * kPairThreads, row = u / (KP / 16), t = u % (KP / 16);
            if (u >= UNITS) continue;
            float *dst = tile + row * LD + 4 * t;
            *reinterpret_cast<float4 *>(dst + 0 * S) = make_float4(pre[n][0].x, pre[n][1].x, pre[n][2].x, pre[n][3].x);
            *reinterpret_cast<float4 *>(dst + 1 * S) = make_float4(pre[n][0].y, pre[n][1].y, pre[n][2].y, pre[n][3].y);
            *reinterpret_cast<float4 *>(dst + 2 * S) = make_float4(pre[n][0].z, pre[n][1].z, pre[n][2].z, pre[n][3].z);
            *reinterpret_cast<float4 *>(dst + 3 * S) = make_float4(pre[n][0].w, pre[n][1].w, pre[n][2].w, pre[n][3].w);
        }
        if (tid < TD) bd[tid] = pre_y - w0;
    }
    // Advance to tile d0, whose rows the previous call (or the kernel's first fetch) requested: it goes to LDS, the next tile
    // is requested, and the wave's product with it is formed from zero.  Lane (g, c15) then holds, in acc[j][i], the dot product
    // of (row 4g + i of the wave's A, candidate d0 + 16j + c15), and bd[16j + c15] that candidate's bias.
    __device__ __forceinline__ void product(int64_t d0, const float (&A)[S], f32x4 (&acc)[4]) {
        __syncthreads();                                       // the previous tile has been read by every wave
        stash();
        __syncthreads();
        if (d0 + TD < d_hi) fetch(d0 + TD);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        const float *brow = tile + c15 * LD + g * S;
#pragma unroll
        for (int t = 0; t < S / 4; ++t) {
            float4 b[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = *reinterpret_cast<const float4 *>(brow + 16 * j * LD + 4 * t);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[4 * t + 0], b[j].x, acc[j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[4 * t + 1], b[j].y, acc[j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[4 * t + 2], b[j].z, acc[j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[4 * t + 3], b[j].w, acc[j], 0, 0, 0);
        }
    }
};

}  // namespace fmhip
