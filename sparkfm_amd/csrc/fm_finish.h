// fm_finish.h — what the streaming kernels behind a q-mode forward share (k_pair_finish, fm_pairing.hip; k_weight_finish,
// fm_weights.hip; k_rel_finish and the segmented sums, fm_relational.hip): the P row that carries e, the slot loop, the grid rule,
// the Kp -> (LPN, J) dispatch, the residual forms and the block partial.  Each of those kernels is a pure stream over P — a slot
// of LPN lanes per item, lane l holding floats 4*(l + jj*LPN) .. +3 of a row (the forward's geometry, fm_device.h) — with a wide
// register margin, so everything here is a plain __forceinline__ function.
#pragma once
#include <type_traits>

#include "fm_device.h"

namespace fmhip {
namespace {

// ---- the P row that carries e --------------------------------------------------------------------------------------------------
// THE format the backward reads (e_from_row, fm_device.h; the packed slot, fm_backward.hip): slot pack_k of a packed row holds e;
// a row without a spare slot (k == Kp) carries the 32 bits of e in the low mantissa bits of its first 32 floats (embed_bits4).
// row_finish (fm_forward.hip) keeps the original, written into its P-row loop: calling store_e_row there changed its instances'
// register allocation (the assembly no longer matched), and those instances are tuned to the register.

// where slot pack_k lies: lane kl of the row's slot, float4 kj of that lane, component kc
template <int LPN, bool PACKED>
struct PackPos {
    int kl, kj, kc;
    __device__ __forceinline__ explicit PackPos(int32_t pack_k)
        : kl(PACKED ? (pack_k >> 2) & (LPN - 1) : 0), kj(PACKED ? (pack_k >> 2) / LPN : 0), kc(pack_k & 3) {}
};

// lane l's share o of a formed P row (the caller multiplied, or summed) goes to dst[jj * LPN] with e put into it
template <int LPN, int J, bool PACKED>
__device__ __forceinline__ void store_e_row(float4 *dst, float4 (&o)[J], float e, int l, const PackPos<LPN, PACKED> &k) {
#pragma unroll
    for (int jj = 0; jj < J; ++jj) {
        if (PACKED && jj == k.kj && l == k.kl) f4set(o[jj], k.kc, e);                                          // slot k of the P row carries e
        if (!PACKED && kEInP && jj == 0 && l < 8) o[jj] = embed_bits4(o[jj], __float_as_uint(e) >> (4 * l));   // no spare slot: e rides in the LSBs
        p_store(dst + jj * LPN, o[jj]);
    }
}

// ---- the slot loop -------------------------------------------------------------------------------------------------------------
// for (int i = sl.first; i < items; i += sl.stride): items grid-strided, so no result depends on the grid
template <int LPN>
struct SlotLoop {
    static constexpr int SLOTS = kBlock / LPN;
    int l, first, stride;      // the lane's index in its slot; the slot's first item; items per pass of the grid
    __device__ __forceinline__ SlotLoop() : l(threadIdx.x & (LPN - 1)), first(blockIdx.x * SLOTS + threadIdx.x / LPN), stride(gridDim.x * SLOTS) {}
};

// grid of a slot-per-item kernel: enough workgroups to fill the chip many times over (as k_apply), the rest grid-strided
inline int slot_blocks(int Kp, int64_t items) {
    return grid_blocks(items, kBlock / (Kp <= 64 ? 8 : 16), 8192);      // the forward's slot width (launch_forward)
}

// launch(integral_constant LPN, integral_constant J) for the instance of Kp, then the launch's error
template <typename Launch>
hipError_t for_slot_shape(int Kp, Launch &&launch) {
    switch (Kp) {
        case 32: launch(std::integral_constant<int, 8>(), std::integral_constant<int, 1>()); break;
        case 64: launch(std::integral_constant<int, 8>(), std::integral_constant<int, 2>()); break;
        case 128: launch(std::integral_constant<int, 16>(), std::integral_constant<int, 2>()); break;
        case 256: launch(std::integral_constant<int, 16>(), std::integral_constant<int, 4>()); break;
        default: return hipErrorInvalidValue;      // (padded_factors: one of these four)
    }
    return hipGetLastError();
}

// ---- residuals and statistics --------------------------------------------------------------------------------------------------
// sigma(d) - t, t in {0, 1}, without overflow — the form of row_finish (fm_forward.hip) applied to the pair's margin: z = exp(-|d|)
// <= 1, and 1 - sigma(d) = sigma(-d) is formed directly, so a saturated margin on the right side gives a tiny residual rather
// than a difference of two numbers near 1.  z is handed back for the log-loss, log1p(z) + max(t ? -d : d, 0).
__device__ __forceinline__ float pair_sigma_residual(float d, bool t, float &z) {
    z = expf(-fabsf(d));
    const float inv = 1.f / (1.f + z);
    const bool pos = d >= 0.f;
    return t ? -(pos ? z * inv : inv) : (pos ? inv : z * inv);
}

// The residual of a weighted row (fm_weights.h): c * e, and +0 for a row of weight 0 whatever its e — a non-finite one included —
// so that such a row adds exactly nothing anywhere (its sign bit too: e rides in the P row's bits, kEInP).
__device__ __forceinline__ float weighted_residual(float c, float e) { return c > 0.f ? c * e : 0.f; }

// block partial of N sums (fixed order), to bsum[blockIdx.x][4] (the slots past N: 0)
template <int N>
__device__ __forceinline__ void pair_block_sums(double *bsum, double (&v)[N], const int (&slot)[N]) {
    static_assert(N <= 4, "a partial has four slots");
    __shared__ double sh[N][kBlock / 64];
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) v[i] += __shfl_xor(v[i], m, 64);
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int i = 0; i < N; ++i) sh[i][wv] = v[i];
    __syncthreads();
    if (threadIdx.x == 0) {
        double o[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int i = 0; i < N; ++i) {
            double t = 0.0;
#pragma unroll
            for (int w = 0; w < kBlock / 64; ++w) t += sh[i][w];
            o[slot[i]] = t;
        }
        *reinterpret_cast<double4 *>(bsum + (size_t)blockIdx.x * 4) = make_double4(o[0], o[1], o[2], o[3]);
    }
}

}  // namespace
}  // namespace fmhip
