// fm_relational.hip — relational data (block-structure FM): the finish that combines the blocks' q-mode passes into a data row's
// prediction, residual and P row (k_rel_finish, a sibling of k_weight_finish), and the deterministic segmented sum that turns
// the batch's P rows into a block's P_b / e_b (k_rel_gather_sum, k_rel_gather_long).  The rule and the buffers: fm_relational.h.
// Lane geometry: fm_device.h.
#include "fm_device.h"
#include "fm_kernels.h"
#include "fm_relational.h"

namespace fmhip {
namespace {

__device__ __forceinline__ float f4dot(float4 a, float4 b) { return fmaf(a.x, b.x, fmaf(a.y, b.y, fmaf(a.z, b.z, a.w * b.w))); }

// One slot of LPN lanes per data row (k_weight_finish's geometry): lane l holds floats 4*(l + jj*LPN) .. +3 of a row.  Per relation
// the slot gathers ONE contiguous q row (16 B per lane) and one prediction.  The cross term is accumulated as <q_b, Q so far>
// BEFORE q_b joins Q — the sum over b < b' term by term, not (|Q|^2 - sum |q_b|^2) / 2, which cancels.  The plain part's q row is
// the row's own P row, where its kFwdQ pass left it.  RESID: the scoring form (nothing written to P; the logistic residual also
// sums the rows' log-losses).  Rows grid-strided: the result does not depend on the grid.
template <int LPN, int J, bool PACKED, bool RESID>
__global__ __launch_bounds__(kBlock) void k_rel_finish(RelFinishArgs a) {
    constexpr int KP = 4 * LPN * J;
    constexpr int SLOTS = kBlock / LPN;
    const int l = threadIdx.x & (LPN - 1);
    const int slot = threadIdx.x / LPN;
    const int kl = PACKED ? (a.pack_k >> 2) & (LPN - 1) : 0, kj = PACKED ? (a.pack_k >> 2) / LPN : 0, kc = a.pack_k & 3;
    const bool logistic = a.loss == kLossLogistic;
    const float w0 = *a.w0;
    float st1 = 0.f, st2 = 0.f, stbad = 0.f, stl = 0.f;
    for (int r = blockIdx.x * SLOTS + slot; r < a.n_rows; r += gridDim.x * SLOTS) {
        float4 Q[J];
#pragma unroll
        for (int jj = 0; jj < J; ++jj) Q[jj] = f4zero();
        float cross = 0.f, lin = 0.f;
        for (int b = 0; b < a.m; ++b) {
            const int32_t j = a.map[b][r];
            const float4 *qb = reinterpret_cast<const float4 *>(a.Q[b] + (size_t)j * KP) + l;
            float4 t[J];
#pragma unroll
            for (int jj = 0; jj < J; ++jj) t[jj] = qb[jj * LPN];
            lin += a.yq[b][j] - w0;
#pragma unroll
            for (int jj = 0; jj < J; ++jj) {
                cross += f4dot(t[jj], Q[jj]);
                f4add(Q[jj], t[jj]);
            }
        }
        float4 *p = nullptr;        // (a scoring pass without a plain part has no P at all)
        if (a.has_plain || !RESID) p = reinterpret_cast<float4 *>(a.P + (size_t)r * KP) + l;
        if (a.has_plain) {
            lin += a.yplain[r] - w0;
#pragma unroll
            for (int jj = 0; jj < J; ++jj) {
                const float4 t = p[jj * LPN];
                cross += f4dot(t, Q[jj]);
                f4add(Q[jj], t);
            }
        }
#pragma unroll
        for (int m = LPN >> 1; m >= 1; m >>= 1) cross += __shfl_xor(cross, m, LPN);       // the forward's slot reduction
        const float yh = w0 + (lin + cross);
        float z = 0.f;
        const bool t = a.y[r] > 0.f;
        const float e = logistic ? pair_sigma_residual(yh, t, z) : yh - a.y[r];
        if (!RESID && a.q_only) {       // the pairs' finish follows: the q row as it is, the prediction beside it
#pragma unroll
            for (int jj = 0; jj < J; ++jj) p_store(p + jj * LPN, Q[jj]);
            if (l == 0) a.yhat[r] = yh;
            continue;
        }
        if (!RESID) {
#pragma unroll
            for (int jj = 0; jj < J; ++jj) {
                float4 o = f4mul(Q[jj], e);
                if (PACKED && jj == kj && l == kl) f4set(o, kc, e);                                            // slot k of the P row carries e
                if (!PACKED && kEInP && jj == 0 && l < 8) o = embed_bits4(o, __float_as_uint(e) >> (4 * l));   // no spare slot: e rides in the LSBs (fm_device.h)
                p_store(p + jj * LPN, o);
            }
        }
        if (l == 0) {
            if (a.e) a.e[r] = e;
            if (a.yhat) a.yhat[r] = yh;
            st1 += e;
            st2 = fmaf(e, e, st2);
            if (!isfinite(yh)) stbad += 1.f;
            if (RESID && logistic) stl += fmaxf(t ? -yh : yh, 0.f) + log1pf(z);       // the row's log-loss, as row_finish forms it
        }
    }
    if (!RESID && a.q_only) return;     // (uniform: the statistics are the pairs' finish's)
    double v[4] = {st1, st2, stbad, stl};
    const int where[4] = {0, 1, 2, 3};
    pair_block_sums<4>(a.bsum, v, where);
}

// a finished sum into row `row` of a table in the P row format: e in the packed slot, or embedded in the row's low bits
template <int LPN, int J, bool PACKED>
__device__ __forceinline__ void rel_store_row(float *table, float *etab, int32_t row, int l, float4 (&acc)[J], float es, int32_t pack_k) {
    constexpr int KP = 4 * LPN * J;
    const int kl = PACKED ? (pack_k >> 2) & (LPN - 1) : 0, kj = PACKED ? (pack_k >> 2) / LPN : 0, kc = pack_k & 3;
    float4 *dst = reinterpret_cast<float4 *>(table + (size_t)row * KP) + l;
#pragma unroll
    for (int jj = 0; jj < J; ++jj) {
        float4 o = acc[jj];
        if (PACKED && jj == kj && l == kl) f4set(o, kc, es);
        if (!PACKED && kEInP && jj == 0 && l < 8) o = embed_bits4(o, __float_as_uint(es) >> (4 * l));
        p_store(dst + jj * LPN, o);
    }
    if (l == 0) etab[row] = es;
}

// rows [beg, end) of `list` (row ids into `table`), added in list order; four rows' loads in flight, added in order
template <int LPN, int J>
__device__ __forceinline__ void rel_sum_rows(const float *table, const float *etab, const int32_t *list, int beg, int end, int l, float4 (&acc)[J],
                                             float &es) {
    constexpr int KP = 4 * LPN * J;
    int i = beg;
    for (; i + 4 <= end; i += 4) {
        int32_t r[4];
        float4 t[4][J];
        float ev[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            r[u] = list ? list[i + u] : i + u;
            const float4 *src = reinterpret_cast<const float4 *>(table + (size_t)r[u] * KP) + l;
#pragma unroll
            for (int jj = 0; jj < J; ++jj) t[u][jj] = src[jj * LPN];
            ev[u] = etab[r[u]];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int jj = 0; jj < J; ++jj) f4add(acc[jj], t[u][jj]);
            es += ev[u];
        }
    }
    for (; i < end; ++i) {
        const int32_t r = list ? list[i] : i;
        const float4 *src = reinterpret_cast<const float4 *>(table + (size_t)r * KP) + l;
#pragma unroll
        for (int jj = 0; jj < J; ++jj) f4add(acc[jj], src[jj * LPN]);
        es += etab[r];
    }
}

// One slot per work item (fmhip::host::RelationInverse): up to kRelSumCut listed P rows and their e, summed in ascending row order
// in fp32.  A whole list writes its block row of P_b / e_b; a chunk of a long list writes a partial row.  What an item sums and
// where it writes is fixed by the data (every address has one writer), and the result is the same bits for any grid.
template <int LPN, int J, bool PACKED>
__global__ __launch_bounds__(kBlock) void k_rel_gather_sum(RelGatherArgs a) {
    constexpr int KP = 4 * LPN * J;
    constexpr int SLOTS = kBlock / LPN;
    const int l = threadIdx.x & (LPN - 1);
    const int slot = threadIdx.x / LPN;
    for (int w = blockIdx.x * SLOTS + slot; w < a.n_work; w += gridDim.x * SLOTS) {
        const int32_t t = a.wt[w], beg = a.wbeg[w], dst = a.wdst[w];
        const int32_t end = min(beg + kRelSumCut, a.tptr[t + 1]);
        float4 acc[J];
#pragma unroll
        for (int jj = 0; jj < J; ++jj) acc[jj] = f4zero();
        float es = 0.f;
        rel_sum_rows<LPN, J>(a.P, a.e, a.trow, beg, end, l, acc, es);
        if (dst >= 0) {
            rel_store_row<LPN, J, PACKED>(a.Pb, a.eb, dst, l, acc, es, a.pack_k);
        } else {
            float4 *o = reinterpret_cast<float4 *>(a.part + (size_t)(-1 - dst) * KP) + l;
#pragma unroll
            for (int jj = 0; jj < J; ++jj) o[jj * LPN] = acc[jj];
            if (l == 0) a.part_e[-1 - dst] = es;
        }
    }
}

// One slot per long list: its chunks' partial rows, added in chunk order, into the block row.
template <int LPN, int J, bool PACKED>
__global__ __launch_bounds__(kBlock) void k_rel_gather_long(RelGatherArgs a) {
    constexpr int SLOTS = kBlock / LPN;
    const int l = threadIdx.x & (LPN - 1);
    const int slot = threadIdx.x / LPN;
    for (int i = blockIdx.x * SLOTS + slot; i < a.n_long; i += gridDim.x * SLOTS) {
        const int32_t first = a.lfirst[i];
        float4 acc[J];
#pragma unroll
        for (int jj = 0; jj < J; ++jj) acc[jj] = f4zero();
        float es = 0.f;
        rel_sum_rows<LPN, J>(a.part, a.part_e, nullptr, first, first + a.lcount[i], l, acc, es);
        rel_store_row<LPN, J, PACKED>(a.Pb, a.eb, a.tj[a.lt[i]], l, acc, es, a.pack_k);
    }
}

int slot_blocks(int Kp, int64_t items) {
    const int lpn = Kp <= 64 ? 8 : 16;      // the forward's slot width (launch_forward)
    const int slots = kBlock / lpn;
    int64_t blocks = (items + slots - 1) / slots;
    if (blocks > 8192) blocks = 8192;       // as k_weight_finish: enough workgroups to fill the chip many times over, items grid-strided
    if (blocks < 1) blocks = 1;
    return (int)blocks;
}

}  // namespace

int rel_finish_blocks(int Kp, int64_t n_rows) { return slot_blocks(Kp, n_rows); }

hipError_t launch_rel_finish(int Kp, const RelFinishArgs &a, bool residual_only, hipStream_t s, int *n_partials) {
    const int blocks = rel_finish_blocks(Kp, a.n_rows);
    if (n_partials) *n_partials = blocks;
    const dim3 g((unsigned)blocks), b(kBlock);
#define FMHIP_RF(LPN_, J_)                                                                                          \
    do {                                                                                                            \
        if (residual_only) hipLaunchKernelGGL((k_rel_finish<LPN_, J_, false, true>), g, b, 0, s, a);                \
        else if (a.pack_k >= 0) hipLaunchKernelGGL((k_rel_finish<LPN_, J_, true, false>), g, b, 0, s, a);           \
        else hipLaunchKernelGGL((k_rel_finish<LPN_, J_, false, false>), g, b, 0, s, a);                             \
    } while (0)
    switch (Kp) {       // the instances of launch_weight_finish
        case 32: FMHIP_RF(8, 1); break;
        case 64: FMHIP_RF(8, 2); break;
        case 128: FMHIP_RF(16, 2); break;
        case 256: FMHIP_RF(16, 4); break;
        default: return hipErrorInvalidValue;
    }
#undef FMHIP_RF
    return hipGetLastError();
}

hipError_t launch_rel_gather_sum(int Kp, const RelGatherArgs &a, hipStream_t s) {
    if (a.n_work <= 0) return hipSuccess;
    const dim3 g((unsigned)slot_blocks(Kp, a.n_work)), gl((unsigned)slot_blocks(Kp, a.n_long)), b(kBlock);
#define FMHIP_RG(LPN_, J_)                                                                                          \
    do {                                                                                                            \
        if (a.pack_k >= 0) {                                                                                        \
            hipLaunchKernelGGL((k_rel_gather_sum<LPN_, J_, true>), g, b, 0, s, a);                                  \
            if (a.n_long > 0) hipLaunchKernelGGL((k_rel_gather_long<LPN_, J_, true>), gl, b, 0, s, a);              \
        } else {                                                                                                    \
            hipLaunchKernelGGL((k_rel_gather_sum<LPN_, J_, false>), g, b, 0, s, a);                                 \
            if (a.n_long > 0) hipLaunchKernelGGL((k_rel_gather_long<LPN_, J_, false>), gl, b, 0, s, a);             \
        }                                                                                                           \
    } while (0)
    switch (Kp) {
        case 32: FMHIP_RG(8, 1); break;
        case 64: FMHIP_RG(8, 2); break;
        case 128: FMHIP_RG(16, 2); break;
        case 256: FMHIP_RG(16, 4); break;
        default: return hipErrorInvalidValue;
    }
#undef FMHIP_RG
    return hipGetLastError();
}

}  // namespace fmhip
