// fm_relational.hip — relational data (block-structure FM): the finish that combines the blocks' q-mode passes into a data row's
// prediction, residual and P row (k_rel_finish: a row per slot), and the deterministic segmented sum that turns
// the batch's P rows into a block's P_b / e_b (k_rel_gather_sum, k_rel_gather_long).  The rule and the buffers: fm_relational.h.
// Lane geometry: fm_device.h; what the finishes share: fm_finish.h.
#include "fm_finish.h"
#include "fm_relational.h"

namespace fmhip {
namespace {

// One slot of LPN lanes per data row: lane l holds floats 4*(l + jj*LPN) .. +3 of a row.  Per relation
// the slot gathers ONE contiguous q row (16 B per lane) and one prediction.  The cross term is accumulated as <q_b, Q so far>
// BEFORE q_b joins Q — the sum over b < b' term by term, not (|Q|^2 - sum |q_b|^2) / 2, which cancels.  The plain part's q row is
// the row's own P row, where its kFwdQ pass left it.  RESID: the scoring form (nothing written to P; the logistic residual also
// sums the rows' log-losses).  Rows grid-strided: the result does not depend on the grid.
template <int LPN, int J, bool PACKED, bool RESID>
__global__ __launch_bounds__(kBlock) void k_rel_finish(RelFinishArgs a) {
    constexpr int KP = 4 * LPN * J;
    const SlotLoop<LPN> sl;
    const int l = sl.l;
    const PackPos<LPN, PACKED> k(a.pack_k);
    const bool logistic = a.loss == kLossLogistic;
    const float w0 = *a.w0;
    float st1 = 0.f, st2 = 0.f, stbad = 0.f, stl = 0.f;
    for (int r = sl.first; r < a.n_rows; r += sl.stride) {
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
            for (int jj = 0; jj < J; ++jj) Q[jj] = f4mul(Q[jj], e);
            store_e_row<LPN, J, PACKED>(p, Q, e, l, k);
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
// where it writes is fixed by the data (every address has one writer), and the result is the same bits for any grid — so the
// number of items may as well be read from the device (RelGatherArgs::counts) under a grid sized for the worst case.
template <int LPN, int J, bool PACKED>
__global__ __launch_bounds__(kBlock) void k_rel_gather_sum(RelGatherArgs a) {
    constexpr int KP = 4 * LPN * J;
    const SlotLoop<LPN> sl;
    const int l = sl.l;
    const PackPos<LPN, PACKED> k(a.pack_k);
    const int n_work = a.counts ? min(a.counts[1], a.cap_work) : a.n_work;
    for (int w = sl.first; w < n_work; w += sl.stride) {
        const int32_t t = a.wt[w], beg = a.wbeg[w], dst = a.wdst[w];
        const int32_t end = min(beg + kRelSumCut, a.tptr[t + 1]);
        float4 acc[J];
#pragma unroll
        for (int jj = 0; jj < J; ++jj) acc[jj] = f4zero();
        float es = 0.f;
        rel_sum_rows<LPN, J>(a.P, a.e, a.trow, beg, end, l, acc, es);
        if (dst >= 0) {     // a finished sum: a row of P_b in the P row format, e_b beside it
            store_e_row<LPN, J, PACKED>(reinterpret_cast<float4 *>(a.Pb + (size_t)dst * KP) + l, acc, es, l, k);
            if (l == 0) a.eb[dst] = es;
        } else {
            if (a.counts && -1 - dst >= a.cap_part) continue;      // (device counts: no partial row outside the slice)
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
    constexpr int KP = 4 * LPN * J;
    const SlotLoop<LPN> sl;
    const int l = sl.l;
    const PackPos<LPN, PACKED> k(a.pack_k);
    const int n_long = a.counts ? min(a.counts[2], a.cap_long) : a.n_long;
    for (int i = sl.first; i < n_long; i += sl.stride) {
        const int32_t first = a.lfirst[i], dst = a.tj[a.lt[i]];
        if (a.counts && (first < 0 || a.lcount[i] < 0 || first + a.lcount[i] > a.cap_part)) continue;
        float4 acc[J];
#pragma unroll
        for (int jj = 0; jj < J; ++jj) acc[jj] = f4zero();
        float es = 0.f;
        rel_sum_rows<LPN, J>(a.part, a.part_e, nullptr, first, first + a.lcount[i], l, acc, es);
        store_e_row<LPN, J, PACKED>(reinterpret_cast<float4 *>(a.Pb + (size_t)dst * KP) + l, acc, es, l, k);
        if (l == 0) a.eb[dst] = es;
    }
}

}  // namespace

hipError_t launch_rel_finish(int Kp, const RelFinishArgs &a, bool residual_only, hipStream_t s, int *n_partials) {
    const int blocks = slot_blocks(Kp, a.n_rows);
    if (n_partials) *n_partials = blocks;
    const dim3 g((unsigned)blocks), b(kBlock);
    return for_slot_shape(Kp, [&](auto lpn, auto j) {
        constexpr int L = decltype(lpn)::value, JJ = decltype(j)::value;
        if (residual_only) hipLaunchKernelGGL((k_rel_finish<L, JJ, false, true>), g, b, 0, s, a);
        else if (a.pack_k >= 0) hipLaunchKernelGGL((k_rel_finish<L, JJ, true, false>), g, b, 0, s, a);
        else hipLaunchKernelGGL((k_rel_finish<L, JJ, false, false>), g, b, 0, s, a);
    });
}

hipError_t launch_rel_gather_sum(int Kp, const RelGatherArgs &a, hipStream_t s) {
    const bool dev = a.counts != nullptr;
    if (dev && (a.cap_work < 1 || a.cap_long < 1 || a.cap_part < 1)) return hipErrorInvalidValue;
    const int32_t n_work = dev ? a.cap_work : a.n_work, n_long = dev ? a.cap_long : a.n_long;
    if (n_work <= 0) return hipSuccess;
    const dim3 g((unsigned)slot_blocks(Kp, n_work)), gl((unsigned)slot_blocks(Kp, n_long)), b(kBlock);
    return for_slot_shape(Kp, [&](auto lpn, auto j) {
        constexpr int L = decltype(lpn)::value, JJ = decltype(j)::value;
        if (a.pack_k >= 0) {
            hipLaunchKernelGGL((k_rel_gather_sum<L, JJ, true>), g, b, 0, s, a);
            if (n_long > 0) hipLaunchKernelGGL((k_rel_gather_long<L, JJ, true>), gl, b, 0, s, a);
        } else {
            hipLaunchKernelGGL((k_rel_gather_sum<L, JJ, false>), g, b, 0, s, a);
            if (n_long > 0) hipLaunchKernelGGL((k_rel_gather_long<L, JJ, false>), gl, b, 0, s, a);
        }
    });
}

}  // namespace fmhip
