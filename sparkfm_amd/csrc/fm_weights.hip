// fm_weights.hip — per-row example weights: the residual of a WEIGHTED row, formed after the kFwdQ forward has left the row's
// sv*q in P and its prediction beside it (k_weight_finish: a row per slot), and the weighted scores of a dataset
// (k_weighted_score).  The rule and the buffers: fm_weights.h.  Lane geometry: fm_device.h; what the finishes share: fm_finish.h.
#include "fm_finish.h"
#include "fm_weights.h"

namespace fmhip {
namespace {

// One slot of LPN lanes per row: lane l holds floats 4*(l + jj*LPN) .. +3 of the row (the forward's geometry), so a wave moves
// 64/LPN whole rows per instruction, every row a contiguous 16-B-per-lane segment.  A pure stream over P (read once, written
// once; no LDS but the statistics' few doubles); rows grid-strided, so the result does not depend on the grid.
template <int LPN, int J, bool PACKED>
__global__ __launch_bounds__(kBlock) void k_weight_finish(WeightArgs a) {
    constexpr int KP = 4 * LPN * J;
    const SlotLoop<LPN> sl;
    const int l = sl.l;
    const PackPos<LPN, PACKED> k(a.pack_k);
    const bool logistic = a.loss == kLossLogistic;
    float st1 = 0.f, st2 = 0.f, stbad = 0.f;
    for (int r = sl.first; r < a.n_rows; r += sl.stride) {
        float4 *p = reinterpret_cast<float4 *>(a.P + (size_t)r * KP) + l;
        float4 q[J];
#pragma unroll
        for (int jj = 0; jj < J; ++jj) q[jj] = p[jj * LPN];
        const float yh = a.yhat[r];
        float z;
        // the loss's residual as row_finish (fm_forward.hip) forms it, then the weight
        const float e = weighted_residual(a.c[r], logistic ? pair_sigma_residual(yh, a.y[r] > 0.f, z) : yh - a.y[r]);
#pragma unroll
        for (int jj = 0; jj < J; ++jj) q[jj] = f4mul(q[jj], e);
        store_e_row<LPN, J, PACKED>(p, q, e, l, k);
        if (l == 0) {
            a.e[r] = e;
            st1 += e;
            st2 = fmaf(e, e, st2);
            if (!isfinite(yh)) stbad += 1.f;
        }
    }
    double v[3] = {st1, st2, stbad};
    const int where[3] = {0, 1, 2};
    pair_block_sums<3>(a.bsum, v, where);
}

// a thread per row; fp64 partial sums
__global__ __launch_bounds__(kBlock) void k_weighted_score(const float *yhat, const float *y, const float *c, int32_t n_rows, double *bsum) {
    double sc = 0.0, sse = 0.0, sae = 0.0, sll = 0.0;
    for (int r = blockIdx.x * kBlock + threadIdx.x; r < n_rows; r += gridDim.x * kBlock) {
        const double w = (double)c[r];
        if (!(w > 0.0)) continue;
        const double yh = (double)yhat[r], d = yh - (double)y[r];
        const bool t = y[r] > 0.f;
        sc += w;
        sse += w * d * d;
        sae += w * fabs(d);
        sll += w * (fmax(t ? -yh : yh, 0.0) + log1p(exp(-fabs(yh))));
    }
    double v[4] = {sc, sse, sae, sll};
    const int where[4] = {0, 1, 2, 3};
    pair_block_sums<4>(bsum, v, where);
}

}  // namespace

hipError_t launch_weight_finish(int Kp, const WeightArgs &a, hipStream_t s, int *n_partials) {
    const int blocks = slot_blocks(Kp, a.n_rows);
    if (n_partials) *n_partials = blocks;
    const dim3 g((unsigned)blocks), b(kBlock);
    return for_slot_shape(Kp, [&](auto lpn, auto j) {
        constexpr int L = decltype(lpn)::value, JJ = decltype(j)::value;
        if (a.pack_k >= 0) hipLaunchKernelGGL((k_weight_finish<L, JJ, true>), g, b, 0, s, a);
        else hipLaunchKernelGGL((k_weight_finish<L, JJ, false>), g, b, 0, s, a);
    });
}

int weighted_score_blocks(int64_t n_rows) { return grid_blocks(n_rows, kBlock, 1024); }

hipError_t launch_weighted_score(const float *yhat, const float *y, const float *c, int32_t n_rows, double *bsum, hipStream_t s, int *n_partials) {
    const int blocks = weighted_score_blocks(n_rows);
    if (n_partials) *n_partials = blocks;
    hipLaunchKernelGGL(k_weighted_score, dim3((unsigned)blocks), dim3(kBlock), 0, s, yhat, y, c, n_rows, bsum);
    return hipGetLastError();
}

}  // namespace fmhip
