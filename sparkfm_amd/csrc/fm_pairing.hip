// fm_pairing.hip — pairwise ranking (BPR / RankNet): the residual of a PAIR of rows, formed after the kFwdQ forward has left
// every row's sv*q in P and its prediction beside it (k_pair_finish), and the scoring of held-out pairs (k_pair_score).
// Formulas and buffers: fm_pairing.h.  Lane geometry: fm_device.h; what the finishes share: fm_finish.h.
#include "fm_finish.h"
#include "fm_pairing.h"

namespace fmhip {
namespace {

// One slot of LPN lanes per pair: lane l holds floats 4*(l + jj*LPN) .. +3 of both rows (the forward's geometry), so a wave
// moves 64/LPN pairs = 128/LPN whole rows per instruction, every row a contiguous 16-B-per-lane segment.  A pure stream over P
// (read once, written once; no LDS but the statistics' few doubles); pairs grid-strided, so the result does not depend on the grid.
// sum e is never formed: the partial's first slot is 0.0, which is what (+g) + (-g) summed pair by pair would have to be and what
// a sum over rows in any other order is not.
// WEIGHTED (a weighted dataset, fm_weights.h): the pair's residual is c_2j * g — row 2j's weight; row 2j+1's is not read — so the
// rows' residuals still sum to exactly zero.  The unweighted instances do not see the pointer.
// HINGE (the WARP step, fm_pairing.h: kPairLossHinge; always WEIGHTED): g = -1 where d < margin, else 0 — also for a NaN d, which
// the non-finite count still sees — times the pair's weight.  The other instances do not see the margin.
// GIVEN (the sampled softmax's step, fm_pairing.h: kPairLossGiven): g = -c[2j], formed by the pre-pass (fm_softmax.hip); a pair
// whose c is not > 0 gets e = 0 and P rows of exact zeros whatever its q rows hold, so an interaction the pre-pass zeroed for a
// non-finite margin adds nothing anywhere.  The other instances are what they were.
template <int LPN, int J, bool PACKED, bool WEIGHTED, bool HINGE = false, bool GIVEN = false>
__global__ __launch_bounds__(kBlock) void k_pair_finish(PairArgs a) {
    constexpr int KP = 4 * LPN * J;
    const SlotLoop<LPN> sl;
    const int l = sl.l;
    const PackPos<LPN, PACKED> k(a.pack_k);
    const bool logistic = a.loss == kLossLogistic;
    float st2 = 0.f, stbad = 0.f;
    for (int j = sl.first; j < a.n_pairs; j += sl.stride) {
        float4 *p0 = reinterpret_cast<float4 *>(a.P + (size_t)(2 * j) * KP) + l, *p1 = p0 + KP / 4;
        float4 r0[J], r1[J];
#pragma unroll
        for (int jj = 0; jj < J; ++jj) { r0[jj] = p0[jj * LPN]; r1[jj] = p1[jj * LPN]; }
        const float2 yh = reinterpret_cast<const float2 *>(a.yhat)[j], yy = reinterpret_cast<const float2 *>(a.y)[j];
        const float d = yh.x - yh.y, dy = yy.x - yy.y;
        float z;
        float g;
        if (GIVEN) g = a.c[2 * j] > 0.f ? -a.c[2 * j] : 0.f;
        else if (HINGE) g = d < a.margin ? -1.f : 0.f;
        else g = logistic ? pair_sigma_residual(d, dy > 0.f, z) : d - dy;
        if (WEIGHTED) g = weighted_residual(a.c[2 * j], g);
        const float e0 = g, e1 = -g;
#pragma unroll
        for (int jj = 0; jj < J; ++jj) { r0[jj] = f4mul(r0[jj], e0); r1[jj] = f4mul(r1[jj], e1); }
        if (GIVEN && g == 0.f) {
#pragma unroll
            for (int jj = 0; jj < J; ++jj) r0[jj] = r1[jj] = f4zero();
        }
        store_e_row<LPN, J, PACKED>(p0, r0, e0, l, k);
        store_e_row<LPN, J, PACKED>(p1, r1, e1, l, k);
        if (l == 0) {
            reinterpret_cast<float2 *>(a.e)[j] = make_float2(e0, e1);
            st2 = fmaf(e0, e0, st2);
            st2 = fmaf(e1, e1, st2);
            if (!isfinite(yh.x)) stbad += 1.f;
            if (!isfinite(yh.y)) stbad += 1.f;
        }
    }
    double v[2] = {st2, stbad};
    const int where[2] = {1, 2};
    pair_block_sums<2>(a.bsum, v, where);
}

// a thread per pair; fp64 partial sums
__global__ __launch_bounds__(kBlock) void k_pair_score(const float *yhat, const float *y, int32_t n_pairs, double *bsum) {
    double conc = 0.0, sse = 0.0, bad = 0.0, ll = 0.0;
    for (int j = blockIdx.x * kBlock + threadIdx.x; j < n_pairs; j += gridDim.x * kBlock) {
        const float2 yh = reinterpret_cast<const float2 *>(yhat)[j], yy = reinterpret_cast<const float2 *>(y)[j];
        const float d = yh.x - yh.y;
        const bool t = yy.x - yy.y > 0.f;
        float z;
        const float g = pair_sigma_residual(d, t, z);
        // the pair's loss in fp64 (a scoring pass over rows/2 numbers: the transcendental's rate does not matter), so that a
        // model that cannot tell the rows apart scores log 2 to fp64 rounding
        const double dd = (double)d;
        ll += fmax(t ? -dd : dd, 0.0) + log1p(exp(-fabs(dd)));
        conc += d == 0.f ? 0.5 : ((d > 0.f) == t ? 1.0 : 0.0);
        sse += 2.0 * (double)g * (double)g;
        bad += (isfinite(yh.x) ? 0.0 : 1.0) + (isfinite(yh.y) ? 0.0 : 1.0);
    }
    double v[4] = {conc, sse, bad, ll};
    const int where[4] = {0, 1, 2, 3};
    pair_block_sums<4>(bsum, v, where);
}

}  // namespace

hipError_t launch_pair_finish(int Kp, const PairArgs &a, hipStream_t s, int *n_partials) {
    if (a.loss == kPairLossHinge && (!a.c || !(a.margin >= 0.f))) return hipErrorInvalidValue;
    if (a.loss == kPairLossGiven && !a.c) return hipErrorInvalidValue;
    const int blocks = slot_blocks(Kp, a.n_pairs);
    if (n_partials) *n_partials = blocks;
    const dim3 g((unsigned)blocks), b(kBlock);
    return for_slot_shape(Kp, [&](auto lpn, auto j) {
        constexpr int L = decltype(lpn)::value, JJ = decltype(j)::value;
        if (a.loss == kPairLossGiven) {
            if (a.pack_k >= 0) hipLaunchKernelGGL((k_pair_finish<L, JJ, true, false, false, true>), g, b, 0, s, a);
            else hipLaunchKernelGGL((k_pair_finish<L, JJ, false, false, false, true>), g, b, 0, s, a);
        } else if (a.loss == kPairLossHinge) {
            if (a.pack_k >= 0) hipLaunchKernelGGL((k_pair_finish<L, JJ, true, true, true>), g, b, 0, s, a);
            else hipLaunchKernelGGL((k_pair_finish<L, JJ, false, true, true>), g, b, 0, s, a);
        } else if (a.c) {
            if (a.pack_k >= 0) hipLaunchKernelGGL((k_pair_finish<L, JJ, true, true>), g, b, 0, s, a);
            else hipLaunchKernelGGL((k_pair_finish<L, JJ, false, true>), g, b, 0, s, a);
        } else if (a.pack_k >= 0) hipLaunchKernelGGL((k_pair_finish<L, JJ, true, false>), g, b, 0, s, a);
        else hipLaunchKernelGGL((k_pair_finish<L, JJ, false, false>), g, b, 0, s, a);
    });
}

hipError_t launch_pair_score(const float *yhat, const float *y, int32_t n_pairs, double *bsum, hipStream_t s, int *n_partials) {
    const int blocks = grid_blocks(n_pairs, kBlock, 1024);
    if (n_partials) *n_partials = blocks;
    hipLaunchKernelGGL(k_pair_score, dim3((unsigned)blocks), dim3(kBlock), 0, s, yhat, y, n_pairs, bsum);
    return hipGetLastError();
}

}  // namespace fmhip
