// fm_pairing.hip — pairwise ranking (BPR / RankNet): the residual of a PAIR of rows, formed after the kFwdQ forward has left
// every row's sv*q in P and its prediction beside it (k_pair_finish), and the scoring of held-out pairs (k_pair_score).
// Formulas and buffers: fm_pairing.h.  Lane geometry: fm_device.h.
#include "fm_device.h"
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
template <int LPN, int J, bool PACKED, bool WEIGHTED>
__global__ __launch_bounds__(kBlock) void k_pair_finish(PairArgs a) {
    constexpr int KP = 4 * LPN * J;
    constexpr int SLOTS = kBlock / LPN;
    const int l = threadIdx.x & (LPN - 1);
    const int slot = threadIdx.x / LPN;
    const int kl = PACKED ? (a.pack_k >> 2) & (LPN - 1) : 0, kj = PACKED ? (a.pack_k >> 2) / LPN : 0, kc = a.pack_k & 3;
    const bool logistic = a.loss == kLossLogistic;
    float st2 = 0.f, stbad = 0.f;
    for (int j = blockIdx.x * SLOTS + slot; j < a.n_pairs; j += gridDim.x * SLOTS) {
        float4 *p0 = reinterpret_cast<float4 *>(a.P + (size_t)(2 * j) * KP) + l, *p1 = p0 + KP / 4;
        float4 r0[J], r1[J];
#pragma unroll
        for (int jj = 0; jj < J; ++jj) { r0[jj] = p0[jj * LPN]; r1[jj] = p1[jj * LPN]; }
        const float2 yh = reinterpret_cast<const float2 *>(a.yhat)[j], yy = reinterpret_cast<const float2 *>(a.y)[j];
        const float d = yh.x - yh.y, dy = yy.x - yy.y;
        float z;
        float g = logistic ? pair_sigma_residual(d, dy > 0.f, z) : d - dy;
        if (WEIGHTED) g = weighted_residual(a.c[2 * j], g);
        const float e0 = g, e1 = -g;
#pragma unroll
        for (int jj = 0; jj < J; ++jj) {
            float4 o0 = f4mul(r0[jj], e0), o1 = f4mul(r1[jj], e1);
            if (PACKED && jj == kj && l == kl) { f4set(o0, kc, e0); f4set(o1, kc, e1); }   // slot k of the P row carries e
            if (!PACKED && kEInP && jj == 0 && l < 8) {                                    // no spare slot: e rides in the LSBs (fm_device.h)
                o0 = embed_bits4(o0, __float_as_uint(e0) >> (4 * l));
                o1 = embed_bits4(o1, __float_as_uint(e1) >> (4 * l));
            }
            p_store(p0 + jj * LPN, o0);
            p_store(p1 + jj * LPN, o1);
        }
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

int pair_finish_blocks(int Kp, int64_t n_pairs) {
    const int lpn = Kp <= 64 ? 8 : 16;      // the forward's slot width (launch_forward)
    const int slots = kBlock / lpn;
    int64_t blocks = (n_pairs + slots - 1) / slots;
    if (blocks > 8192) blocks = 8192;       // as k_apply: enough workgroups to fill the chip many times over, pairs grid-strided
    if (blocks < 1) blocks = 1;
    return (int)blocks;
}

hipError_t launch_pair_finish(int Kp, const PairArgs &a, hipStream_t s, int *n_partials) {
    const int blocks = pair_finish_blocks(Kp, a.n_pairs);
    if (n_partials) *n_partials = blocks;
    const dim3 g((unsigned)blocks), b(kBlock);
#define FMHIP_PF(LPN_, J_)                                                                      \
    do {                                                                                        \
        if (a.c) {                                                                                      \
            if (a.pack_k >= 0) hipLaunchKernelGGL((k_pair_finish<LPN_, J_, true, true>), g, b, 0, s, a);  \
            else hipLaunchKernelGGL((k_pair_finish<LPN_, J_, false, true>), g, b, 0, s, a);               \
        } else if (a.pack_k >= 0) hipLaunchKernelGGL((k_pair_finish<LPN_, J_, true, false>), g, b, 0, s, a); \
        else hipLaunchKernelGGL((k_pair_finish<LPN_, J_, false, false>), g, b, 0, s, a);                \
    } while (0)
    switch (Kp) {
        case 32: FMHIP_PF(8, 1); break;
        case 64: FMHIP_PF(8, 2); break;
        case 128: FMHIP_PF(16, 2); break;
        case 256: FMHIP_PF(16, 4); break;
        default: return hipErrorInvalidValue;
    }
#undef FMHIP_PF
    return hipGetLastError();
}

int pair_score_blocks(int64_t n_pairs) {
    int64_t blocks = (n_pairs + kBlock - 1) / kBlock;
    if (blocks > 1024) blocks = 1024;
    if (blocks < 1) blocks = 1;
    return (int)blocks;
}

hipError_t launch_pair_score(const float *yhat, const float *y, int32_t n_pairs, double *bsum, hipStream_t s, int *n_partials) {
    const int blocks = pair_score_blocks(n_pairs);
    if (n_partials) *n_partials = blocks;
    hipLaunchKernelGGL(k_pair_score, dim3((unsigned)blocks), dim3(kBlock), 0, s, yhat, y, n_pairs, bsum);
    return hipGetLastError();
}

}  // namespace fmhip
