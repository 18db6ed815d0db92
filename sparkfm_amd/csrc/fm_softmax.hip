// fm_softmax.hip — the sampled softmax's pre-pass (include/fmhip_softmax.h): per interaction of a batch of the BPR trainer's pair
// layout, the softmax of {the positive, its n negatives} from the rows' predictions.  Arguments and buffers: fm_softmax.h; the
// block partial: fm_finish.h.
#include "fm_finish.h"
#include "fm_softmax.h"

namespace fmhip {
namespace {

// One group of G lanes per interaction, G the least power of two >= n, 64 at most: lane l takes the pairs q = l, l + G, ... of
// its interaction, q ascending, so an interaction of more than 64 negatives is strode over by one wavefront.  Interactions are
// grid-strided and a group's lanes run the same trips, so every shuffle below stays among active lanes of one group.
// THE ORDER (fixed by n alone, through G): amax = the lane's fmaxf over its q ascending, then an xor tree over the group
// (m = G/2 .. 1); mx = fmaxf(0, amax); z = the lane's sum of expf(a_q - mx) over its q ascending, then the same xor tree (a + b
// and b + a are the same float, so every lane holds the same sum); Z = expf(-mx) + z; pi_q = expf(a_q - mx) / Z;
// loss = mx + logf(Z).  The three passes re-read the 8 B per pair of predictions (and, correcting, the two mapped rows' lq) from
// cache; nothing but pi and the block's partial is written, and there are no atomics.
// An interaction with a non-finite d_q: every pi of it is 0, it adds nothing to the loss and is not counted on top.
template <int G, bool LOGQ>
__global__ __launch_bounds__(kBlock) void k_softmax_pre(SoftmaxArgs a) {
    constexpr int GROUPS = kBlock / G;
    const int l = threadIdx.x & (G - 1);
    const int n = a.n;
    float st2 = 0.f, stbad = 0.f;
    double sttop = 0.0, stl = 0.0;
    for (int j = blockIdx.x * GROUPS + threadIdx.x / G; j < a.n_inter; j += gridDim.x * GROUPS) {
        const size_t p0 = (size_t)j * (size_t)n;
        const float2 *yh2 = reinterpret_cast<const float2 *>(a.yhat) + p0;
        const int32_t *mp = LOGQ ? a.map + 2 * p0 : nullptr;
        const float lqpos = LOGQ ? a.lq[mp[0]] : 0.f;
        // a_q = -d_q - (lq[negative q] - lq[positive]); the correction is not evaluated without LOGQ
        const auto logit = [&](int q, const float2 yh) {
            float v = -(yh.x - yh.y);
            if (LOGQ) v -= a.lq[mp[2 * q + 1]] - lqpos;
            return v;
        };
        float amax = -INFINITY;
        int bad = 0;
        for (int q = l; q < n; q += G) {
            const float2 yh = yh2[q];
            amax = fmaxf(amax, logit(q, yh));
            if (!isfinite(yh.x - yh.y)) bad = 1;
            if (!isfinite(yh.x)) stbad += 1.f;
            if (!isfinite(yh.y)) stbad += 1.f;
        }
#pragma unroll
        for (int m = G / 2; m >= 1; m >>= 1) {
            amax = fmaxf(amax, __shfl_xor(amax, m, 64));
            bad |= __shfl_xor(bad, m, 64);
        }
        const float mx = fmaxf(0.f, amax);
        float z = 0.f;
        for (int q = l; q < n; q += G) z += expf(logit(q, yh2[q]) - mx);
#pragma unroll
        for (int m = G / 2; m >= 1; m >>= 1) z += __shfl_xor(z, m, 64);
        const float Z = expf(-mx) + z;
        for (int q = l; q < n; q += G) {
            const float pi = bad ? 0.f : expf(logit(q, yh2[q]) - mx) / Z;
            if (a.pi) a.pi[2 * (p0 + (size_t)q)] = pi;
            st2 = fmaf(2.f * pi, pi, st2);
        }
        if (l == 0 && !bad) {
            stl += (double)(mx + logf(Z));
            if (amax < 0.f) sttop += 1.0;
        }
    }
    double v[4] = {sttop, st2, stbad, stl};
    const int where[4] = {0, 1, 2, 3};
    pair_block_sums<4>(a.bsum, v, where);
}

int group_width(int32_t n) {
    int g = 1;
    while (g < n && g < 64) g <<= 1;
    return g;
}

template <int G>
void launch_g(const SoftmaxArgs &a, dim3 g, hipStream_t s) {
    if (a.lq) hipLaunchKernelGGL((k_softmax_pre<G, true>), g, dim3(kBlock), 0, s, a);
    else hipLaunchKernelGGL((k_softmax_pre<G, false>), g, dim3(kBlock), 0, s, a);
}

}  // namespace

int softmax_blocks(int32_t n, int64_t n_inter) { return grid_blocks(n_inter, kBlock / group_width(n), 8192); }

hipError_t launch_softmax_pre(const SoftmaxArgs &a, hipStream_t s, int *n_partials) {
    if (a.n < 1 || a.n_inter < 0 || !a.yhat || !a.bsum || (a.lq && !a.map)) return hipErrorInvalidValue;
    const int blocks = softmax_blocks(a.n, a.n_inter);
    if (n_partials) *n_partials = blocks;
    const dim3 g((unsigned)blocks);
    switch (group_width(a.n)) {
        case 1: launch_g<1>(a, g, s); break;
        case 2: launch_g<2>(a, g, s); break;
        case 4: launch_g<4>(a, g, s); break;
        case 8: launch_g<8>(a, g, s); break;
        case 16: launch_g<16>(a, g, s); break;
        case 32: launch_g<32>(a, g, s); break;
        default: launch_g<64>(a, g, s); break;
    }
    return hipGetLastError();
}

}  // namespace fmhip
