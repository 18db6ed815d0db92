// mcmc_rng.h — the counter-based random numbers of the MCMC learner (include/fmhip_mcmc.h), shared by the host arithmetic
// (fmhip_host.cpp) and the noise kernel (als_kernels.hip): Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random
// numbers: as easy as 1, 2, 3", SC 2011) and the two variates derived from one block of it.  Integer arithmetic only up
// to u53; log / cos / sqrt are the caller's libm (host) or the device's (kernel), so host and device normals agree to a
// few ulp, not bit for bit.  No HIP header: g++ compiles it for the sanitizer harnesses.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIP__)
#define FMHIP_RNG_FN __host__ __device__ inline
#else
#define FMHIP_RNG_FN inline
#endif

namespace fmhip {
namespace rng {

// the streams of a counter (index, group, t, stream): what a draw is for
enum { kStreamCoord = 0, kStreamW0 = 1, kStreamAlpha = 2, kStreamLambda = 3, kStreamMu = 4 };

struct Block { uint32_t x[4]; };

FMHIP_RNG_FN Block philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    Block b;
    b.x[0] = c0; b.x[1] = c1; b.x[2] = c2; b.x[3] = c3;
    return b;
}

// 53 bits of (a, b), a the high word, as a double in (0, 1]: never 0 (its log is taken); the top word rounds to 1
FMHIP_RNG_FN double u53(uint32_t a, uint32_t b) {
    const uint64_t w = ((uint64_t)a << 32 | b) >> 11;
    return ((double)w + 0.5) * 0x1p-53;
}

FMHIP_RNG_FN Block block_of(uint64_t seed, uint32_t index, uint32_t group, uint32_t t, uint32_t stream) {
    return philox4x32_10(index, group, t, stream, (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32));
}

FMHIP_RNG_FN double uniform(uint64_t seed, uint32_t index, uint32_t group, uint32_t t, uint32_t stream) {
    const Block b = block_of(seed, index, group, t, stream);
    return u53(b.x[0], b.x[1]);
}

// Box-Muller, the cosine branch only: one normal per counter
FMHIP_RNG_FN double normal(uint64_t seed, uint32_t index, uint32_t group, uint32_t t, uint32_t stream) {
    const Block b = block_of(seed, index, group, t, stream);
    return sqrt(-2.0 * log(u53(b.x[0], b.x[1]))) * cos(6.283185307179586 * u53(b.x[2], b.x[3]));
}

}  // namespace rng
}  // namespace fmhip
