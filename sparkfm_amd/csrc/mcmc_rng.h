// mcmc_rng.h — the counter-based random numbers of the MCMC learner (include/fmhip_mcmc.h), shared by the host arithmetic
// (fmhip_host.cpp) and the noise kernel (als_kernels.hip): Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random
// numbers: as easy as 1, 2, 3", SC 2011), the two variates derived from one block of it, and the probit link's truncated
// normal (include/fmhip_mcmc_task.h), a bounded rejection loop over blocks of a stream of its own.  Integer arithmetic only up
// to u53; log / cos / sqrt are the caller's libm (host) or the device's (kernel), so host and device normals agree to a
// few ulp, not bit for bit.  Also here: the BPR trainer's negative rows (include/fmhip_bpr.h; fm_bpr.hip), integer arithmetic
// throughout, so those agree bit for bit — under the uniform proposal and under a weighted one (include/fmhip_proposal.h: an alias
// table the host builds).  No HIP header: g++ compiles it for the sanitizer harnesses.
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
enum { kStreamCoord = 0, kStreamW0 = 1, kStreamAlpha = 2, kStreamLambda = 3, kStreamMu = 4, kStreamTarget = 5, kStreamNegative = 6 };

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

// ---- the probit link's latent target (include/fmhip_mcmc_task.h) ----------------------------------------------------------------
constexpr int kTruncMaxAttempts = 64;

// z ~ N(0,1) conditioned on z > a, by rejection: attempt j = 0, 1, ... takes the block of counter (row, j, t, kStreamTarget),
// u1 = u53(x0, x1), u2 = u53(x2, x3).  a <= 0: the block's normal, accepted if z > a (at least every second attempt is);
// a > 0: Robert's exponential proposal (C. P. Robert, "Simulation of truncated normal variables", 1995), z = a - ln(u1) / l with
// l = (a + sqrt(a^2 + 4)) / 2, accepted if u2 <= exp(-(z - l)^2 / 2) (at least 0.76 of the attempts are).  The last attempt's
// proposal is taken unconditionally (a <= 0: as |z|, which is > a), so the loop is bounded whatever a holds — a NaN included.
// *attempts (nullable): how many blocks the draw took.  No fused multiply-add.
FMHIP_RNG_FN double truncated_normal(uint64_t seed, uint32_t row, uint32_t t, double a, int *attempts) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double l = (a + sqrt(a * a + 4.0)) / 2.0;
    double z = 0.0;
    int j = 0;
    for (; j < kTruncMaxAttempts; ++j) {
        const Block b = block_of(seed, row, (uint32_t)j, t, kStreamTarget);
        const double u1 = u53(b.x[0], b.x[1]), u2 = u53(b.x[2], b.x[3]);
        if (a <= 0.0) {
            z = sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
            if (z > a) break;
            if (j == kTruncMaxAttempts - 1) z = fabs(z);
        } else {
            z = a - log(u1) / l;
            const double d = z - l;
            if (u2 <= exp(-0.5 * (d * d))) break;
        }
    }
    if (attempts) *attempts = j < kTruncMaxAttempts ? j + 1 : kTruncMaxAttempts;
    return z;
}

// E[z | z > a] for z ~ N(0,1): phi(a) / Q(a), Q(a) = erfc(a / sqrt 2) / 2.  Past a = 30 both terms head for the subnormals and the
// asymptote a + 1 / a takes over (it is 2 / a^3 above the quotient there: 3e-6 relative)
FMHIP_RNG_FN double truncated_normal_mean(double a) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (a > 30.0) return a + 1.0 / a;
    return exp(-0.5 * (a * a)) * 0.3989422804014327 / (0.5 * erfc(a / 1.4142135623730951));
}

// Phi(x) = erfc(-x / sqrt 2) / 2: the probability a probit score stands for
FMHIP_RNG_FN double normal_cdf(double x) { return 0.5 * erfc(-x / 1.4142135623730951); }

// ---- the BPR trainer's negative rows (include/fmhip_bpr.h) ------------------------------------------------------------------------
constexpr int kNegMaxAttempts = 64;

// the block of words a negative's attempts share: counter (p, group, t, kStreamNegative) — the samplers' one site
FMHIP_RNG_FN Block negative_block(uint64_t seed, uint32_t p, uint32_t group, uint32_t t) { return block_of(seed, p, group, t, kStreamNegative); }

// is row c in the ascending list?
FMHIP_RNG_FN bool row_listed(const int32_t *list, int32_t len, int32_t c) {
    int32_t lo = 0, hi = len;
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (list[mid] < c) lo = mid + 1;
        else hi = mid;
    }
    return lo < len && list[lo] == c;
}

// A row of [0, M) outside `list` (ascending, distinct, fewer than M entries: the caller has checked) for pair p at epoch t, by
// rejection: attempt a = 0 .. 63 takes word a & 3 of the block of counter (p, a >> 2, t, kStreamNegative), c = (word * M) >> 32,
// accepted if c is not listed.  All 64 rejected: from the last c on, c = (c + 1) mod M until c is not listed (at most len steps);
// *forced = 1.  *attempts: the attempts made (1 .. 64).  Integer arithmetic only: host and device agree bit for bit.
// group0 is added to the counter's group word: candidate c of the adaptive sampler (include/fmhip_bpr_adaptive.h) draws with
// group0 = c << 4, so its 16 blocks are its own and candidate 0 is the uniform sampler's draw.
FMHIP_RNG_FN int32_t negative_row(uint64_t seed, uint32_t p, uint32_t t, uint32_t M, const int32_t *list, int32_t len, int *attempts, int *forced,
                                  uint32_t group0 = 0) {
    int32_t c = 0;
    Block b{};
    for (int a = 0; a < kNegMaxAttempts; ++a) {
        if ((a & 3) == 0) b = negative_block(seed, p, group0 | (uint32_t)(a >> 2), t);
        c = (int32_t)(((uint64_t)b.x[a & 3] * M) >> 32);
        if (!row_listed(list, len, c)) {
            *attempts = a + 1;
            *forced = 0;
            return c;
        }
    }
    for (int32_t i = 0; i <= len && row_listed(list, len, c); ++i) c = (uint32_t)(c + 1) == M ? 0 : c + 1;
    *attempts = kNegMaxAttempts;
    *forced = 1;
    return c;
}

// ---- ... drawn from a weighted proposal (include/fmhip_proposal.h) ------------------------------------------------------------------
constexpr int kPropMaxAttempts = 32;

// one bucket of the alias table (Walker / Vose): 8 bytes, read with one load.  A bucket that is never redirected has alias = its
// own index, so both sides of the comparison give it and no threshold of 2^32 is needed.
struct alignas(8) AliasEntry {
    uint32_t thresh;      // floor(p * 2^32), at most 2^32 - 1: the bucket keeps its own row when the second word is below it
    int32_t alias;        // the row it gives otherwise, in [0, M)
};

// negative_row's sibling under a weighted proposal: attempt a = 0 .. 31 takes the words x0 = x[2 (a & 1)], x1 = x[2 (a & 1) + 1] of
// the block of counter (p, group0 | (a >> 1), t, kStreamNegative) — two attempts a block, 16 blocks a candidate, the c << 4 spacing
// of the walk — j = (x0 * M) >> 32, c = x1 < tab[j].thresh ? j : tab[j].alias, accepted if c is not listed.  All 32 rejected: the
// forced walk of negative_row from the last c on; *forced = 1.  *attempts: 1 .. 32.  tab: M entries, every alias in [0, M).
FMHIP_RNG_FN int32_t proposal_row(uint64_t seed, uint32_t p, uint32_t t, uint32_t M, const AliasEntry *tab, const int32_t *list, int32_t len,
                                  int *attempts, int *forced, uint32_t group0 = 0) {
    int32_t c = 0;
    Block b{};
    for (int a = 0; a < kPropMaxAttempts; ++a) {
        if ((a & 1) == 0) b = negative_block(seed, p, group0 | (uint32_t)(a >> 1), t);
        const uint32_t x0 = (a & 1) ? b.x[2] : b.x[0], x1 = (a & 1) ? b.x[3] : b.x[1];
        const uint32_t j = (uint32_t)(((uint64_t)x0 * M) >> 32);
        const AliasEntry e = tab[j];
        c = x1 < e.thresh ? (int32_t)j : e.alias;
        if (!row_listed(list, len, c)) {
            *attempts = a + 1;
            *forced = 0;
            return c;
        }
    }
    for (int32_t i = 0; i <= len && row_listed(list, len, c); ++i) c = (uint32_t)(c + 1) == M ? 0 : c + 1;
    *attempts = kPropMaxAttempts;
    *forced = 1;
    return c;
}

}  // namespace rng
}  // namespace fmhip
