// als_kernels.hip — SparkFM's own learner, ALS / coordinate descent (S/fm/lib/ALS.scala:15-75,
// 152-198), on the GPU in fp64.
//
// The algorithm is Gauss-Seidel over the features: every closed-form update sees the residuals
// left by the previous one, so features are visited strictly in order by ONE persistent
// workgroup; the parallelism is inside a column (its entries are spread over the 1024 threads,
// sums are tree-reduced in a fixed order).  All arithmetic is fp64 without fma contraction — the
// reference runs on the JVM, which never fuses — so an epoch tracks the fp64 oracle to ~1e-13.
// Four shapes of the sweep, chosen per epoch in this order (walk_choice, epoch_tail):
//  * k_als_level — the level schedule, when the dataset has one and its levels are wide (one-hot fields): the columns of a
//    level share no row, so they take a wave each side by side, a launch per level and parameter group.
//  * k_als_sweep_lds — residuals e and the factor's q live in LDS (n_rows * 16 B <= 160,000 B: BASELINE config 1's
//    10,000 rows fill it exactly); ONE wave walks the columns (a column of ~100 entries is two wave-iterations: no
//    workgroup barrier per feature, wave sums by DPP row reductions), the next column's entries are prefetched
//    while the current one is reduced.
//  Larger datasets keep e and q in global memory and follow a launch plan made from the column lengths:
//  * k_als_cols_wg — a RUN of consecutive short columns by one workgroup (~3 barriers per column);
//  * k_als_col_sums + k_als_col_update — ONE long column (>= kAlsLongColumn entries) on the whole chip: every
//    workgroup sums its slice (sum h^2, sum e*h), the second launch adds the partials in a fixed tree (every workgroup
//    the same bits), forms theta* and updates its slice of e and q.  The dependency between consecutive columns is the
//    launch boundary — no device-side grid barrier to get wrong.  A column of 10^5 entries costs a CPU core ~0.2 ms per
//    step and this path two launches.  (A level's long columns take it too, behind the level's launch.)
// Every factor's q comes from one up-front pass over the feature-sorted rows (k_als_q_all), the per-row order of the
// reference's transposed pass.
// The MCMC learner (include/fmhip_mcmc.h) walks the same columns with the Gaussian conditional's draw in computeTheta's place:
// every walk takes a parameter pack that is empty for ALS and holds the epoch's McmcDev / McmcGroupDev for MCMC, so the ALS
// kernels keep their arguments and their code.  Its own kernels — the noise, the probit targets, the hyper-parameter sums, the
// test rows' accumulation — sit beside the walks' in the first section.
// The second section is the block-structure sweep over relational data (include/fmhip_mcmc_relational.h; launchers: mcmc_blocks.h):
// the same conditional on a block's columns with the sums taken over the BLOCK's rows from per-row caches.  It shares this file's
// anonymous-namespace device functions (the draw, the sums, the probit residual), the walk choice and — for the plain part — the
// per-group pass.
#include "als_kernels.h"
#include "fm_relational.h"
#include "mcmc_blocks.h"
#include "mcmc_rng.h"

#include <cstdlib>

namespace fmhip {
namespace {

// S/fm/lib/ALS.scala:190-192
__device__ __forceinline__ bool is_updatable(double nv, double ov) { return !isnan(nv) && !isinf(nv) && nv != ov; }

// S/fm/lib/ALS.scala:167-176
__device__ __forceinline__ double compute_theta(double theta, double reg, double sum_e_h, double sum_h_sqr) {
#pragma clang fp contract(off)
    const double theta_new = -(sum_e_h - theta * sum_h_sqr) / (reg + sum_h_sqr);
    return is_updatable(theta_new, theta) ? theta_new : theta;
}

// The closed-form step of one coordinate as a value: what the walks below call where ALS.scala calls computeTheta.
//  * DrawAls  — computeTheta itself (the ALS epoch: the arithmetic it always had);
//  * DrawMcmc — libFM's Gaussian conditional (include/fmhip_mcmc.h): precision lambda + alpha sum h^2, its mean, and (sample)
//    the coordinate's own N(0,1) scaled by 1 / sqrt(precision).  With alpha = 1, mu = 0, sample off it rounds exactly as
//    computeTheta does (1 * x and x - 0 are exact): ALS = MCMC without sampling, bit for bit.
struct DrawAls {
    double reg;
    __device__ __forceinline__ double operator()(double theta, double sum_e_h, double sum_h_sqr, double) const {
        return compute_theta(theta, reg, sum_e_h, sum_h_sqr);
    }
    __device__ __forceinline__ const DrawAls &at(int64_t) const { return *this; }      // the step of feature i: the same for every feature
};

struct DrawMcmc {
    double alpha, lambda, mu;
    bool sample;
    __device__ __forceinline__ double operator()(double theta, double sum_e_h, double sum_h_sqr, double z) const {
#pragma clang fp contract(off)
        const double prec = lambda + alpha * sum_h_sqr;
        const double mean = -(alpha * (sum_e_h - theta * sum_h_sqr) - mu * lambda) / prec;
        const double theta_new = sample ? mean + z / sqrt(prec) : mean;      // (no `+ 0 * sigma` without sampling)
        return is_updatable(theta_new, theta) ? theta_new : theta;
    }
    __device__ __forceinline__ const DrawMcmc &at(int64_t) const { return *this; }
};

// ... with attribute groups (include/fmhip_mcmc_groups.h): the step is per column — feature i takes the lambda and the mu of its
// group.  lambda / mu: parameter group g's rows of the state, G values each.
struct DrawMcmcGroups {
    double alpha;
    const double *lambda, *mu;
    const int32_t *group;
    bool sample;
    __device__ __forceinline__ DrawMcmc at(int64_t i) const {
        const int32_t a = group[i];
        return DrawMcmc{alpha, lambda[a], mu[a], sample};
    }
};

// Every walk below takes a parameter pack M that is EMPTY for the ALS epoch — its kernels keep the signatures, the kernel
// arguments and the code they always had — and holds one McmcDev for the MCMC epoch; the overloads pick the step by it.
// The draw of parameter group g (0: w, 1 + f: factor f); m.hyp = {alpha, lambda[k + 1], mu[k + 1]}
__device__ __forceinline__ DrawAls group_draw(const AlsArgs &, int, double reg) { return DrawAls{reg}; }
__device__ __forceinline__ DrawMcmc group_draw(const AlsArgs &a, int g, double, const McmcDev &m) {
    return DrawMcmc{m.hyp[0], m.hyp[1 + g], m.hyp[2 + a.k + g], m.sample != 0};
}

__device__ __forceinline__ DrawMcmcGroups group_draw(const AlsArgs &a, int g, double, const McmcGroupDev &m) {
    const int64_t G = m.n_groups;
    return DrawMcmcGroups{m.hyp[0], m.hyp + 1 + g * G, m.hyp + 1 + (a.k + 1 + g) * G, m.group, m.sample != 0};
}

// the noise of entry idx of m.z (k_mcmc_noise filled it before the epoch's first dependent launch); of a long column's own step
// (a McmcGroupDev is a McmcDev here and in the bias step)
__device__ __forceinline__ double noise_at(int64_t) { return 0.0; }
__device__ __forceinline__ double noise_at(int64_t idx, const McmcDev &m) { return m.z[idx]; }
__device__ __forceinline__ double noise_own() { return 0.0; }
__device__ __forceinline__ double noise_own(const McmcDev &m) { return m.z[m.zi]; }

// the bias step: computeTheta(w0, reg0, sum e, size) / the conditional with h = 1, lambda = reg0, mu = 0 (its noise sits behind
// the coordinates'; the bias has no group: alpha is hyp[0] in both layouts)
__device__ __forceinline__ double bias_step(const AlsArgs &a, double w0, double se) { return compute_theta(w0, a.reg0, se, (double)a.n_rows); }
__device__ __forceinline__ double bias_step(const AlsArgs &a, double w0, double se, const McmcDev &m) {
    return DrawMcmc{m.hyp[0], a.reg0, 0.0, m.sample != 0}(w0, se, (double)a.n_rows, m.z[(int64_t)(a.k + 1) * a.n_cols]);
}

// FMModel.predict's exact order of operations (S/fm/FMModel.scala:34-63) for row r: sequential sums in stored order
__device__ __forceinline__ double row_predict(const AlsArgs &a, int64_t r) {
#pragma clang fp contract(off)
    const int64_t p0 = a.row_ptr[r], p1 = a.row_ptr[r + 1];
    double result = 0.0;
    result += *a.w0;
    if (p1 > p0) {
        double lin = a.w[a.col[p0]] * a.val[p0];
        for (int64_t p = p0 + 1; p < p1; ++p) lin += a.w[a.col[p]] * a.val[p];
        result += lin;
        for (int f = 0; f < a.k; ++f) {
            double t = a.v[f + (int64_t)a.col[p0] * a.k] * a.val[p0];
            double sum_f = t, sum_sqr_f = t * t;
            for (int64_t p = p0 + 1; p < p1; ++p) {
                t = a.v[f + (int64_t)a.col[p] * a.k] * a.val[p];
                sum_f += t;
                sum_sqr_f += t * t;
            }
            result += 0.5 * (sum_f * sum_f - sum_sqr_f);
        }
    }
    return result;
}

// ALS.precomputeTermE (S/fm/lib/ALS.scala:142-144): one thread per row
__global__ __launch_bounds__(256) void k_als_residual(AlsArgs a) {
#pragma clang fp contract(off)
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < a.n_rows; r += (int64_t)gridDim.x * 256) a.e[r] = row_predict(a, r) - a.y[r];
}

// The probit link's latent targets (include/fmhip_mcmc_task.h), in the place of the epoch's first residual pass: per row the
// forward, the target y* the whole epoch trains on — p.ystar, which a.y points at — and the residual e = yhat - y*.  The sign
// s = +1 / -1 is that of the label's class [y > 0].  p.mode kProbitStart (the handle's first epoch): y* = s; kProbitSample:
// y* = yhat + s z, z the row's own truncated normal (z > -s yhat; counter (row, attempt, t, kStreamTarget): no schedule enters it);
// kProbitMean: z is that draw's expectation.  A wave waits for the lane with the most attempts — 64 at the most, by construction.
// probit_residual: row r's target around the forward yhat into p.ystar -> its residual (the block sweep's combine calls it too)
__device__ __forceinline__ double probit_residual(const McmcProbit &p, int64_t r, double yhat, uint64_t seed, uint32_t t) {
#pragma clang fp contract(off)
    const double s = p.labels[r] > 0.0 ? 1.0 : -1.0;
    double target = s;
    if (p.mode != kProbitStart) {
        const double lo = -s * yhat;
        const double z = p.mode == kProbitSample ? rng::truncated_normal(seed, (uint32_t)r, t, lo, nullptr) : rng::truncated_normal_mean(lo);
        target = yhat + s * z;
    }
    p.ystar[r] = target;
    return yhat - target;
}

__global__ __launch_bounds__(256) void k_mcmc_probit_targets(AlsArgs a, McmcProbit p, uint64_t seed, uint32_t t) {
#pragma clang fp contract(off)
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < a.n_rows; r += (int64_t)gridDim.x * 256) a.e[r] = probit_residual(p, r, row_predict(a, r), seed, t);
}

// The MCMC learner's averaged prediction.  The test rows' predictions under the draw the epoch left are k_als_residual's own —
// launched on the test rows with labels of zero, e = yhat - 0 is yhat exactly — written to `last`; this adds them to the running sum.
__global__ __launch_bounds__(256) void k_mcmc_accumulate(const double *last, double *sum, int64_t n_rows) {
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n_rows; r += (int64_t)gridDim.x * 256) sum[r] += last[r];
}

// ... and what a draw's prediction becomes before it joins the sum and `last` under a task (include/fmhip_mcmc_task.h): the
// probability Phi(yhat) of the probit link, or the score clamped to the range the caller gave
struct LinkProbit {
    __device__ __forceinline__ double operator()(double yhat) const { return rng::normal_cdf(yhat); }
};
struct LinkClamp {
    double lo, hi;
    __device__ __forceinline__ double operator()(double yhat) const { return yhat < lo ? lo : yhat > hi ? hi : yhat; }
};
template <class Link>
__global__ __launch_bounds__(256) void k_mcmc_accumulate_link(double *last, double *sum, int64_t n_rows, Link link) {
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n_rows; r += (int64_t)gridDim.x * 256) {
        const double p = link(last[r]);
        last[r] = p;
        sum[r] += p;
    }
}

// fixed-order block sum of two doubles; result valid in every thread
template <int kAlsBlock>
__device__ __forceinline__ void block_sum2(double &x, double &y, double (*sh)[kAlsBlock / 64]) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        x += __shfl_xor(x, m, 64);
        y += __shfl_xor(y, m, 64);
    }
    const int wv = threadIdx.x >> 6;
    __syncthreads();   // sh may still be read from the previous call
    if ((threadIdx.x & 63) == 0) { sh[0][wv] = x; sh[1][wv] = y; }
    __syncthreads();
    double tx = 0.0, ty = 0.0;
#pragma unroll
    for (int i = 0; i < kAlsBlock / 64; ++i) { tx += sh[0][i]; ty += sh[1][i]; }
    x = tx;
    y = ty;
}

// The N(0,1) of every coordinate the epoch will draw — z[g * n_cols + s] for column slot s of group g, then the bias's — in one
// chip-wide launch before anything else: a draw depends on its counter only, so none of it sits on the sweep's dependent chain.
__global__ __launch_bounds__(256) void k_mcmc_noise(AlsArgs a, double *z, uint64_t seed, uint32_t t) {
    const int64_t total = (int64_t)(a.k + 1) * a.n_cols;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx <= total; idx += (int64_t)gridDim.x * 256) {
        if (idx == total) {
            z[idx] = rng::normal(seed, 0u, 0u, t, rng::kStreamW0);
        } else {
            const uint32_t g = (uint32_t)(idx / a.n_cols);
            z[idx] = rng::normal(seed, (uint32_t)a.cfeat[idx % a.n_cols], g, t, rng::kStreamCoord);
        }
    }
}

// What the hyper-parameter draws need, in one launch of fixed-order reductions: quantity 0 = sum e^2 over the rows, quantity
// 1 + g = {sum theta_i, sum (theta_i - mu_g)^2} over group g's trained parameters (the column slots with id < num_attribute;
// mu_g: the mean the epoch starts from, m.hyp).  Every quantity is cut into P contiguous chunks, a workgroup each:
// out[2 * (quantity * P + chunk)], + 1 — the host adds a quantity's P partials in order.  All groups at epoch start: nothing
// writes w, or column f of V, before that group's own sweep (the argument that lets k_als_q_all run up front).
constexpr int kSumsBlock = 256;

// this thread's share of {sum theta, sum (theta - mu)^2} of parameter group g over chunk `chunk` of P of the column slots: the
// slots lo + tid, lo + tid + kSumsBlock, ... that trained(s) keeps
template <class Trained>
__device__ __forceinline__ void theta_sums(const AlsArgs &a, int g, double mu, int chunk, int P, int tid, Trained trained, double &s0, double &s1) {
#pragma clang fp contract(off)
    const int64_t lo = (int64_t)a.n_cols * chunk / P, hi = (int64_t)a.n_cols * (chunk + 1) / P;
    for (int64_t s = lo + tid; s < hi; s += kSumsBlock) {
        if (!trained(s)) continue;
        const int64_t i = a.cfeat[s];
        const double th = g == 0 ? a.w[i] : a.v[(g - 1) + i * a.k];
        const double d = th - mu;
        s0 += th;
        s1 += d * d;
    }
}

__global__ __launch_bounds__(kSumsBlock) void k_mcmc_sums(AlsArgs a, McmcDev m, double *out, int P) {
#pragma clang fp contract(off)
    __shared__ double sh[2][kSumsBlock / 64];
    const int quantity = (int)blockIdx.x / P, chunk = (int)blockIdx.x % P, tid = threadIdx.x;
    double s0 = 0.0, s1 = 0.0;
    if (quantity == 0) {
        const int64_t lo = a.n_rows * chunk / P, hi = a.n_rows * (chunk + 1) / P;
        for (int64_t r = lo + tid; r < hi; r += kSumsBlock) {
            const double e = a.e[r];
            s0 += e * e;
        }
    } else {
        const int g = quantity - 1;                                // (quirk Q1: slot n is never trained)
        theta_sums(a, g, m.hyp[2 + a.k + g], chunk, P, tid, [&](int64_t s) { return a.cfeat[s] < a.num_attribute; }, s0, s1);
    }
    block_sum2<kSumsBlock>(s0, s1, sh);
    if (tid == 0) {
        out[2 * (int64_t)blockIdx.x] = s0;
        out[2 * (int64_t)blockIdx.x + 1] = s1;
    }
}

// The same sums per (parameter group g, attribute group a) of a handle with groups (include/fmhip_mcmc_groups.h): (k + 1) * G
// pairs.  A workgroup per (g, a) would be tens of thousands of tiny workgroups, each striding V by k; here a workgroup takes one
// CHUNK of the host's plan — at most kMcmcGroupChunk trained slots of ONE attribute group, in the plan's stable order — and
// produces the chunk's partial pair of all k + 1 parameter groups.  The block is cut into S = 256 / L sub-groups of L = the power
// of two >= k + 1 (at most 256) lanes: lane j of a sub-group owns parameter group g = j (w at j = 0, then the feature's V row,
// read contiguously by the sub-group's lanes), sub-group u adds the chunk's slots u, u + S, u + 2S ... in that order, and lane j of
// sub-group 0 adds the S sub-sums in order through LDS.  k + 1 = 257 takes a second pass.  No atomics; the order of every
// addition is fixed by (chunk, k) alone, so neither the CU count nor the launch schedule enters the result.
constexpr int kGroupSumsBlock = 256;
__global__ __launch_bounds__(kGroupSumsBlock) void k_mcmc_group_sums(AlsArgs a, McmcGroupDev m, McmcGroupSums plan) {
#pragma clang fp contract(off)
    __shared__ double sh[2][kGroupSumsBlock];
    const int chunk = (int)blockIdx.x, tid = threadIdx.x, k1 = a.k + 1;
    if (chunk >= plan.n_chunks) return;
    int L = 1;
    while (L < k1 && L < kGroupSumsBlock) L <<= 1;
    const int S = kGroupSumsBlock / L, u = tid / L, j = tid % L;
    const int lo = plan.chunk_ptr[chunk], hi = plan.chunk_ptr[chunk + 1];
    const int64_t G = m.n_groups;
    const int32_t ag = plan.chunk_group[chunk];
    for (int g0 = 0; g0 < k1; g0 += L) {
        const int g = g0 + j;
        double s0 = 0.0, s1 = 0.0;
        if (g < k1) {
            const double mu = m.hyp[1 + (k1 + g) * G + ag];
            for (int p = lo + u; p < hi; p += S) {
                const int64_t i = a.cfeat[plan.order[p]];          // trained by the plan's construction: i < num_attribute
                const double th = g == 0 ? a.w[i] : a.v[(g - 1) + i * a.k];
                const double d = th - mu;
                s0 += th;
                s1 += d * d;
            }
        }
        __syncthreads();                                           // sh may still be read from the previous pass
        sh[0][tid] = s0;
        sh[1][tid] = s1;
        __syncthreads();
        if (u == 0 && g < k1) {
            double t0 = 0.0, t1 = 0.0;
            for (int x = 0; x < S; ++x) {
                t0 += sh[0][x * L + j];
                t1 += sh[1][x * L + j];
            }
            plan.out[2 * ((int64_t)chunk * k1 + g)] = t0;
            plan.out[2 * ((int64_t)chunk * k1 + g) + 1] = t1;
        }
    }
}

// drawGlobalBias :152-154 = computeTheta(w0, reg0, sum e, size) and `fm.w0 = w0` (:19-27) — once per epoch, one workgroup.
// The residuals are NOT shifted here: as Spark evaluates :23-31 the lazy `error` RDD is materialised after `fm.w0 = w0`, so
// its `fm.predict` already carries the new bias and the mapped term `w0 - fm.w0` is zero — the
// launcher simply runs k_als_residual again with the new bias.
template <int kAlsBlock, class... M>
__global__ __launch_bounds__(kAlsBlock) void k_als_w0(AlsArgs a, M... m) {
#pragma clang fp contract(off)
    __shared__ double sh[2][kAlsBlock / 64];
    const int tid = threadIdx.x;
    double se = 0.0, dummy = 0.0;
    for (int64_t r = tid; r < a.n_rows; r += kAlsBlock) se += a.e[r];
    block_sum2<kAlsBlock>(se, dummy, sh);
    const double w0 = *a.w0;
    const double w0n = bias_step(a, w0, se, m...);
    if (tid == 0) *a.w0 = w0n;
}

// The closed-form steps of the consecutive columns [s_lo, s_hi) by ONE workgroup, in order (S/fm/lib/ALS.scala:36-43
// linear weights, :52-68 factor f): the run of SHORT columns between two long ones.  e and q in global memory.
template <int kAlsBlock, bool FACTOR, class... M>   // threads: 256 for short columns (cheaper barriers), 1024 for longer ones
__global__ __launch_bounds__(kAlsBlock) void k_als_cols_wg(AlsArgs a, double *q, int s_lo, int s_hi, int f, M... m) {
#pragma clang fp contract(off)
    __shared__ double sh[2][kAlsBlock / 64];
    const int tid = threadIdx.x;
    const int k = a.k;
    const int g = FACTOR ? 1 + f : 0;
    const auto draw = group_draw(a, g, FACTOR ? a.regv : a.regw, m...);
    for (int s = s_lo; s < s_hi; ++s) {
        const int64_t i = a.cfeat[s];
        if (i >= a.num_attribute) continue;                       // `0 until num_attribute` (quirk Q1: slot n is never trained)
        const int c0 = a.cptr[s], c1 = a.cptr[s + 1];
        double *par = FACTOR ? a.v + f + i * k : a.w + i;
        const double th = *par;
        const double zn = noise_at((int64_t)g * a.n_cols + s, m...);
        const auto &step = draw.at(i);                            // (with attribute groups: requested before the column is reduced)
        double shs = 0.0, seh = 0.0;
        for (int p = c0 + tid; p < c1; p += kAlsBlock) {
            const uint32_t r = a.crow[p] & 0x7fffffffu;
            const double x = a.cval[p];
            const double h = FACTOR ? x * q[r] - x * x * th : x;      // :56-58 / :40
            shs += h * h;
            seh += a.e[r] * h;
        }
        block_sum2<kAlsBlock>(shs, seh, sh);
        const double tn = step(th, seh, shs, zn);
        const double d = tn - th;
        const bool upd = is_updatable(tn, th);
        for (int p = c0 + tid; p < c1; p += kAlsBlock) {
            const uint32_t r = a.crow[p] & 0x7fffffffu;
            const double x = a.cval[p];
            if (upd) {
                const double h = FACTOR ? x * q[r] - x * x * th : x;
                a.e[r] += h * d;                                  // updateError :194-198
            }
            if (FACTOR) q[r] += x * d;                            // :60-62
        }
        __syncthreads();
        if (tid == 0) *par = tn;                                  // :40 / :64
        __syncthreads();
    }
}

// ---- one LONG column on the whole chip: two launches -------------------------------------------------
constexpr int kColBlock = 256;

// launch 1: workgroup g sums its contiguous slice of the column -> part[2g], part[2g + 1]; part[2G] = theta
template <bool FACTOR>
__global__ __launch_bounds__(kColBlock) void k_als_col_sums(AlsArgs a, const double *q, int c0, int c1, int64_t i, int f) {
#pragma clang fp contract(off)
    __shared__ double sh[2][kColBlock / 64];
    const int tid = threadIdx.x, G = (int)gridDim.x;
    const int per = (c1 - c0 + G - 1) / G;
    const int lo = c0 + (int)blockIdx.x * per, hi = lo + per < c1 ? lo + per : c1;
    const double th = FACTOR ? a.v[f + i * a.k] : a.w[i];
    double shs = 0.0, seh = 0.0;
    for (int p = lo + tid; p < hi; p += kColBlock) {
        const uint32_t r = a.crow[p] & 0x7fffffffu;
        const double x = a.cval[p];
        const double h = FACTOR ? x * q[r] - x * x * th : x;
        shs += h * h;
        seh += a.e[r] * h;
    }
    block_sum2<kColBlock>(shs, seh, sh);
    if (tid == 0) {
        a.part[2 * blockIdx.x] = shs;
        a.part[2 * blockIdx.x + 1] = seh;
        if (blockIdx.x == 0) a.part[2 * G] = th;      // the update launch must not read a parameter another workgroup is writing
    }
}

// launch 2: every workgroup adds the G partials in the same fixed tree (the same bits everywhere), forms theta* and
// updates its slice of e (and q); workgroup 0 stores the parameter
template <bool FACTOR, class... M>
__global__ __launch_bounds__(kColBlock) void k_als_col_update(AlsArgs a, double *q, int c0, int c1, int64_t i, int f, M... m) {
#pragma clang fp contract(off)
    __shared__ double sh[2][kColBlock / 64];
    const int tid = threadIdx.x, G = (int)gridDim.x;
    double shs = 0.0, seh = 0.0;
    for (int g = tid; g < G; g += kColBlock) {       // G <= kAlsMaxParts = 2 * kColBlock: at most two terms per thread
        shs += a.part[2 * g];
        seh += a.part[2 * g + 1];
    }
    block_sum2<kColBlock>(shs, seh, sh);
    const double th = a.part[2 * G];
    const double tn = group_draw(a, FACTOR ? 1 + f : 0, FACTOR ? a.regv : a.regw, m...).at(i)(th, seh, shs, noise_own(m...));
    const double d = tn - th;
    const bool upd = is_updatable(tn, th);
    const int per = (c1 - c0 + G - 1) / G;
    const int lo = c0 + (int)blockIdx.x * per, hi = lo + per < c1 ? lo + per : c1;
    for (int p = lo + tid; p < hi; p += kColBlock) {
        const uint32_t r = a.crow[p] & 0x7fffffffu;       // the rows of a column are distinct (als_dup is refused): no two writers
        const double x = a.cval[p];
        if (upd) {
            const double h = FACTOR ? x * q[r] - x * x * th : x;
            a.e[r] += h * d;
        }
        if (FACTOR) q[r] += x * d;
    }
    if (blockIdx.x == 0 && tid == 0) {
        if (FACTOR) a.v[f + i * a.k] = tn;
        else a.w[i] = tn;
    }
}


// precomputeTermQ (S/fm/lib/ALS.scala:146-150) of EVERY factor before the sweeps, on the whole chip: q_f only
// reads v[f, :], which nothing modifies before factor f's own sweep.  One thread per (row, factor); a row's terms
// are added in ascending feature order (the feature-sorted copy of the rows) — the order of the reference's
// transposed pass.  qall[f * n_rows + r].
__global__ __launch_bounds__(256) void k_als_q_all(AlsArgs a, double *qall) {
#pragma clang fp contract(off)
    const int64_t total = a.n_rows * a.k;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t r = idx / a.k;
        const int f = (int)(idx % a.k);
        double qv = 0.0;
        for (int64_t p = a.row_ptr[r]; p < a.row_ptr[r + 1]; ++p) qv += a.v[f + (int64_t)a.scol[p] * a.k] * a.sval[p];
        qall[(int64_t)f * a.n_rows + r] = qv;
    }
}

// ---- LDS-resident sweep -------------------------------------------------------------------------------
constexpr int kLdsSweepThreads = 1024;
constexpr int kLevelBlock = 256;            // level sweep: four waves = four columns per workgroup
constexpr size_t kAlsLdsBytes = 160000;     // e + q of at most 10,000 rows (the static reduction scratch fits beside it)

template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

// sum over the 64 lanes, identical in every lane; fixed order: quad butterfly, half-row and row mirrors on
// the vector ALU (DPP), then the four row sums through scalar registers
__device__ __forceinline__ double wave_sum(double v) {
#pragma clang fp contract(off)
    v += dpp_f64<0xB1>(v);     // quad_perm:[1,0,3,2]
    v += dpp_f64<0x4E>(v);     // quad_perm:[2,3,0,1]
    v += dpp_f64<0x141>(v);    // row_half_mirror
    v += dpp_f64<0x140>(v);    // row_mirror
    double r[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
        r[i] = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 16 * i), __builtin_amdgcn_readlane(__double2loint(v), 16 * i));
    return (r[0] + r[1]) + (r[2] + r[3]);
}

// The first 128 entries of a column as one wave holds them: lane l has entries l and 64 + l (raw CSC words: bit 31 of
// a row word still carries the column-start flag).  Loaded a step ahead, at clamped addresses and without touching the
// values, so that the requests stay in flight across the step (a mask or a branch on a loaded value makes the
// compiler wait for it on the spot).
struct ColHead {
    uint32_t r0, r1;
    double x0, x1;
};

__device__ __forceinline__ ColHead load_head(const AlsArgs &a, int c0, int lane) {
    const int64_t last = a.nnz - 1;
    const int64_t p0 = (int64_t)c0 + lane < last ? (int64_t)c0 + lane : last;
    const int64_t p1 = (int64_t)c0 + 64 + lane < last ? (int64_t)c0 + 64 + lane : last;
    ColHead h;
    h.r0 = a.crow[p0];
    h.r1 = a.crow[p1];
    h.x0 = a.cval[p0];
    h.x1 = a.cval[p1];
    return h;
}

// One closed-form step on column [c0, c1) by ONE wave (S/fm/lib/ALS.scala:36-43 linear, :52-68 factor):
// h_r, the sums sum h^2 / sum e*h, theta*, then e += h*(theta* - theta) (and q += x*(theta* - theta)).
// The first two wave-iterations of the column (<= 128 entries: every column of config 1) stay in registers
// between the sums and the update — e and q are read from LDS once; `head` arrives prefetched and leaves holding
// the next column's.
template <bool FACTOR, bool NEXT, class DRAW>
__device__ __forceinline__ double column_step(const AlsArgs &a, double *e, double *q, int c0, int c1, double theta, const DRAW &draw,
                                              double zn, ColHead &head, int lane) {
#pragma clang fp contract(off)
    const int n = c1 - c0;
    const ColHead next = NEXT ? load_head(a, c1, lane) : head;      // in flight while this column is reduced
    const bool v0 = lane < n, v1 = 64 + lane < n;
    const uint32_t ra = v0 ? head.r0 & 0x7fffffffu : 0u, rb = v1 ? head.r1 & 0x7fffffffu : 0u;
    const double xa = head.x0, xb = head.x1;
    const double ea = e[ra], eb = e[rb];
    const double qa = FACTOR ? q[ra] : 0.0, qb = FACTOR ? q[rb] : 0.0;
    double ha = FACTOR ? xa * qa - xa * xa * theta : xa;            // :56-58 / :40
    double hb = FACTOR ? xb * qb - xb * xb * theta : xb;
    ha = v0 ? ha : 0.0;
    hb = v1 ? hb : 0.0;
    double shs = 0.0, seh = 0.0;
    shs += ha * ha;
    seh += (v0 ? ea : 0.0) * ha;
    shs += hb * hb;
    seh += (v1 ? eb : 0.0) * hb;
    for (int p = c0 + 128 + lane; p < c1; p += 64) {               // long columns: re-read in the update pass
        const uint32_t r = a.crow[p] & 0x7fffffffu;
        const double x = a.cval[p];
        const double h = FACTOR ? x * q[r] - x * x * theta : x;
        shs += h * h;
        seh += e[r] * h;
    }
    shs = wave_sum(shs);
    seh = wave_sum(seh);
    const double tn = draw(theta, seh, shs, zn);
    const double d = tn - theta;
    const bool upd = is_updatable(tn, theta);
    if (v0) {
        if (upd) e[ra] = ea + ha * d;                              // updateError :194-198
        if (FACTOR) q[ra] = qa + xa * d;                           // :60-62
    }
    if (v1) {
        if (upd) e[rb] = eb + hb * d;
        if (FACTOR) q[rb] = qb + xb * d;
    }
    for (int p = c0 + 128 + lane; p < c1; p += 64) {
        const uint32_t r = a.crow[p] & 0x7fffffffu;
        const double x = a.cval[p];
        if (upd) {
            const double h = FACTOR ? x * q[r] - x * x * theta : x;
            e[r] += h * d;
        }
        if (FACTOR) q[r] += x * d;
    }
    head = next;
    return tn;
}

// The column walk of one pass (linear weights, or factor f) by wave 0.  Everything a step needs from global memory
// is requested a step (the column's entries, theta) or two (its feature id and end offset) ahead, so the chain of a
// step is LDS + vector ALU only.  Valid because a pass touches every parameter exactly once.
// (The MCMC walk's noise rides beside theta: drawn before the epoch's first dependent launch, read a step ahead.)
template <bool FACTOR, class... M>
__device__ __forceinline__ void walk_columns(const AlsArgs &a, double *e, double *q, int f, int lane, const M &...m) {
    const int k = a.k, nc = a.n_cols;
    if (nc < 1 || a.nnz < 1) return;
    double *par = FACTOR ? a.v + f : a.w;                          // parameter of feature i: par[i * stride]
    const int64_t stride = FACTOR ? k : 1;
    const int g = FACTOR ? 1 + f : 0;
    const auto draw = group_draw(a, g, FACTOR ? a.regv : a.regw, m...);
    const int64_t zrow = (int64_t)g * nc;
    int c0 = a.cptr[0], c1 = a.cptr[1];
    int64_t i_cur = a.cfeat[0], i_nx = a.cfeat[nc > 1 ? 1 : 0];
    int c_nx1 = a.cptr[nc > 1 ? 2 : 1];
    double th_cur = par[i_cur * stride];
    double z_cur = noise_at(zrow, m...);
    auto step_cur = draw.at(i_cur);                                // (with attribute groups: the column's own lambda and mu, looked up a step ahead)
    ColHead head = load_head(a, c0, lane);
    for (int s = 0; s < nc; ++s) {
        const double th_nx = par[i_nx * stride];                   // step s+1's parameter
        const double z_nx = noise_at(zrow + (s + 1 < nc ? s + 1 : nc - 1), m...);        // ... and its noise
        const auto step_nx = draw.at(i_nx);
        const int64_t i_nn = a.cfeat[s + 2 < nc ? s + 2 : nc - 1]; // step s+2's feature id and end offset (clamped, unconditional)
        const int c_nn1 = a.cptr[s + 3 < nc ? s + 3 : nc];
        if (i_cur < a.num_attribute) {                             // `0 until num_attribute`: slot n is never trained (quirk Q1)
            const double tn = column_step<FACTOR, true>(a, e, q, c0, c1, th_cur, step_cur, z_cur, head, lane);
            if (lane == 0) par[i_cur * stride] = tn;               // :40 / :64
        } else {
            head = load_head(a, c1, lane);                         // skipped column: still hand the next column's head on
        }
        c0 = c1; c1 = c_nx1; c_nx1 = c_nn1;
        i_cur = i_nx; i_nx = i_nn;
        th_cur = th_nx;
        z_cur = z_nx;
        step_cur = step_nx;
    }
}

// ---- level sweep ----------------------------------------------------------------------------------------
// The columns of ONE level of the schedule side by side, a wave each: they share no row, so each step reads and writes
// residuals / q entries no other step of the launch touches, and all the columns it depends on (smaller ids sharing a
// row) sit in earlier levels = earlier launches.  The step itself is column_step — the operations and the summation order
// of the one-wave LDS walk, on global memory — so a level-scheduled pass leaves the bits the sequential walk leaves.
// One-hot fields (the reference's own MovieLens demo, S/driver.scala:73-113: a user field and an item field) are the
// case this is for: all columns of a field form one level.
template <bool FACTOR, class... M>
__global__ __launch_bounds__(kLevelBlock) void k_als_level(AlsArgs a, double *q, const int32_t *cols, int n, int f, int long_col, M... m) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int j = (int)blockIdx.x * (kLevelBlock / 64) + (int)(threadIdx.x >> 6);
    if (j >= n) return;
    const int s = cols[j];
    const int64_t i = a.cfeat[s];
    if (i >= a.num_attribute) return;                              // `0 until num_attribute` (quirk Q1)
    const int c0 = a.cptr[s], c1 = a.cptr[s + 1];
    if (c1 - c0 >= long_col) return;                               // a long column of the level: the chip-wide step behind this launch
    double *par = FACTOR ? a.v + f + i * a.k : a.w + i;
    ColHead head = load_head(a, c0, lane);
    const int g = FACTOR ? 1 + f : 0;
    const double tn = column_step<FACTOR, false>(a, a.e, q, c0, c1, *par, group_draw(a, g, FACTOR ? a.regv : a.regw, m...).at(i),
                                                 noise_at((int64_t)g * a.n_cols + s, m...), head, lane);
    if (lane == 0) *par = tn;                                      // :40 / :64
}

template <class... M>
__global__ __launch_bounds__(kLdsSweepThreads) void k_als_sweep_lds(AlsArgs a, const double *qall, M... m) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double lds_eq[];
    double *e = lds_eq, *q = lds_eq + a.n_rows;
    const int tid = threadIdx.x, lane = tid & 63;
    const bool walker = tid < 64;                                  // wave 0 walks the columns
    for (int64_t r = tid; r < a.n_rows; r += kLdsSweepThreads) e[r] = a.e[r];
    __syncthreads();
    // (the global bias step ran before this launch: k_als_w0, then the residuals again with the new bias)
    // ---- linear weights (:36-43)
    if (walker) walk_columns<false>(a, e, q, 0, lane, m...);
    // ---- factors (:50-68): q of the factor comes in from the up-front pass, every thread copies its share
    for (int f = 0; f < a.k; ++f) {
        __syncthreads();
        for (int64_t r = tid; r < a.n_rows; r += kLdsSweepThreads) q[r] = qall[(int64_t)f * a.n_rows + r];
        __syncthreads();
        if (walker) walk_columns<true>(a, e, q, f, lane, m...);
    }
}

// ---- the launch plan ----------------------------------------------------------------------------------------

// one chip-wide closed-form step of a long column (two launches; see k_als_col_sums)
template <class Dev>
inline Dev own_noise(Dev m, int64_t zi) {
    m.zi = zi;
    return m;
}

// (slot: the column's index among the compressed columns — where its noise lies)
template <bool FACTOR, class... M>
void long_column_step(const AlsArgs &a, double *q, int c0, int c1, int64_t i, int f, int slot, hipStream_t s, const M &...m) {
    int G = (c1 - c0 + 2047) / 2048;
    if (G > kAlsMaxParts) G = kAlsMaxParts;
    const int64_t zi = (int64_t)(FACTOR ? 1 + f : 0) * a.n_cols + slot;
    hipLaunchKernelGGL((k_als_col_sums<FACTOR>), dim3((unsigned)G), dim3(kColBlock), 0, s, a, q, c0, c1, i, f);
    hipLaunchKernelGGL((k_als_col_update<FACTOR, M...>), dim3((unsigned)G), dim3(kColBlock), 0, s, a, q, c0, c1, i, f, own_noise(m, zi)...);
}

// How a dataset's columns are walked, decided once per launch_* call from the host's view of them and the two environment knobs:
// columns of at least long_col entries take the chip-wide step (FMHIP_ALS_LONG overrides kAlsLongColumn); `levels`: the level
// schedule — a launch per level and pass, every column of the level on a wave of its own — pays when the levels are wide (one-hot
// fields: two levels of thousands of columns), while a dense conflict graph (config 1: every column shares rows with most others)
// has about as many levels as columns and keeps the sequential walks (FMHIP_ALS_LEVELS=0 / 1: never / always);
// wide_wg: the sequential walk's workgroup has 1024 threads, not 256 (a barrier over 4 waves is ~3x cheaper than over 16), when
// the columns it walks average at least 512 entries.  The two walks take that mean differently and both rules are kept as they
// were measured: the flat walk over its SHORT columns only (the long ones leave it for the chip-wide step), the block walk over
// all of the block's columns (it walks every one of them itself).
struct WalkChoice {
    int long_col;
    bool levels, wide_wg;
};

WalkChoice walk_choice(const AlsArgs &a, const ColumnPlan &plan, bool block_walk) {
    WalkChoice c{kAlsLongColumn, false, false};
    if (const char *ev = getenv("FMHIP_ALS_LONG")) c.long_col = atoi(ev) > 0 ? atoi(ev) : c.long_col;
    const bool have = plan.h_lev_ptr && plan.h_lev_cols && a.lev_cols && plan.n_levels > 0;
    c.levels = have && (int64_t)plan.n_levels * 16 <= a.n_cols;
    if (const char *ev = getenv("FMHIP_ALS_LEVELS")) c.levels = have && atoi(ev) != 0;
    if (c.levels || a.n_cols < 1) return c;
    if (block_walk) {
        c.wide_wg = (int64_t)plan.h_cptr[a.n_cols] / a.n_cols >= 512;
    } else {
        int64_t short_nnz = 0, n_short = 0;
        for (int col = 0; col < a.n_cols; ++col) {
            const int len = plan.h_cptr[col + 1] - plan.h_cptr[col];
            if (len < c.long_col) { short_nnz += len; ++n_short; }
        }
        c.wide_wg = n_short > 0 && short_nnz / n_short >= 512;
    }
    return c;
}

// e and q in global memory, following the column lengths: a run of short columns is one launch of one workgroup, a long column two
// chip-wide launches
template <bool FACTOR, class... M>
hipError_t sweep_pass(const AlsArgs &a, const ColumnPlan &plan, const WalkChoice &c, int f, hipStream_t s, const M &...m) {
    const int32_t *h_cfeat = plan.h_cfeat, *h_cptr = plan.h_cptr;
    double *q = a.q + (FACTOR ? (int64_t)f * a.n_rows : 0);
    int s0 = 0;
    while (s0 < a.n_cols) {
        const int len = h_cptr[s0 + 1] - h_cptr[s0];
        if (len >= c.long_col) {
            if (h_cfeat[s0] < a.num_attribute) long_column_step<FACTOR>(a, q, h_cptr[s0], h_cptr[s0 + 1], (int64_t)h_cfeat[s0], f, s0, s, m...);
            ++s0;
            continue;
        }
        int s1 = s0 + 1;
        while (s1 < a.n_cols && h_cptr[s1 + 1] - h_cptr[s1] < c.long_col) ++s1;
        if (c.wide_wg) hipLaunchKernelGGL((k_als_cols_wg<1024, FACTOR, M...>), dim3(1), dim3(1024), 0, s, a, q, s0, s1, f, m...);
        else hipLaunchKernelGGL((k_als_cols_wg<256, FACTOR, M...>), dim3(1), dim3(256), 0, s, a, q, s0, s1, f, m...);
        s0 = s1;
    }
    return hipGetLastError();
}

template <bool FACTOR, class... M>
hipError_t level_pass(const AlsArgs &a, const ColumnPlan &plan, const WalkChoice &c, int f, hipStream_t s, const M &...m) {
    const int32_t *h_cfeat = plan.h_cfeat, *h_cptr = plan.h_cptr, *h_lev_ptr = plan.h_lev_ptr;
    double *q = a.q + (FACTOR ? (int64_t)f * a.n_rows : 0);
    for (int l = 0; l < plan.n_levels; ++l) {
        const int n = h_lev_ptr[l + 1] - h_lev_ptr[l];
        if (n < 1) continue;
        hipLaunchKernelGGL((k_als_level<FACTOR, M...>), dim3((unsigned)((n + kLevelBlock / 64 - 1) / (kLevelBlock / 64))), dim3(kLevelBlock), 0, s, a, q,
                           a.lev_cols + h_lev_ptr[l], n, f, c.long_col, m...);
        // the level's long columns share no row with its other columns either: their chip-wide steps follow, in any order
        for (int j = h_lev_ptr[l]; j < h_lev_ptr[l + 1]; ++j) {
            const int col = plan.h_lev_cols[j];
            if (h_cptr[col + 1] - h_cptr[col] >= c.long_col && h_cfeat[col] < a.num_attribute)
                long_column_step<FACTOR>(a, q, h_cptr[col], h_cptr[col + 1], (int64_t)h_cfeat[col], f, col, s, m...);
        }
    }
    return hipGetLastError();
}

// The pass of ONE parameter group (0: w; 1 + f: factor f) over e and q in global memory: the level walk or the sweep walk
template <class... M>
hipError_t group_pass(const AlsArgs &a, int g, const ColumnPlan &plan, const WalkChoice &c, hipStream_t s, const M &...m) {
    if (c.levels) return g == 0 ? level_pass<false>(a, plan, c, 0, s, m...) : level_pass<true>(a, plan, c, g - 1, s, m...);
    return g == 0 ? sweep_pass<false>(a, plan, c, 0, s, m...) : sweep_pass<true>(a, plan, c, g - 1, s, m...);
}

unsigned row_blocks(int64_t n_rows) {
    int64_t blocks = (n_rows + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    return (unsigned)(blocks < 1 ? 1 : blocks);
}

// Everything of an epoch behind its first residual pass (which the caller has launched): the bias step, the residuals
// again, every factor's q, the sweeps.  With an McmcDev every closed-form step is the Gaussian conditional's draw.
template <class... M>
hipError_t epoch_tail(const AlsArgs &a, const ColumnPlan &plan, hipStream_t s, const M &...m) {
    const unsigned blocks = row_blocks(a.n_rows);
    // precomputeTermE (:17) with the old bias feeds the bias step (:19-27); the residuals the sweeps start from are
    // evaluated after `fm.w0 = w0` (see k_als_w0)
    hipLaunchKernelGGL((k_als_w0<1024, M...>), dim3(1), dim3(1024), 0, s, a, m...);
    hipLaunchKernelGGL(k_als_residual, dim3(blocks), dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    int64_t qb = (a.n_rows * a.k + 255) / 256;
    if (qb > 4096) qb = 4096;
    hipLaunchKernelGGL(k_als_q_all, dim3((unsigned)(qb < 1 ? 1 : qb)), dim3(256), 0, s, a, a.q);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const WalkChoice c = walk_choice(a, plan, false);
    if (!c.levels && (size_t)a.n_rows * 2 * sizeof(double) <= kAlsLdsBytes && !getenv("FMHIP_ALS_NO_LDS")) {
        // e and q fit the LDS of one CU: the one-wave column walk
        e = hipFuncSetAttribute((const void *)k_als_sweep_lds<M...>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kAlsLdsBytes);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_als_sweep_lds<M...>, dim3(1), dim3(kLdsSweepThreads), (size_t)a.n_rows * 2 * sizeof(double), s, a, a.q, m...);
        return hipGetLastError();
    }
    for (int g = 0; g <= a.k; ++g)
        if ((e = group_pass(a, g, plan, c, s, m...)) != hipSuccess) return e;
    return hipSuccess;
}

}  // namespace

hipError_t launch_als_epoch(const AlsArgs &a, const ColumnPlan &plan, hipStream_t s) {
    hipLaunchKernelGGL(k_als_residual, dim3(row_blocks(a.n_rows)), dim3(256), 0, s, a);
    return epoch_tail(a, plan, s);
}

hipError_t launch_mcmc_noise(const AlsArgs &a, double *z, uint64_t seed, uint32_t t, hipStream_t s) {
    int64_t nb = ((int64_t)(a.k + 1) * a.n_cols + 1 + 255) / 256;
    if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL(k_mcmc_noise, dim3((unsigned)nb), dim3(256), 0, s, a, z, seed, t);
    return hipGetLastError();
}

hipError_t launch_mcmc_begin(const AlsArgs &a, const McmcDev &m, double *z, uint64_t seed, uint32_t t, double *sums, hipStream_t s,
                             const McmcProbit *probit, const McmcGroupSums *groups) {
    if (m.sample) {
        const hipError_t e = launch_mcmc_noise(a, z, seed, t, s);
        if (e != hipSuccess) return e;
    }
    if (probit)
        hipLaunchKernelGGL(k_mcmc_probit_targets, dim3(row_blocks(a.n_rows)), dim3(256), 0, s, a, *probit, seed, t);
    else
        hipLaunchKernelGGL(k_als_residual, dim3(row_blocks(a.n_rows)), dim3(256), 0, s, a);
    // with groups quantity 0 (sum e^2) stays where it is: k_mcmc_sums' first kMcmcSumParts workgroups, which read nothing of the state
    hipLaunchKernelGGL(k_mcmc_sums, dim3((unsigned)((groups ? 1 : a.k + 2) * kMcmcSumParts)), dim3(kSumsBlock), 0, s, a, m, sums, kMcmcSumParts);
    if (groups && m.sample && groups->n_chunks > 0)
        hipLaunchKernelGGL(k_mcmc_group_sums, dim3((unsigned)groups->n_chunks), dim3(kGroupSumsBlock), 0, s, a, static_cast<const McmcGroupDev &>(m), *groups);
    return hipGetLastError();
}

hipError_t launch_mcmc_sweeps(const AlsArgs &a, const McmcDev &m, const ColumnPlan &plan, hipStream_t s) { return epoch_tail(a, plan, s, m); }
hipError_t launch_mcmc_sweeps(const AlsArgs &a, const McmcGroupDev &m, const ColumnPlan &plan, hipStream_t s) { return epoch_tail(a, plan, s, m); }

hipError_t launch_mcmc_accumulate_link(double *last, double *sum, int64_t n_rows, const McmcLink &link, hipStream_t s) {
    if (n_rows < 1) return hipSuccess;
    const dim3 grid(row_blocks(n_rows)), block(256);
    if (link.kind == kLinkProbit)
        hipLaunchKernelGGL(k_mcmc_accumulate_link<LinkProbit>, grid, block, 0, s, last, sum, n_rows, LinkProbit{});
    else if (link.kind == kLinkClamp)
        hipLaunchKernelGGL(k_mcmc_accumulate_link<LinkClamp>, grid, block, 0, s, last, sum, n_rows, LinkClamp{link.lo, link.hi});
    else
        hipLaunchKernelGGL(k_mcmc_accumulate, grid, block, 0, s, last, sum, n_rows);
    return hipGetLastError();
}

hipError_t launch_mcmc_accumulate(const AlsArgs &t, double *sum, hipStream_t s, const McmcLink &link) {
    if (t.n_rows < 1) return hipSuccess;
    hipLaunchKernelGGL(k_als_residual, dim3(row_blocks(t.n_rows)), dim3(256), 0, s, t);
    return launch_mcmc_accumulate_link(t.e, sum, t.n_rows, link, s);
}

// ==== the block-structure sweep (include/fmhip_mcmc_relational.h; launchers: mcmc_blocks.h) =====================================
// The same conditional on the same columns, with a block column's sums taken over the BLOCK's rows from per-row caches instead of
// over the data rows that reference them.  Per part and parameter group: k_block_gather (+ _long) builds the caches by a segmented
// sum over the handle's inverse map, k_block_level / k_block_cols_wg walk the block's columns, k_block_scatter takes the steps back
// to e and Q_f.  Every operation's order is written down in the public header; no fused multiply-add anywhere.
namespace {

// yhat_r, e_r and Q_f[r] of every data row from the blocks' yhat_p and q_p; PROBIT: k_mcmc_probit_targets' draw around yhat_r
template <bool PROBIT>
__global__ __launch_bounds__(256) void k_block_combine(BlockCombine c, McmcProbit p, uint64_t seed, uint32_t t) {
#pragma clang fp contract(off)
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < c.n_rows; r += (int64_t)gridDim.x * 256) {
        const double w0 = *c.w0;
        int64_t j[kBlockPartsMax];
        double yhat = w0;
        for (int b = 0; b < c.n_parts; ++b) {
            j[b] = c.map[b] ? (int64_t)c.map[b][r] : r;
            yhat += c.yhat[b][j[b]] - w0;
        }
        for (int f = 0; f < c.k; ++f) {
            double run = c.q[0][f * c.J[0] + j[0]], cross = 0.0;
            for (int b = 1; b < c.n_parts; ++b) {
                const double qb = c.q[b][f * c.J[b] + j[b]];
                cross += run * qb;
                run += qb;
            }
            yhat += cross;
            if (c.Q) c.Q[f * c.n_rows + r] = run;
        }
        c.e[r] = PROBIT ? probit_residual(p, r, yhat, seed, t) : yhat - c.y[r];
    }
}

// k_mcmc_sums' quantity 1 + g over ONE part's trained columns
__global__ __launch_bounds__(kSumsBlock) void k_block_theta_sums(AlsArgs a, const int32_t *trained, const double *hyp, double *out, int P) {
#pragma clang fp contract(off)
    __shared__ double sh[2][kSumsBlock / 64];
    const int g = (int)blockIdx.x / P, chunk = (int)blockIdx.x % P, tid = threadIdx.x;
    double s0 = 0.0, s1 = 0.0;
    theta_sums(a, g, hyp[2 + a.k + g], chunk, P, tid, [&](int64_t s) { return trained[s] != 0; }, s0, s1);
    block_sum2<kSumsBlock>(s0, s1, sh);
    if (tid == 0) {
        out[2 * (int64_t)blockIdx.x] = s0;
        out[2 * (int64_t)blockIdx.x + 1] = s1;
    }
}

// The cache build: work item w = one list of the inverse map (or one chunk of kRelSumCut rows of a longer list), a thread each, the
// rows ascending.  One writer per address: a block row's caches (or a partial row), and qrest[r] of the rows it reads.
template <bool FACTOR>
__global__ __launch_bounds__(256) void k_block_gather(BlockPart b, const double *e, const double *Qf, const double *qp) {
#pragma clang fp contract(off)
    const int w = (int)blockIdx.x * 256 + threadIdx.x;
    if (w >= b.n_work) return;
    const int t = b.wt[w], beg = b.wbeg[w];
    const int end = beg + kRelSumCut < b.tptr[t + 1] ? beg + kRelSumCut : b.tptr[t + 1];
    double E = 0.0, A = 0.0, B = 0.0, Cc = 0.0;
    const double qj = FACTOR ? qp[b.tj[t]] : 0.0;
    for (int pos = beg; pos < end; ++pos) {
        const int r = b.trow[pos];
        const double er = e[r];
        E += er;
        if (FACTOR) {
            const double qr = Qf[r] - qj;
            b.qrest[r] = qr;
            A += qr;
            B += qr * qr;
            Cc += er * qr;
        }
    }
    const int dst = b.wdst[w];
    if (dst >= 0) {
        b.cache[dst] = E;
        if (FACTOR) {
            b.cache[b.J + dst] = A;
            b.cache[2 * b.J + dst] = B;
            b.cache[3 * b.J + dst] = Cc;
        }
    } else {
        double *part = b.part + 4 * (int64_t)(-1 - dst);
        part[0] = E;
        part[1] = A;
        part[2] = B;
        part[3] = Cc;
    }
}

// ... and the long lists: their chunks' sums added in chunk order
__global__ __launch_bounds__(256) void k_block_gather_long(BlockPart b) {
#pragma clang fp contract(off)
    const int l = (int)blockIdx.x * 256 + threadIdx.x;
    if (l >= b.n_long) return;
    const int64_t j = b.tj[b.lt[l]];
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int c = 0; c < b.lcount[l]; ++c) {
        const double *part = b.part + 4 * (int64_t)(b.lfirst[l] + c);
        for (int x = 0; x < 4; ++x) s[x] += part[x];
    }
    for (int x = 0; x < 4; ++x) b.cache[x * b.J + j] = s[x];
}

// sum h^2 and sum e*h of block column [c0, c1) from the caches: this thread's share (entries tid, tid + stride, ...)
template <bool FACTOR>
__device__ __forceinline__ void block_col_sums(const BlockPart &b, const double *qp, int c0, int c1, double th, int tid, int stride, double &shs,
                                               double &seh) {
#pragma clang fp contract(off)
    const double *E = b.cache, *A = b.cache + b.J, *B = b.cache + 2 * b.J, *Cc = b.cache + 3 * b.J;
    for (int p = c0 + tid; p < c1; p += stride) {
        const uint32_t j = b.a.crow[p] & 0x7fffffffu;
        const double x = b.a.cval[p];
        if (FACTOR) {
            const double u = qp[j] - x * th;
            shs += (x * x) * ((b.n[j] * (u * u) + (2.0 * u) * A[j]) + B[j]);
            seh += x * (u * E[j] + Cc[j]);
        } else {
            shs += (x * x) * b.n[j];
            seh += x * E[j];
        }
    }
}

// the step d = theta' - theta of block column [c0, c1) into the caches (a column's block rows are distinct: one writer each)
template <bool FACTOR>
__device__ __forceinline__ void block_col_update(const BlockPart &b, double *qp, int c0, int c1, double th, double d, int tid, int stride) {
#pragma clang fp contract(off)
    double *E = b.cache, *A = b.cache + b.J, *B = b.cache + 2 * b.J, *Cc = b.cache + 3 * b.J, *S1 = b.cache + 4 * b.J, *S2 = b.cache + 5 * b.J;
    for (int p = c0 + tid; p < c1; p += stride) {
        const uint32_t j = b.a.crow[p] & 0x7fffffffu;
        const double xd = b.a.cval[p] * d;
        if (FACTOR) {
            const double u = qp[j] - b.a.cval[p] * th;
            E[j] += xd * (b.n[j] * u + A[j]);
            Cc[j] += xd * (u * A[j] + B[j]);
            S1[j] += xd * u;
            S2[j] += xd;
            qp[j] += xd;
        } else {
            E[j] += b.n[j] * xd;
            S2[j] += xd;                                          // (the w pass's D)
        }
    }
}

// The columns of one LEVEL of the block's schedule, a wave each (k_als_level's shape: they share no block row)
template <bool FACTOR>
__global__ __launch_bounds__(kLevelBlock) void k_block_level(BlockPart b, const int32_t *cols, int n, int f, int long_col, McmcDev m) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int jc = (int)blockIdx.x * (kLevelBlock / 64) + (int)(threadIdx.x >> 6);
    if (jc >= n) return;
    const int s = cols[jc];
    if (!b.trained[s]) return;
    const int c0 = b.a.cptr[s], c1 = b.a.cptr[s + 1];
    if (c1 - c0 >= long_col) return;                               // the 1024-thread workgroup walk behind this launch
    const int64_t i = b.a.cfeat[s];
    double *par = FACTOR ? b.a.v + f + i * b.a.k : b.a.w + i;
    double *qp = b.a.q + (FACTOR ? (int64_t)f * b.J : 0);
    const int g = FACTOR ? 1 + f : 0;
    const double th = *par;
    double shs = 0.0, seh = 0.0;
    block_col_sums<FACTOR>(b, qp, c0, c1, th, lane, 64, shs, seh);
    shs = wave_sum(shs);
    seh = wave_sum(seh);
    const double tn = group_draw(b.a, g, 0.0, m).at(i)(th, seh, shs, noise_at((int64_t)g * b.a.n_cols + s, m));
    if (is_updatable(tn, th)) block_col_update<FACTOR>(b, qp, c0, c1, th, tn - th, lane, 64);
    if (lane == 0) *par = tn;
}

// The columns [s_lo, s_hi) in order by ONE workgroup (k_als_cols_wg's shape): a dense conflict graph, or one long column
template <int kAlsBlock, bool FACTOR>
__global__ __launch_bounds__(kAlsBlock) void k_block_cols_wg(BlockPart b, int s_lo, int s_hi, int f, McmcDev m) {
#pragma clang fp contract(off)
    __shared__ double sh[2][kAlsBlock / 64];
    const int tid = threadIdx.x;
    const int g = FACTOR ? 1 + f : 0;
    double *qp = b.a.q + (FACTOR ? (int64_t)f * b.J : 0);
    const auto draw = group_draw(b.a, g, 0.0, m);
    for (int s = s_lo; s < s_hi; ++s) {
        if (!b.trained[s]) continue;
        const int64_t i = b.a.cfeat[s];
        const int c0 = b.a.cptr[s], c1 = b.a.cptr[s + 1];
        double *par = FACTOR ? b.a.v + f + i * b.a.k : b.a.w + i;
        const double th = *par;
        const double zn = noise_at((int64_t)g * b.a.n_cols + s, m);
        double shs = 0.0, seh = 0.0;
        block_col_sums<FACTOR>(b, qp, c0, c1, th, tid, kAlsBlock, shs, seh);
        block_sum2<kAlsBlock>(shs, seh, sh);
        const double tn = draw.at(i)(th, seh, shs, zn);
        if (is_updatable(tn, th)) block_col_update<FACTOR>(b, qp, c0, c1, th, tn - th, tid, kAlsBlock);
        __syncthreads();
        if (tid == 0) *par = tn;
        __syncthreads();
    }
}

// the part's steps back to the data rows
template <bool FACTOR>
__global__ __launch_bounds__(256) void k_block_scatter(BlockPart b, double *e, double *Qf) {
#pragma clang fp contract(off)
    const double *S1 = b.cache + 4 * b.J, *S2 = b.cache + 5 * b.J;
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < b.n_rows; r += (int64_t)gridDim.x * 256) {
        const int64_t j = b.map[r];
        if (FACTOR) {
            e[r] += S1[j] + S2[j] * b.qrest[r];
            Qf[r] += S2[j];
        } else {
            e[r] += S2[j];
        }
    }
}

template <bool FACTOR>
hipError_t block_pass(const BlockPart &b, const BlockPlan &plan, const WalkChoice &c, int f, double *e, double *Q, const McmcDev &m, hipStream_t s) {
    const int n_cols = b.a.n_cols;
    double *Qf = FACTOR ? Q + (int64_t)f * b.n_rows : nullptr;
    const double *qp = FACTOR ? b.a.q + (int64_t)f * b.J : nullptr;
    hipError_t err = hipMemsetAsync(b.cache, 0, (size_t)kBlockCaches * (size_t)b.J * sizeof(double), s);      // rows nobody references: exact zeros
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL((k_block_gather<FACTOR>), dim3((unsigned)((b.n_work + 255) / 256)), dim3(256), 0, s, b, e, Qf, qp);
    if (b.n_long > 0) hipLaunchKernelGGL(k_block_gather_long, dim3((unsigned)((b.n_long + 255) / 256)), dim3(256), 0, s, b);
    if (c.levels) {
        for (int l = 0; l < plan.n_levels; ++l) {
            const int n = plan.h_lev_ptr[l + 1] - plan.h_lev_ptr[l];
            if (n < 1) continue;
            hipLaunchKernelGGL((k_block_level<FACTOR>), dim3((unsigned)((n + kLevelBlock / 64 - 1) / (kLevelBlock / 64))), dim3(kLevelBlock), 0, s, b,
                               b.a.lev_cols + plan.h_lev_ptr[l], n, f, c.long_col, m);
            for (int j = plan.h_lev_ptr[l]; j < plan.h_lev_ptr[l + 1]; ++j) {      // the level's long columns share no row with its others
                const int col = plan.h_lev_cols[j];
                if (plan.h_cptr[col + 1] - plan.h_cptr[col] >= c.long_col && plan.h_trained[col])
                    hipLaunchKernelGGL((k_block_cols_wg<1024, FACTOR>), dim3(1), dim3(1024), 0, s, b, col, col + 1, f, m);
            }
        }
    } else if (n_cols > 0) {
        if (c.wide_wg) hipLaunchKernelGGL((k_block_cols_wg<1024, FACTOR>), dim3(1), dim3(1024), 0, s, b, 0, n_cols, f, m);
        else hipLaunchKernelGGL((k_block_cols_wg<256, FACTOR>), dim3(1), dim3(256), 0, s, b, 0, n_cols, f, m);
    }
    hipLaunchKernelGGL((k_block_scatter<FACTOR>), dim3(row_blocks(b.n_rows)), dim3(256), 0, s, b, e, Qf);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_block_forward(const AlsArgs &a, bool with_q, hipStream_t s) {
    if (a.n_rows < 1) return hipSuccess;
    hipLaunchKernelGGL(k_als_residual, dim3(row_blocks(a.n_rows)), dim3(256), 0, s, a);
    int64_t qb = (a.n_rows * a.k + 255) / 256;
    if (qb > 4096) qb = 4096;
    if (with_q && a.k > 0) hipLaunchKernelGGL(k_als_q_all, dim3((unsigned)(qb < 1 ? 1 : qb)), dim3(256), 0, s, a, a.q);
    return hipGetLastError();
}

hipError_t launch_block_combine(const BlockCombine &c, const McmcProbit *probit, uint64_t seed, uint32_t t, hipStream_t s) {
    if (c.n_rows < 1) return hipSuccess;
    if (probit) hipLaunchKernelGGL(k_block_combine<true>, dim3(row_blocks(c.n_rows)), dim3(256), 0, s, c, *probit, seed, t);
    else hipLaunchKernelGGL(k_block_combine<false>, dim3(row_blocks(c.n_rows)), dim3(256), 0, s, c, McmcProbit{}, seed, t);
    return hipGetLastError();
}

hipError_t launch_block_sse(const AlsArgs &rows, double *sums, hipStream_t s) {      // k_mcmc_sums' quantity 0: it reads nothing of McmcDev
    hipLaunchKernelGGL(k_mcmc_sums, dim3((unsigned)kMcmcSumParts), dim3(kSumsBlock), 0, s, rows, McmcDev{}, sums, kMcmcSumParts);
    return hipGetLastError();
}

hipError_t launch_block_theta_sums(const AlsArgs &a, const int32_t *trained, const double *hyp, double *out, hipStream_t s) {
    hipLaunchKernelGGL(k_block_theta_sums, dim3((unsigned)((a.k + 1) * kMcmcSumParts)), dim3(kSumsBlock), 0, s, a, trained, hyp, out, kMcmcSumParts);
    return hipGetLastError();
}

hipError_t launch_block_bias(const AlsArgs &rows, const McmcDev &m, hipStream_t s) {
    hipLaunchKernelGGL((k_als_w0<1024, McmcDev>), dim3(1), dim3(1024), 0, s, rows, m);
    return hipGetLastError();
}

hipError_t launch_block_pass(const BlockPart &b, const BlockPlan &plan, int g, double *e, double *Q, const McmcDev &m, hipStream_t s) {
    const WalkChoice c = walk_choice(b.a, plan, true);
    return g == 0 ? block_pass<false>(b, plan, c, 0, e, Q, m, s) : block_pass<true>(b, plan, c, g - 1, e, Q, m, s);
}

hipError_t launch_plain_pass(const AlsArgs &a, int g, const McmcDev &m, const ColumnPlan &plan, hipStream_t s) {
    if (a.n_cols < 1) return hipSuccess;
    return group_pass(a, g, plan, walk_choice(a, plan, false), s, m);
}

}  // namespace fmhip
