// fm_autoint.hip — the kernels of AutoInt (include/fmhip_autoint.h; DESIGN.md, "AutoInt"): gfx950, wave64.
//   k_autoint_forward  a workgroup of four waves owns kAutoIntRowsPerBlock rows and takes them ONE ROW AT A TIME: the row's Fp = F
//                      rounded up to 16 tokens are the M dimension of every product on the exact-f32 MFMA.  Per layer: the projection
//                      X_l WT_l^T into the LDS tile Y = [Q | K | V | R]; per head Q^h K^h^T in accumulators, the row softmax in
//                      registers (a wave per M tile, every N tile of it), the probabilities of that ONE head into the tile P, then
//                      P^h V^h, whose epilogue adds R, applies the ReLU and writes X_{l+1}.  A training launch goes on backwards over
//                      the same tiles: Gz into R's place, P^h recomputed from the kept Q^h, K^h, dSc^h beside it, the three products
//                      dV^h, dQ^h, dK^h held in accumulators across a barrier and written over V^h, Q^h, K^h, the dense gradient
//                      e_r X_l^T Y added into MFMA accumulators that live for the workgroup's 128 rows, d yhat / d X_l = Y WT_l into
//                      the tile of X_{l+1}; J ends in X_0's tile and a lane group per entry writes x_a J[f_a].  Also the scorer
//   k_autoint_dupdate  a thread per dense parameter: the workgroups' partials in block order, then the step
// v, w, w0 and the statistics: fm_fwfm.hip's backward and update launches over this forward's dz, e and bsum.
// No atomics: one writer per element, every sum in an order fixed by the data and by the constants of fm_autoint.h.
// exp: OCML's expf, at most 1 ulp from the exact value (it is given s - max <= 0, so it never overflows).
#include "fm_device.h"
#include "fm_finish.h"      // pair_sigma_residual
#include "fm_autoint.h"

namespace fmhip {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// MFMA lane roles (v_mfma_f32_16x16x4_f32): lane (g, c) = (lane / 16, lane % 16) supplies A[c][g] and B[g][c] of a step and holds
// D[4g + i][c] in acc[i].  The four waves take the (M tile, N tile) jobs of a product in the fixed order job = wave, wave + 4, ...

__device__ __forceinline__ f32x4 mfma4(float4 a, float4 b, f32x4 acc) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
}

// OUT[16][16] = Ar Br^T over n16 slices of 16: both operands are rows of LDS tiles, `ar` this lane's row of A and `br` its row of B,
// each at the reduction's first column; step j of slice u takes k = 16u + 4g + j on both sides: one ds_read_b128 each
__device__ __forceinline__ f32x4 rows_product(const float *ar, const float *br, int n16, int g) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma nounroll
    for (int u = 0; u < n16; ++u) acc = mfma4(reinterpret_cast<const float4 *>(ar)[4 * u + g], reinterpret_cast<const float4 *>(br)[4 * u + g], acc);
    return acc;
}

// acc += A B over K = 4 n4 in natural order (step s takes k = 4s + g), both operands LDS tiles read by the element: A[m][k] at
// am[m a_ms + k a_ks] (`am` at the M tile's first row), B[k][n] at bn[k b_ks + n] (`bn` at the N tile's first column); `scale` on A
__device__ __forceinline__ f32x4 lds_product(f32x4 acc, const float *am, int a_ms, int a_ks, const float *bn, int b_ks, int n4, float scale, int g, int c) {
#pragma nounroll
    for (int s = 0; s < n4; ++s)
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(am[c * a_ms + (4 * s + g) * a_ks] * scale, bn[(4 * s + g) * b_ks + c], acc, 0, 0, 0);
    return acc;
}

struct Tiles {
    float *X0, *XL, *Y, *P, *DS, *sm;
    int F, Fp, MT, A, d, LA, LQ, LP;
    bool train;          // scoring keeps X_l, l >= 1, in two tiles by turns
    __device__ float *X(int l) const { return l == 0 ? X0 : XL + (train ? l - 1 : (l - 1) & 1) * Fp * LA; }
    __device__ int ldx(int l) const { return l == 0 ? kAutoIntD0 + kAutoIntPad : LA; }
};

// One head's probabilities: wave mt < MT takes the M tile mt and every N tile of it, so a token's whole score row lies in the 16 lanes
// of its lane group (c) times the wave's MT accumulators.  Row f = 16 mt + 4g + i, column n = 16 nt + c; the columns n >= F are no
// tokens: masked by their index.  Maximum, exp of the max-subtracted score, sum: each over nt ascending in the lane, then the
// butterfly 8, 4, 2, 1 over c.  BWD: also dP = Gz^h V^h^T for the same elements and dSc = P o (dP - rowsum(dP o P)) into DS.
template <bool BWD>
__device__ __forceinline__ void head_softmax(const Tiles &t, int h, int wave, int g, int c) {
    if (wave >= t.MT) return;
    const int mt = wave, n16 = t.d / 16, hc = h * t.d;
    const float *qrow = t.Y + (mt * 16 + c) * t.LQ + hc;
    f32x4 p[4];
    float mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY}, sum[4] = {0.f, 0.f, 0.f, 0.f}, rs[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        if (nt >= t.MT) continue;
        const float *krow = t.Y + (nt * 16 + c) * t.LQ + hc;
        p[nt] = rows_product(qrow, krow + t.A, n16, g);
        if (nt * 16 + c < t.F)
#pragma unroll
            for (int i = 0; i < 4; ++i) mx[i] = fmaxf(mx[i], p[nt][i]);
    }
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1)
#pragma unroll
        for (int i = 0; i < 4; ++i) mx[i] = fmaxf(mx[i], __shfl_xor(mx[i], m, 64));
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        if (nt >= t.MT) continue;
        const bool real = nt * 16 + c < t.F;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float x = real ? expf(p[nt][i] - mx[i]) : 0.f;
            p[nt][i] = x;
            sum[i] += x;
        }
    }
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1)
#pragma unroll
        for (int i = 0; i < 4; ++i) sum[i] += __shfl_xor(sum[i], m, 64);
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        if (nt >= t.MT) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float x = p[nt][i] / sum[i];
            p[nt][i] = x;
            t.P[(mt * 16 + 4 * g + i) * t.LP + nt * 16 + c] = x;
        }
        if (BWD) {                           // dP's tile is formed twice, here and below, instead of being held beside p
            const f32x4 dp = rows_product(qrow + 3 * t.A, t.Y + (nt * 16 + c) * t.LQ + hc + 2 * t.A, n16, g);
#pragma unroll
            for (int i = 0; i < 4; ++i) rs[i] = fmaf(dp[i], p[nt][i], rs[i]);
        }
    }
    if (!BWD) return;
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1)
#pragma unroll
        for (int i = 0; i < 4; ++i) rs[i] += __shfl_xor(rs[i], m, 64);
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        if (nt >= t.MT) continue;
        const f32x4 dp = rows_product(qrow + 3 * t.A, t.Y + (nt * 16 + c) * t.LQ + hc + 2 * t.A, n16, g);
#pragma unroll
        for (int i = 0; i < 4; ++i) t.DS[(mt * 16 + 4 * g + i) * t.LP + nt * 16 + c] = p[nt][i] * (dp[i] - rs[i]);
    }
}

// acc[jj] += e X_l^T Y for the wave's jobs jj of the Dt x NT output tiles (the reduction over the row's tokens); acc lives in
// registers for the workgroup's 128 rows
template <int NJ>
__device__ __forceinline__ void wgrad_add(f32x4 (&acc)[NJ], const float *Xi, int ldi, int Dt, int NT, const Tiles &t, float e, int wave, int g, int c) {
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) {
        const int job = wave + 4 * jj;
        if (job >= Dt * NT) continue;
        const int mt = job / NT, nt = job - mt * NT;
        acc[jj] = lds_product(acc[jj], Xi + mt * 16, 1, ldi, t.Y + nt * 16, t.LQ, t.Fp / 4, e, g, c);
    }
}

// The same at A = 64, where a layer's MTD x 16 output tiles are exactly 4 MTD a wave: no guards, and the tiles as a register block —
// accumulator 4 m + j is the tile (m, wave + 4 j), so a step's MTD reads of X_l and 4 of Y serve 4 MTD MFMAs.  The same k order
template <int MTD>
__device__ __forceinline__ void wgrad_add_wide(f32x4 (&acc)[4 * MTD], const float *Xi, int ldi, const Tiles &t, float e, int wave, int g, int c) {
#pragma nounroll
    for (int s = 0; s < t.Fp / 4; ++s) {
        const float *xr = Xi + (4 * s + g) * ldi + c, *yr = t.Y + (4 * s + g) * t.LQ + wave * 16 + c;
        float b[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = yr[64 * j];
#pragma unroll
        for (int m = 0; m < MTD; ++m) {
            const float av = xr[16 * m] * e;
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[4 * m + j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b[j], acc[4 * m + j], 0, 0, 0);
        }
    }
}

template <int MTD>
__device__ __forceinline__ void wgrad_store_wide(const f32x4 (&acc)[4 * MTD], float *out, int wave, int g, int c) {
#pragma unroll
    for (int m = 0; m < MTD; ++m)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) out[((wave + 4 * j) * 16 + c) * (16 * MTD) + m * 16 + 4 * g + i] = acc[4 * m + j][i];
}

// ... and their one store: element (dd, n) of the D x 4A gradient at WT_l's [n][dd]
template <int NJ>
__device__ __forceinline__ void wgrad_store(const f32x4 (&acc)[NJ], float *out, int D, int NT, int wave, int g, int c) {
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) {
        const int job = wave + 4 * jj;
        if (job >= D / 16 * NT) continue;
        const int mt = job / NT, nt = job - mt * NT;
#pragma unroll
        for (int i = 0; i < 4; ++i) out[(nt * 16 + c) * D + mt * 16 + 4 * g + i] = acc[jj][i];
    }
}

template <int KP, bool TRAIN, bool WIDE>
__global__ __launch_bounds__(kBlock) void k_autoint_forward(AutoIntArgs a) {
    constexpr int Q4 = KP / 4, LX0 = kAutoIntD0 + kAutoIntPad;
    extern __shared__ float4 autoint_lds[];
    const FwfmArgs &b = a.b;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, c = lane & 15;
    const int F = b.F, Fp = b.Fp, MT = Fp / 16, A = WIDE ? 64 : a.A, L = a.L, H = a.H, d = a.d, ND = d / 16, NT = A / 4;          // NT: the N tiles of 4A
    Tiles t;
    t.F = F, t.Fp = Fp, t.MT = MT, t.A = A, t.d = d, t.LA = A + kAutoIntPad, t.LQ = 4 * A + kAutoIntPad, t.LP = Fp + kAutoIntPad;
    t.X0 = reinterpret_cast<float *>(autoint_lds);          // [Fp][LX0]: X_0 = the field sums; at the end J
    t.train = TRAIN;
    t.XL = t.X0 + Fp * LX0;                                 // L tiles [Fp][LA] (scoring: 2 by turns): X_1 .. X_L; backwards X_{l+1}'s tile takes d yhat / d X_l
    t.Y = t.XL + autoint_x_tiles(L, TRAIN) * Fp * t.LA;                             // [Fp][LQ]: [Q | K | V | R], backwards [dQ | dK | dV | Gz]
    t.P = t.Y + Fp * t.LQ;                                  // [Fp][LP]: one head's probabilities
    t.DS = t.P + Fp * t.LP;                                 // [Fp][LP]: one head's dSc (a training launch only)
    t.sm = t.DS + (TRAIN ? Fp * t.LP : 0);                                // [kAutoIntSmall]
    const int LA = t.LA, LQ = t.LQ, LP = t.LP;
    float *X0 = t.X0, *Y = t.Y;
    const float4 *V4 = reinterpret_cast<const float4 *>(b.V);
    const float w0 = *b.w0;
    const float *uvec = a.D + a.hoff;
    const bool grad = TRAIN && a.train_d;
    const int qkv4 = 3 * A / 4;                             // float4 of a token's Q, K, V
    float4 *scr = TRAIN && L > 1 ? reinterpret_cast<float4 *>(a.scratch + (int64_t)blockIdx.x * autoint_scratch(Fp, A, L)) : nullptr;
    double se = 0.0, sse = 0.0, nf = 0.0;                   // thread 0
    // the dense gradient's owners: layer 0 has 1 x NT output tiles, the others A / 16 x NT; WIDE (A = 64): NT = 16, so 4 and 16 a
    // wave; else (A <= 32) NT <= 8: 2 and 4 a wave.  u's element tid + 256 j is thread tid's gu[j] (F A <= 4096, 2048 when not WIDE)
    constexpr int NJ0 = WIDE ? 4 : 2, NJ1 = WIDE ? 16 : 4, NJU = WIDE ? 16 : 8;
    f32x4 gw0[NJ0], gw1[NJ1], gw2[NJ1];
    float gu[NJU];
    if (TRAIN) {
#pragma unroll
        for (int j = 0; j < NJ0; ++j) gw0[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < NJ1; ++j) gw1[j] = gw2[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < NJU; ++j) gu[j] = 0.f;
    }

    const int64_t row_lo = (int64_t)blockIdx.x * kAutoIntRowsPerBlock;
    for (int rr = 0; rr < kAutoIntRowsPerBlock; ++rr) {
        const int64_t row = row_lo + rr;
        if (row >= b.rows) break;            // (the same for every thread)
        const int64_t E0 = b.row_ptr[row];
        const int ne = (int)(b.row_ptr[row + 1] - E0);
        __syncthreads();                     // the previous row has been read
        for (int i = tid; i < Fp * LX0 / 4; i += kBlock) reinterpret_cast<float4 *>(X0)[i] = f4zero();
        __syncthreads();
        // the field sums: a lane group per entry, the head of a same-field run sums its run in ascending order
        for (int it = tid; it < ne * Q4; it += kBlock) {
            const int p = it / Q4, q = it % Q4;
            const int rb = b.run[E0 + p];
            if (rb == 0) continue;
            float4 s = f4zero();
            for (int j = 0; j < rb; ++j) {
                const float x = b.val[E0 + p + j];
                const float4 v = V4[(int64_t)b.col[E0 + p + j] * Q4 + q];
                s.x = fmaf(x, v.x, s.x);
                s.y = fmaf(x, v.y, s.y);
                s.z = fmaf(x, v.z, s.z);
                s.w = fmaf(x, v.w, s.w);
            }
            *reinterpret_cast<float4 *>(X0 + (int)b.fld[E0 + p] * LX0 + 4 * q) = s;
        }
        // the linear term: wave 0, a lane per entry, a fixed tree
        if (wave == 0) {
            float lin = 0.f;
            if (lane < ne) lin = __fmul_rn(b.w[b.col[E0 + lane]], b.val[E0 + lane]);
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) lin += __shfl_xor(lin, m, 64);
            if (lane == 0) t.sm[4] = lin;
        }
        __syncthreads();
        for (int l = 0; l < L; ++l) {
            const float *Xi = t.X(l), *WT = a.D + a.woff[l];
            float *Xo = t.X(l + 1);
            const int ldi = t.ldx(l), D = l == 0 ? kAutoIntD0 : A;
            // [Q | K | V | R] = X_l W_l: B[k][n] = WT[n][k], one global_load_dwordx4 of WT[16 nt + c][16u + 4g ..]
            for (int job = wave; job < MT * NT; job += kBlock / 64) {
                const int nt = job / MT, mt = job - nt * MT;
                const float4 *arow = reinterpret_cast<const float4 *>(Xi + (mt * 16 + c) * ldi), *brow = reinterpret_cast<const float4 *>(WT + (nt * 16 + c) * D);
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                for (int u = 0; u < D / 16; ++u) acc = mfma4(arow[4 * u + g], brow[4 * u + g], acc);
#pragma unroll
                for (int i = 0; i < 4; ++i) Y[(mt * 16 + 4 * g + i) * LQ + nt * 16 + c] = acc[i];
            }
            __syncthreads();
            if (TRAIN && l < L - 1)          // Q, K, V of a layer that is not the last: to the workgroup's scratch (the thread that reads them back)
                for (int i = tid; i < Fp * qkv4; i += kBlock) scr[l * Fp * qkv4 + i] = reinterpret_cast<const float4 *>(Y + i / qkv4 * LQ)[i % qkv4];
            for (int h = 0; h < H; ++h) {
                head_softmax<false>(t, h, wave, g, c);
                __syncthreads();
                // O^h = P^h V^h, then X_{l+1} = relu(O + R) on the real tokens, 0 below them
                for (int job = wave; job < MT * ND; job += kBlock / 64) {
                    const int mt = job / ND, n0 = h * d + (job - mt * ND) * 16;
                    const float4 *prow = reinterpret_cast<const float4 *>(t.P + (mt * 16 + c) * LP);
                    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                    for (int u = 0; u < MT; ++u) {
                        const float *vp = Y + (16 * u + 4 * g) * LQ + 2 * A + n0 + c;
                        acc = mfma4(prow[4 * u + g], make_float4(vp[0], vp[LQ], vp[2 * LQ], vp[3 * LQ]), acc);
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int f = mt * 16 + 4 * g + i;
                        Xo[f * LA + n0 + c] = f < F ? fmaxf(acc[i] + Y[f * LQ + 3 * A + n0 + c], 0.f) : 0.f;
                    }
                }
                __syncthreads();             // P is free for the next head; after the last head X_{l+1} is whole
            }
        }
        // <vec(X_L), u>: thread tid the elements tid, tid + 256, ..., a fixed tree over the lanes, the four waves' sums in one order
        const float *XLast = t.X(L);
        float cr = 0.f;
        for (int i = tid; i < F * A; i += kBlock) cr = fmaf(XLast[i / A * LA + i % A], uvec[i], cr);
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) cr += __shfl_xor(cr, m, 64);
        if (lane == 0) t.sm[wave] = cr;
        __syncthreads();
        if (tid == 0) {
            const float yh = (w0 + t.sm[4]) + ((t.sm[0] + t.sm[1]) + (t.sm[2] + t.sm[3]));
            b.yhat[row] = yh;
            if (TRAIN) {
                float z;
                const float e = b.loss == kLossLogistic ? pair_sigma_residual(yh, b.y[row] > 0.f, z) : yh - b.y[row];
                b.e[row] = e;
                t.sm[5] = e;
                se += (double)e;
                sse += (double)e * (double)e;
                nf += isfinite(yh) ? 0.0 : 1.0;
            }
        }
        if (!TRAIN) continue;
        __syncthreads();
        const float e = t.sm[5];
        if (grad) {
#pragma unroll
            for (int j = 0; j < NJU; ++j) {
                const int i = tid + kBlock * j;
                if (i < F * A) gu[j] = fmaf(e, XLast[i / A * LA + i % A], gu[j]);
            }
        }
        // backwards, d yhat / d . of this row
        for (int l = L - 1; l >= 0; --l) {
            const float *Xi = t.X(l), *Xn = t.X(l + 1), *Gin = l == L - 1 ? nullptr : t.X(l + 2), *WT = a.D + a.woff[l];
            const int ldi = t.ldx(l), D = l == 0 ? kAutoIntD0 : A;
            if (l < L - 1)
                for (int i = tid; i < Fp * qkv4; i += kBlock) reinterpret_cast<float4 *>(Y + i / qkv4 * LQ)[i % qkv4] = scr[l * Fp * qkv4 + i];
            // Gz = G o [Z > 0] into R's place; G_L = u on the real tokens
            for (int i = tid; i < Fp * A; i += kBlock) {
                const int f = i / A, j = i - f * A;
                const float gv = f < F ? (Gin ? Gin[f * LA + j] : uvec[i]) : 0.f;
                Y[f * LQ + 3 * A + j] = Xn[f * LA + j] > 0.f ? gv : 0.f;
            }
            __syncthreads();
            for (int h = 0; h < H; ++h) {
                head_softmax<true>(t, h, wave, g, c);
                __syncthreads();
                // dV^h = P^T Gz^h, dQ^h = dSc K^h, dK^h = dSc^T Q^h: 3 MT ND <= 24 jobs, held across the barrier behind which no wave
                // reads Q^h, K^h, V^h any more, then written in their place
                f32x4 o[6];
#pragma unroll
                for (int jj = 0; jj < 6; ++jj) {
                    const int job = wave + 4 * jj;
                    o[jj] = (f32x4){0.f, 0.f, 0.f, 0.f};
                    if (job >= 3 * MT * ND) continue;
                    const int which = job / (MT * ND), rem = job - which * MT * ND, mt = rem / ND, n0 = h * d + (rem - mt * ND) * 16;
                    if (which == 0) o[jj] = lds_product(o[jj], t.P + mt * 16, 1, LP, Y + 3 * A + n0, LQ, Fp / 4, 1.f, g, c);
                    else if (which == 1) o[jj] = lds_product(o[jj], t.DS + mt * 16 * LP, LP, 1, Y + A + n0, LQ, Fp / 4, 1.f, g, c);
                    else o[jj] = lds_product(o[jj], t.DS + mt * 16, 1, LP, Y + n0, LQ, Fp / 4, 1.f, g, c);
                }
                __syncthreads();
#pragma unroll
                for (int jj = 0; jj < 6; ++jj) {
                    const int job = wave + 4 * jj;
                    if (job >= 3 * MT * ND) continue;
                    const int which = job / (MT * ND), rem = job - which * MT * ND, mt = rem / ND, n0 = h * d + (rem - mt * ND) * 16;
                    const int col = (which == 0 ? 2 * A : (which == 1 ? 0 : A)) + n0 + c;
#pragma unroll
                    for (int i = 0; i < 4; ++i) Y[(mt * 16 + 4 * g + i) * LQ + col] = o[jj][i];
                }
            }
            __syncthreads();                 // Y = [dQ | dK | dV | Gz] is whole
            if (grad) {
                if constexpr (WIDE) {
                    if (l == 0) wgrad_add_wide<1>(gw0, Xi, ldi, t, e, wave, g, c);
                    else if (l == 1) wgrad_add_wide<4>(gw1, Xi, ldi, t, e, wave, g, c);
                    else wgrad_add_wide<4>(gw2, Xi, ldi, t, e, wave, g, c);
                } else {
                    if (l == 0) wgrad_add(gw0, Xi, ldi, 1, NT, t, e, wave, g, c);
                    else if (l == 1) wgrad_add(gw1, Xi, ldi, A / 16, NT, t, e, wave, g, c);
                    else wgrad_add(gw2, Xi, ldi, A / 16, NT, t, e, wave, g, c);
                }
                __syncthreads();             // X_0's tile is about to take J
            }
            // d yhat / d X_l = Y W_l^T: B[k][n] = WT[k][n], four global_load_dword of WT[16u + 4g + j][16 nt + c]
            float *out = l == 0 ? X0 : t.X(l + 1);
            const int ldo = t.ldx(l == 0 ? 0 : 1);
            for (int job = wave; job < MT * (D / 16); job += kBlock / 64) {
                const int nt = job / MT, mt = job - nt * MT;
                const float4 *yrow = reinterpret_cast<const float4 *>(Y + (mt * 16 + c) * LQ);
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                for (int u = 0; u < NT; ++u) {
                    const float *wp = WT + (16 * u + 4 * g) * D + nt * 16 + c;
                    acc = mfma4(yrow[4 * u + g], make_float4(wp[0], wp[D], wp[2 * D], wp[3 * D]), acc);
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) out[(mt * 16 + 4 * g + i) * ldo + nt * 16 + c] = acc[i];
            }
            __syncthreads();
        }
        // per entry x_a J[f_a]: a lane group per entry
        for (int it = tid; it < ne * Q4; it += kBlock) {
            const int p = it / Q4, q = it % Q4;
            const float4 jf = *reinterpret_cast<const float4 *>(X0 + (int)b.fld[E0 + p] * LX0 + 4 * q);
            reinterpret_cast<float4 *>(b.dz)[(E0 + p - b.nnz0) * Q4 + q] = f4mul(jf, b.val[E0 + p]);
        }
    }
    if (TRAIN) {
        if (tid == 0) {
            double *out = b.bsum + (int64_t)blockIdx.x * 4;
            out[0] = se;
            out[1] = sse;
            out[2] = nf;
            out[3] = 0.0;
        }
        if (grad) {                          // the workgroup's partial of the dense gradient: every element has one owner, one store
            float *part = a.gpart + (int64_t)blockIdx.x * a.total;
            if constexpr (WIDE) {
                wgrad_store_wide<1>(gw0, part + a.woff[0], wave, g, c);
                if (L > 1) wgrad_store_wide<4>(gw1, part + a.woff[1], wave, g, c);
                if (L > 2) wgrad_store_wide<4>(gw2, part + a.woff[2], wave, g, c);
            } else {
                wgrad_store(gw0, part + a.woff[0], kAutoIntD0, NT, wave, g, c);
                if (L > 1) wgrad_store(gw1, part + a.woff[1], A, NT, wave, g, c);
                if (L > 2) wgrad_store(gw2, part + a.woff[2], A, NT, wave, g, c);
            }
#pragma unroll
            for (int j = 0; j < NJU; ++j)
                if (tid + kBlock * j < F * A) part[a.hoff + tid + kBlock * j] = gu[j];
        }
    }
}

// A thread per dense parameter: its partials — workgroup s into accumulator s % 8 in order, the eight in a fixed tree: eight loads in
// flight — then the step on g / |B| + regd theta.
template <bool ADAGRAD>
__global__ __launch_bounds__(kBlock) void k_autoint_dupdate(AutoIntArgs a) {
    const int idx = blockIdx.x * kBlock + threadIdx.x;
    if (idx >= a.total) return;
    const float *src = a.gpart + idx;
    float s8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < a.n_splits; s += 8)
#pragma unroll
        for (int j = 0; j < 8; ++j) s8[j] += s + j < a.n_splits ? src[(int64_t)(s + j) * a.total] : 0.f;
    const float sum = ((s8[0] + s8[1]) + (s8[2] + s8[3])) + ((s8[4] + s8[5]) + (s8[6] + s8[7]));
    float th = a.D[idx];
    const float gh = fmaf(a.regd, th, sum * a.b.invb);
    if (ADAGRAD) {
        float n = a.ND[idx];
        adagrad_step(th, n, gh, a.b.eta, a.b.eps);
        a.ND[idx] = n;
    } else {
        th = th - a.b.eta * gh;
    }
    a.D[idx] = th;
}

template <int KP>
hipError_t forward_kp(const AutoIntArgs &a, bool train, hipStream_t s) {
    const size_t lds = autoint_forward_lds(a.b.Fp, a.A, a.L, train);
    const bool wide = a.A > 32;              // the instance's dense-gradient accumulators are sized for A = 64 or for A <= 32
    const void *fn = train ? (wide ? reinterpret_cast<const void *>(&k_autoint_forward<KP, true, true>) : reinterpret_cast<const void *>(&k_autoint_forward<KP, true, false>))
                           : reinterpret_cast<const void *>(&k_autoint_forward<KP, false, false>);
    if (lds > 65536) {                       // above the default: up to what the device gives a workgroup (checked at model creation)
        const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    dim3 g((unsigned)autoint_forward_blocks(a.b.rows)), b(kBlock);
    if (train && wide) hipLaunchKernelGGL((k_autoint_forward<KP, true, true>), g, b, lds, s, a);
    else if (train) hipLaunchKernelGGL((k_autoint_forward<KP, true, false>), g, b, lds, s, a);
    else hipLaunchKernelGGL((k_autoint_forward<KP, false, false>), g, b, lds, s, a);
    return hipGetLastError();
}

bool shape_ok(const AutoIntArgs &a) {
    return a.L >= 1 && a.L <= kAutoIntMaxLayers && (a.H == 1 || a.H == 2 || a.H == 4) && (a.d == 16 || a.d == 32) && a.A == a.H * a.d &&
           a.A <= kAutoIntMaxWidth && a.b.F >= 1 && a.b.F <= 64 && a.b.Fp == (a.b.F + 15) / 16 * 16 && a.k >= 1 && a.k <= a.b.Kp;
}

}  // namespace

hipError_t launch_autoint_forward(const AutoIntArgs &a, bool train, hipStream_t s) {
    const FwfmArgs &b = a.b;
    if (b.rows <= 0) return hipSuccess;
    if (!b.V || !b.w || !b.w0 || !a.D || !b.row_ptr || !b.yhat || !shape_ok(a)) return hipErrorInvalidValue;
    if (train && (!b.y || !b.e || !b.bsum || !b.dz || (a.L > 1 && !a.scratch) || (a.train_d && (!a.gpart || a.n_splits != autoint_forward_blocks(b.rows)))))
        return hipErrorInvalidValue;
    switch (b.Kp) {
        case 4: return forward_kp<4>(a, train, s);
        case 8: return forward_kp<8>(a, train, s);
        case 16: return forward_kp<16>(a, train, s);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_autoint_dupdate(const AutoIntArgs &a, bool adagrad, hipStream_t s) {
    if (a.b.rows <= 0) return hipSuccess;
    if (!a.D || !a.gpart || (adagrad && !a.ND) || a.total < 1 || a.n_splits < 1) return hipErrorInvalidValue;
    dim3 g((unsigned)((a.total + kBlock - 1) / kBlock)), b(kBlock);
    if (adagrad) hipLaunchKernelGGL(k_autoint_dupdate<true>, g, b, 0, s, a);
    else hipLaunchKernelGGL(k_autoint_dupdate<false>, g, b, 0, s, a);
    return hipGetLastError();
}

}  // namespace fmhip
