// fm_afm.hip — the kernels of the Attentional Factorization Machine (include/fmhip_afm.h; DESIGN.md, "AFM"): gfx950, wave64.
//   k_afm_forward  a workgroup of four waves owns kAfmRowsPerBlock rows; wave w takes the rows w, w + 4, .. and carries a row from its
//                  entries to its dz ALONE: the field sums S [Fp][Kp + pad], a training launch's J and one score per pair live in the
//                  wave's own LDS region, the dense part (W, b, h, p) in its registers, and nothing inside the row loop waits for
//                  another wave.  A TILE is (field i, a 16-block jt of j): M-row m is the pair (i, 16 jt + m), masked (score -inf,
//                  E = 0) unless i < j < F; the tiles with 16 jt + 15 <= i are skipped.  Pass 1: the scores s = <h, relu(W E + b)>, the
//                  product E W^T on the exact-f32 MFMA with the A element S_i[d] S_j[d] formed in registers, one multiply ahead of
//                  the matrix instruction.  Then the softmax over the score array, pass 2: o = sum a E and T = <p, o>, yhat, and —
//                  training — e_r and, tile by tile again, ds, dH, dE = a p + dH W, J and the dense gradients, kept in registers
//                  over all of the wave's rows.  At the end the four waves' partials are added (w0 + w1) + (w2 + w3) through LDS.
//   k_afm_dupdate  a thread per dense parameter: the workgroups' partials in block order, then the step
// v, w, w0 and the statistics: fm_fwfm.hip's backward and update launches over this forward's dz, e and bsum.
// No atomics: one writer per element, every sum in an order fixed by the data and by the constants of fm_afm.h — never by the CU count.
#include "fm_device.h"
#include "fm_finish.h"      // pair_sigma_residual
#include "fm_afm.h"

namespace fmhip {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// the wave's earlier LDS writes are visible to its later reads, in every lane
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// MFMA lane roles (v_mfma_f32_16x16x4_f32): lane (g, c) = (lane / 16, lane % 16) supplies A[c][g] and B[g][c] of a step and holds
// D[4g + r][c] in acc[r].  Step s of a product over the factors takes d = Q g + s from lane group g (Q = Kp / 4): the lane's slice of
// a row of S, and of a stored row of W, is Q consecutive floats.
//
// the lane's slice of E = S_i o S_j for the pair (i, j), 0 for a masked pair
template <int Q>
__device__ __forceinline__ void afm_e(const float *S, int ld, int i, int j, int g, bool valid, float (&E)[Q]) {
#pragma unroll
    for (int s = 0; s < Q; ++s) E[s] = valid ? S[i * ld + Q * g + s] * S[j * ld + Q * g + s] : 0.f;
}

// PAIRS_ON_ROWS: acc[nt][r] = (W E + b's product part) of pair 4g + r, unit 16 nt + c; else of pair c, unit 16 nt + 4g + r — the same
// two registers a step, handed to the matrix instruction the other way round
template <int Q, bool PAIRS_ON_ROWS>
__device__ __forceinline__ void afm_product(const float (&E)[Q], const float (&wreg)[4][Q], int NT, f32x4 (&acc)[4]) {
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        acc[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (nt >= NT) continue;              // (the same for every thread)
#pragma unroll
        for (int s = 0; s < Q; ++s)
            acc[nt] = PAIRS_ON_ROWS ? __builtin_amdgcn_mfma_f32_16x16x4f32(E[s], wreg[nt][s], acc[nt], 0, 0, 0)
                                    : __builtin_amdgcn_mfma_f32_16x16x4f32(wreg[nt][s], E[s], acc[nt], 0, 0, 0);
    }
}

__device__ __forceinline__ float sum_over_c(float v) {          // the butterfly 8, 4, 2, 1 over the 16 lanes of a group
    v += __shfl_xor(v, 8, 64);
    v += __shfl_xor(v, 4, 64);
    v += __shfl_xor(v, 2, 64);
    return v + __shfl_xor(v, 1, 64);
}

__device__ __forceinline__ float sum_over_g(float v) {          // ... and 16, 32 over the four groups
    v += __shfl_xor(v, 16, 64);
    return v + __shfl_xor(v, 32, 64);
}

template <int KP, bool TRAIN>
__global__ __launch_bounds__(kAfmBlock) void k_afm_forward(AfmArgs a) {
    extern __shared__ float4 afm_lds[];
    __shared__ float bh[2][kAfmMaxAttention];          // b and h for the backward half's second layout
    __shared__ double shs[kAfmWaves][4];
    constexpr int Q = KP / 4, LD = KP + kAfmPad;
    const FwfmArgs &b = a.b;
    const int F = b.F, Fp = b.Fp, k = a.k, t = a.t, NT = t / 16;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, c = lane & 15;
    const size_t region = afm_wave_floats(Fp, KP, TRAIN);
    float *S = reinterpret_cast<float *>(afm_lds) + wave * region;          // [Fp][LD]: the field sums
    float *J = S + Fp * LD;                                                 // [Fp][LD]: d yhat / d S (a training launch's)
    float *sc = S + (TRAIN ? 2 : 1) * Fp * LD;                              // [tiles][16]: the scores, then exp(s - max)
    const float *Wd = a.D, *bd = Wd + t * KP, *hd = bd + t, *pd = hd + t;
    const float4 *V4 = reinterpret_cast<const float4 *>(b.V);
    const float w0 = *b.w0;

    // the dense part, stationary: W's B operand (unit 16 nt + c, factors Q g ..), b and h of the lane's units, p of its factors
    float wreg[4][Q], b1[4], h1[4], preg[Q];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        const bool on = nt < NT;
#pragma unroll
        for (int s = 0; s < Q; ++s) wreg[nt][s] = on ? Wd[(16 * nt + c) * KP + Q * g + s] : 0.f;
        b1[nt] = on ? bd[16 * nt + c] : 0.f;
        h1[nt] = on ? hd[16 * nt + c] : 0.f;
    }
#pragma unroll
    for (int s = 0; s < Q; ++s) preg[s] = pd[Q * g + s];
    // a training launch's: W as the B operand of dE = dH W (unit 16 nt + 4g + r, factor c), p of factor c, and the gradients
    float wt[4][4], pc = 0.f;
    f32x4 dW[4];
    float dh[4], db[4], dp[Q];
    double se = 0.0, sse = 0.0, nf = 0.0;
    if (TRAIN) {
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) wt[nt][r] = nt < NT && c < KP ? Wd[(16 * nt + 4 * g + r) * KP + c] : 0.f;
            dW[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
            dh[nt] = db[nt] = 0.f;
        }
#pragma unroll
        for (int s = 0; s < Q; ++s) dp[s] = 0.f;
        pc = c < KP ? pd[c] : 0.f;
        if (tid < t) {
            bh[0][tid] = bd[tid];
            bh[1][tid] = hd[tid];
        }
        __syncthreads();                     // the only workgroup barrier before the tail
    }

    const int64_t row_lo = (int64_t)blockIdx.x * kAfmRowsPerBlock;
    for (int rr = wave; rr < kAfmRowsPerBlock; rr += kAfmWaves) {
        const int64_t row = row_lo + rr;
        if (row >= b.rows) break;            // (the same for every thread of the wave)
        const int64_t E0 = b.row_ptr[row];
        const int n = (int)(b.row_ptr[row + 1] - E0);
        wave_sync();                         // the previous row has been read
        for (int i = lane; i < (TRAIN ? 2 : 1) * Fp * LD / 4; i += 64) reinterpret_cast<float4 *>(S)[i] = f4zero();
        wave_sync();
        // the field sums: a lane per (entry, four factors), the head of a same-field run sums its run in ascending order
        for (int it = lane; it < n * Q; it += 64) {
            const int p = it / Q, q = it % Q;
            const int rb = b.run[E0 + p];
            if (rb == 0) continue;
            float4 s = f4zero();
            for (int u = 0; u < rb; ++u) {
                const float x = b.val[E0 + p + u];
                const float4 v = V4[(int64_t)b.col[E0 + p + u] * Q + q];
                s.x = fmaf(x, v.x, s.x);
                s.y = fmaf(x, v.y, s.y);
                s.z = fmaf(x, v.z, s.z);
                s.w = fmaf(x, v.w, s.w);
            }
            *reinterpret_cast<float4 *>(S + (int)b.fld[E0 + p] * LD + 4 * q) = s;
        }
        // the linear term: a lane per entry, a fixed tree
        float lin = 0.f;
        for (int p = lane; p < n; p += 64) lin += __fmul_rn(b.w[b.col[E0 + p]], b.val[E0 + p]);
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) lin += __shfl_xor(lin, m, 64);
        wave_sync();

        // pass 1: the scores
        int tiles = 0;
        for (int i = 0; i + 1 < F; ++i)
            for (int jt = (i + 1) >> 4; 16 * jt < F; ++jt, ++tiles) {
                const int j = 16 * jt + c;
                float E[Q];
                afm_e<Q>(S, LD, i, j, g, j > i && j < F, E);
                f32x4 acc[4];
                afm_product<Q, true>(E, wreg, NT, acc);
                float sp[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) {
                    if (nt >= NT) continue;
#pragma unroll
                    for (int r = 0; r < 4; ++r) sp[r] = fmaf(h1[nt], fmaxf(acc[nt][r] + b1[nt], 0.f), sp[r]);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) sp[r] = sum_over_c(sp[r]);
                const float mine = c == 0 ? sp[0] : (c == 1 ? sp[1] : (c == 2 ? sp[2] : sp[3]));
                const int jj = 16 * jt + 4 * g + c;          // lane (g, c < 4) stores M-row 4g + c
                if (c < 4) sc[tiles * 16 + 4 * g + c] = jj > i && jj < F ? mine : -INFINITY;
            }
        wave_sync();
        // the softmax over the score array: a fixed lane stride and tree
        float T = 0.f, invz = 0.f, o[Q];
#pragma unroll
        for (int s = 0; s < Q; ++s) o[s] = 0.f;
        if (tiles > 0) {
            const int ns = 16 * tiles;
            float mx = -INFINITY, z = 0.f;
            for (int idx = lane; idx < ns; idx += 64) mx = fmaxf(mx, sc[idx]);
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) mx = fmaxf(mx, __shfl_xor(mx, m, 64));
            for (int idx = lane; idx < ns; idx += 64) {
                const float pv = expf(sc[idx] - mx);
                sc[idx] = pv;
                z += pv;
            }
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) z += __shfl_xor(z, m, 64);
            invz = 1.f / z;
            wave_sync();
            // pass 2: o = sum a E, T = <p, o>
            int ti = 0;
            for (int i = 0; i + 1 < F; ++i)
                for (int jt = (i + 1) >> 4; 16 * jt < F; ++jt, ++ti) {
                    const int j = 16 * jt + c;
                    float E[Q];
                    afm_e<Q>(S, LD, i, j, g, j > i && j < F, E);
                    const float av = sc[ti * 16 + c] * invz;
#pragma unroll
                    for (int s = 0; s < Q; ++s) o[s] = fmaf(av, E[s], o[s]);
                }
#pragma unroll
            for (int s = 0; s < Q; ++s) {
                o[s] = sum_over_c(o[s]);
                T = fmaf(preg[s], o[s], T);
            }
            T = sum_over_g(T);
        }
        const float yh = (w0 + lin) + T;
        if (lane == 0) b.yhat[row] = yh;
        if (!TRAIN) continue;
        float z0;
        const float e = b.loss == kLossLogistic ? pair_sigma_residual(yh, b.y[row] > 0.f, z0) : yh - b.y[row];
        if (lane == 0) b.e[row] = e;
        se += (double)e;
        sse += (double)e * (double)e;
        nf += isfinite(yh) ? 0.0 : 1.0;

        // the backward half, tile by tile again
        int ti = 0;
        for (int i = 0; i + 1 < F; ++i) {
            const float si_c = c < KP ? S[i * LD + c] : 0.f;          // S_i[d = c]: the layout of dE's and dW's columns
            float ji = 0.f;
            for (int jt = (i + 1) >> 4; 16 * jt < F; ++jt, ++ti) {
                const int j = 16 * jt + c;
                float E[Q];
                afm_e<Q>(S, LD, i, j, g, j > i && j < F, E);
                // ds of pair c, then of the pairs 4g + r
                const float a2 = sc[ti * 16 + c] * invz;
                float c2 = 0.f;
#pragma unroll
                for (int s = 0; s < Q; ++s) c2 = fmaf(preg[s], E[s], c2);
                c2 = sum_over_g(c2);
                const float ds2 = a2 * (c2 - T);
                float ds1[4], a1[4], sjb[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    ds1[r] = e * __shfl(ds2, 4 * g + r, 64);
                    a1[r] = __shfl(a2, 4 * g + r, 64);
                    sjb[r] = c < KP ? S[(16 * jt + 4 * g + r) * LD + c] : 0.f;
                }
                // pairs on rows: dh, db and dW += (e dH)^T E, the pairs 4g + s the reduction
                f32x4 acc[4];
                afm_product<Q, true>(E, wreg, NT, acc);
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) {
                    if (nt >= NT) continue;
                    float dH[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float pre = acc[nt][r] + b1[nt];
                        dh[nt] = fmaf(ds1[r], fmaxf(pre, 0.f), dh[nt]);
                        dH[r] = pre > 0.f ? ds1[r] * h1[nt] : 0.f;
                        db[nt] += dH[r];
                    }
#pragma unroll
                    for (int s = 0; s < 4; ++s) dW[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(dH[s], si_c * sjb[s], dW[nt], 0, 0, 0);
                }
                // pairs on columns: dE = a p + dH W, the units 16 nt + 4g + r the reduction
                afm_product<Q, false>(E, wreg, NT, acc);
                f32x4 dE = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) {
                    if (nt >= NT) continue;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int u = 16 * nt + 4 * g + r;
                        const float d2 = acc[nt][r] + bh[0][u] > 0.f ? ds2 * bh[1][u] : 0.f;
                        dE = __builtin_amdgcn_mfma_f32_16x16x4f32(d2, wt[nt][r], dE, 0, 0, 0);
                    }
                }
                // J[i] is a column sum over the tile's M-rows, J[j] has one M-row a tile
                float js = 0.f;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float de = fmaf(a1[r], pc, dE[r]);
                    const int jj = 16 * jt + 4 * g + r;
                    js = fmaf(de, sjb[r], js);
                    if (c < KP && jj > i && jj < F) J[jj * LD + c] += de * si_c;
                }
                ji += sum_over_g(js);
                wave_sync();
            }
            if (g == 0 && c < KP) J[i * LD + c] += ji;
            wave_sync();
        }
#pragma unroll
        for (int s = 0; s < Q; ++s) dp[s] = fmaf(e, o[s], dp[s]);
        // per entry x_a J[f_a]: a lane per (entry, d), 0 in the pad slots
        for (int it = lane; it < n * KP; it += 64) {
            const int p = it / KP, d = it - p * KP;
            b.dz[(E0 + p - b.nnz0) * KP + d] = d < k ? J[(int)b.fld[E0 + p] * LD + d] * b.val[E0 + p] : 0.f;
        }
    }
    if (TRAIN) {
        // the wave's partial of D's gradient into its own region, then the four in a fixed tree
        if (a.train_d) {
            wave_sync();
            float *part = S;
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                if (nt >= NT) continue;
                const float dbs = sum_over_g(db[nt]), dhs = sum_over_g(dh[nt]);
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (c < KP) part[(16 * nt + 4 * g + r) * KP + c] = dW[nt][r];
                if (g == 0) {
                    part[t * KP + 16 * nt + c] = dbs;
                    part[t * KP + t + 16 * nt + c] = dhs;
                }
            }
#pragma unroll
            for (int s = 0; s < Q; ++s)
                if (c == 0) part[t * KP + 2 * t + Q * g + s] = dp[s];
        }
        if (lane == 0) {
            shs[wave][0] = se;
            shs[wave][1] = sse;
            shs[wave][2] = nf;
        }
        __syncthreads();
        if (a.train_d) {
            const float *P = reinterpret_cast<const float *>(afm_lds);
            float *out = a.gpart + (int64_t)blockIdx.x * a.total;
            for (int idx = tid; idx < a.total; idx += kAfmBlock)
                out[idx] = (P[idx] + P[region + idx]) + (P[2 * region + idx] + P[3 * region + idx]);
        }
        if (tid < 3) b.bsum[(int64_t)blockIdx.x * 4 + tid] = (shs[0][tid] + shs[1][tid]) + (shs[2][tid] + shs[3][tid]);
        if (tid == 3) b.bsum[(int64_t)blockIdx.x * 4 + 3] = 0.0;
    }
}

// A thread per dense parameter: its partials — block s into accumulator s % 8 in block order, the eight in a fixed tree: eight loads
// in flight — then the step on g / |B| + regd theta.
template <bool ADAGRAD>
__global__ __launch_bounds__(kBlock) void k_afm_dupdate(AfmArgs a) {
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
hipError_t forward_instance(const AfmArgs &a, bool train, hipStream_t s) {
    const size_t lds = afm_forward_lds(a.b.Fp, KP, train);
    if (lds + afm_forward_static() > (size_t)a.lds_limit) return hipErrorInvalidValue;
    if (lds + afm_forward_static() > 65536) {          // above the default: up to what the device gives a workgroup
        const void *fn = train ? reinterpret_cast<const void *>(&k_afm_forward<KP, true>) : reinterpret_cast<const void *>(&k_afm_forward<KP, false>);
        const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    dim3 g((unsigned)afm_forward_blocks(a.b.rows)), b(kAfmBlock);
    if (train) hipLaunchKernelGGL((k_afm_forward<KP, true>), g, b, lds, s, a);
    else hipLaunchKernelGGL((k_afm_forward<KP, false>), g, b, lds, s, a);
    return hipGetLastError();
}

bool shape_ok(const AfmArgs &a) {
    return a.k >= 1 && a.k <= kAfmMaxFactors && a.k <= a.b.Kp && a.t >= 16 && a.t <= kAfmMaxAttention && a.t % 16 == 0 && a.total == afm_total(a.t, a.b.Kp) &&
           a.b.F >= 1 && a.b.Fp == (a.b.F + 15) / 16 * 16 && a.b.Fp <= 64;
}

}  // namespace

hipError_t launch_afm_forward(const AfmArgs &a, bool train, hipStream_t s) {
    const FwfmArgs &b = a.b;
    if (b.rows <= 0) return hipSuccess;
    if (!b.V || !b.w || !b.w0 || !a.D || !b.row_ptr || !b.yhat || (b.Kp != 4 && b.Kp != 8 && b.Kp != 16) || !shape_ok(a)) return hipErrorInvalidValue;
    if (train && (!b.y || !b.e || !b.bsum || !b.dz || (a.train_d && (!a.gpart || a.n_splits != afm_forward_blocks(b.rows))))) return hipErrorInvalidValue;
    return b.Kp == 4 ? forward_instance<4>(a, train, s) : (b.Kp == 8 ? forward_instance<8>(a, train, s) : forward_instance<16>(a, train, s));
}

hipError_t launch_afm_dupdate(const AfmArgs &a, bool adagrad, hipStream_t s) {
    if (a.b.rows <= 0) return hipSuccess;
    if (!a.D || !a.gpart || (adagrad && !a.ND) || a.total < 1 || a.n_splits != afm_forward_blocks(a.b.rows)) return hipErrorInvalidValue;
    dim3 g((unsigned)((a.total + kBlock - 1) / kBlock)), b(kBlock);
    if (adagrad) hipLaunchKernelGGL(k_afm_dupdate<true>, g, b, 0, s, a);
    else hipLaunchKernelGGL(k_afm_dupdate<false>, g, b, 0, s, a);
    return hipGetLastError();
}

}  // namespace fmhip
