// fm_cin.hip — the kernels of xDeepFM's Compressed Interaction Network (include/fmhip_cin.h; DESIGN.md, "CIN"): gfx950, wave64.
//   k_cin_forward  a workgroup of eight waves owns kCinRowsPerBlock rows and walks them in tiles of rt rows, Mp = rt k M-rows (row,
//                  d).  X^0 [Mp][F] (the field sums, one M-row per factor) and every X^l [Mp][H_l] stay resident in LDS.  A layer is
//                  one product on the exact-f32 MFMA, M = the M-rows, N = H_l, the reduction over (i, j): the A operand
//                  X^{l-1}[m][i] X^0[m][j] is formed in registers, one multiply ahead of each matrix instruction, from the lane's
//                  own slice of X^0[m][.] (held for the whole layer) and one ds_read_b128 of X^{l-1}[m][i .. i+3] per four i; the B
//                  operand streams along W_l's stored rows, one dwordx4 a lane.  A training launch goes on backwards over the same
//                  tiles: G^L = u^L, and per layer dZ = G^l W_l as the transposed product, whose accumulator — (i, four j) of the
//                  lane's own M-rows — is contracted at once with X^0 into G^{l-1} and with X^{l-1} into J; at the end a thread per
//                  (entry, d) writes x_a J[f_a] to the workspace dz.  Also the scorer
//   k_cin_wgrad    dW_l[h][i][j] = sum_m e_m G^l[m][h] X^{l-1}[m][i] X^0[m][j] over the stored tiles: a workgroup per (a few i, all
//                  h, all j) and row split stages kCinGradStage M-rows through LDS and forms the Khatri-Rao operand in registers;
//                  behind them come the workgroups of u's column sums sum_r e_r p_r
//   k_cin_dupdate  a thread per dense parameter: the splits' partials in split order, then the step
// v, w, w0 and the statistics: fm_fwfm.hip's backward and update launches over this forward's dz, e and bsum.
// No atomics: one writer per element, every sum in an order fixed by the data and by the constants of fm_cin.h — never by the CU count.
#include "fm_device.h"
#include "fm_finish.h"      // pair_sigma_residual
#include "fm_cin.h"

namespace fmhip {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// MFMA lane roles (v_mfma_f32_16x16x4_f32): lane (g, c) = (lane / 16, lane % 16) supplies A[c][g] and B[g][c] of a step and holds
// D[4g + r][c] in acc[r].
//
// One unit of a layer's forward product: MTW M tiles (mg MTW ..) by NTW N tiles (n0 ..), the whole reduction.  Step (i, t, s) takes
// field j = 16 t + 4 s + g from lane group g: A = Xp[m][i] X0[m][j], B = W[n][i] at position 16 t + 4 g + s (fm_cin.h) — component s
// of the lane's dwordx4 at 16 t + 4 g.  A tile index past the last is clamped: its accumulators are computed and never handed out.
template <int MTW, int NTW, typename Epi>
__device__ __forceinline__ void cin_unit(const float *Xp, int ldp, int ni, const float *X0, int ld0, int F, int Fp, const float *__restrict__ W, int hp,
                                         int TM, int mg, int n0, int nt, int g, int c, Epi epi) {
    int mrow[MTW];
    float x0r[MTW][4][4];
#pragma unroll
    for (int q = 0; q < MTW; ++q) {
        mrow[q] = 16 * min(mg * MTW + q, TM - 1) + c;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int s = 0; s < 4; ++s) x0r[q][t][s] = 16 * t < Fp ? X0[mrow[q] * ld0 + 16 * t + 4 * s + g] : 0.f;
    }
    const float *wl[NTW];
#pragma unroll
    for (int nq = 0; nq < NTW; ++nq) wl[nq] = W + (int64_t)(16 * min(n0 + nq, nt - 1) + c) * hp * Fp + 4 * g;
    f32x4 acc[MTW][NTW];
#pragma unroll
    for (int q = 0; q < MTW; ++q)
#pragma unroll
        for (int nq = 0; nq < NTW; ++nq) acc[q][nq] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int i4 = 0; i4 < ni; i4 += 4) {
        f32x4 xa[MTW];
#pragma unroll
        for (int q = 0; q < MTW; ++q) xa[q] = *reinterpret_cast<const f32x4 *>(Xp + mrow[q] * ldp + i4);
#pragma unroll
        for (int ii = 0; ii < 4; ++ii)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (16 * t >= F) break;          // (the same for every thread)
                f32x4 bv[NTW];
#pragma unroll
                for (int nq = 0; nq < NTW; ++nq) bv[nq] = *reinterpret_cast<const f32x4 *>(wl[nq] + (int64_t)(i4 + ii) * Fp + 16 * t);
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    if (16 * t + 4 * s >= F) break;
#pragma unroll
                    for (int q = 0; q < MTW; ++q) {
                        const float av = xa[q][ii] * x0r[q][t][s];
#pragma unroll
                        for (int nq = 0; nq < NTW; ++nq) acc[q][nq] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[nq][s], acc[q][nq], 0, 0, 0);
                    }
                }
            }
    }
#pragma unroll
    for (int q = 0; q < MTW; ++q)
#pragma unroll
        for (int nq = 0; nq < NTW; ++nq)
            if (mg * MTW + q < TM && n0 + nq < nt) epi(mg * MTW + q, n0 + nq, acc[q][nq]);
}

// OUT[Mp][N] = (Xp (.) X0) W^T: the units (M tile group, chunk of up to four N tiles) go round the waves.  epi(mt, nt, acc): the lane
// holds OUT[16 mt + 4g + r][16 nt + c] in acc[r]
template <int MTW, typename Epi>
__device__ __forceinline__ void cin_product(const float *Xp, int ldp, int ni, const float *X0, int ld0, int F, int Fp, const float *__restrict__ W, int hp, int N,
                                            int TM, int wave, int g, int c, Epi epi) {
    const int nt = N / 16, NC = (nt + 3) / 4, MG = (TM + MTW - 1) / MTW;
    for (int unit = wave; unit < MG * NC; unit += kCinWaves) {
        const int mg = unit / NC, n0 = 4 * (unit - mg * NC), cnt = nt - n0;
        if (cnt == 1) cin_unit<MTW, 1>(Xp, ldp, ni, X0, ld0, F, Fp, W, hp, TM, mg, n0, nt, g, c, epi);
        else if (cnt == 2) cin_unit<MTW, 2>(Xp, ldp, ni, X0, ld0, F, Fp, W, hp, TM, mg, n0, nt, g, c, epi);
        else cin_unit<MTW, 4>(Xp, ldp, ni, X0, ld0, F, Fp, W, hp, TM, mg, n0, nt, g, c, epi);
    }
}

// The backward half of a layer for the M tile mt and the i split sp of S: for every fourth-of-a-tile i (lane c: i = 4 ib + c / 4, the
// positions 16 t + 4 (c % 4) + s, s = 0 .. 3, one dwordx4 of W[h][i]) the product dZ[m][i][j] = sum_h Gin[m][h] W[h][i][j], four
// accumulators (s) of the lane's M-rows 16 mt + 4g + r and field j = 16 t + 4 s + c % 4.  Contracted in registers:
//   Gout[m][i] = sum_j dZ X0[m][j] (+ uprev[i]): in the lane over (t, s), then over the four lanes c % 4
//   J[m][j]   += sum_i dZ Xp[m][i]: in the lane over ib, then over the four lanes c / 4, then into the split's partial Jp
__device__ __forceinline__ void cin_backward_unit(const float *Gin, int ldg, int H, const float *Xp, int ldp, int ni, const float *X0, int ld0, int F, int Fp,
                                                  const float *__restrict__ W, int hp, const float *uprev, float *Gout, float *Jp, int mt, int sp, int S, int g,
                                                  int c) {
    const int ii = c >> 2, gg = c & 3, m0 = 16 * mt + 4 * g;
    const float *ga = Gin + (16 * mt + c) * ldg + 4 * g;
    const int64_t hs = (int64_t)hp * Fp;
    f32x4 jacc[4][4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int s = 0; s < 4; ++s) jacc[t][s] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int ib = sp; ib < ni / 4; ib += S) {
        const int i = 4 * ib + ii;
        float xp[4], gs[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 4; ++r) xp[r] = Xp[(m0 + r) * ldp + i];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (16 * t >= F) break;              // (the same for every thread)
            f32x4 acc[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) acc[s] = (f32x4){0.f, 0.f, 0.f, 0.f};
            const float *wp = W + (4 * g * hs + (int64_t)i * Fp + 16 * t + 4 * gg);
            for (int u = 0; u < H / 16; ++u) {
                const f32x4 av = *reinterpret_cast<const f32x4 *>(ga + 16 * u);
#pragma unroll
                for (int hh = 0; hh < 4; ++hh) {
                    const f32x4 bv = *reinterpret_cast<const f32x4 *>(wp + (16 * u + hh) * hs);
#pragma unroll
                    for (int s = 0; s < 4; ++s) acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[hh], bv[s], acc[s], 0, 0, 0);
                }
            }
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    gs[r] = fmaf(acc[s][r], X0[(m0 + r) * ld0 + 16 * t + 4 * s + gg], gs[r]);
                    jacc[t][s][r] = fmaf(acc[s][r], xp[r], jacc[t][s][r]);
                }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            gs[r] += __shfl_xor(gs[r], 1, 64);
            gs[r] += __shfl_xor(gs[r], 2, 64);
            if (gg == 0) Gout[(m0 + r) * ldg + i] = uprev ? gs[r] + uprev[i] : gs[r];
        }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        if (16 * t >= F) break;
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float v = jacc[t][s][r];
                v += __shfl_xor(v, 4, 64);
                v += __shfl_xor(v, 8, 64);
                if (ii == 0) Jp[(m0 + r) * ld0 + 16 * t + 4 * s + gg] += v;
            }
    }
}

template <int MTW, bool TRAIN>
__global__ __launch_bounds__(kCinBlock) void k_cin_forward(CinArgs a) {
    extern __shared__ float4 cin_lds[];
    __shared__ double sh[kCinMaxTile][3];
    const FwfmArgs &b = a.b;
    const int k = a.k, F = b.F, Fp = a.Fp, L = a.L, rt = a.rt, KP = b.Kp, Q = KP / 4, SH = cin_hsum(a);
    const int Mp = cin_round16(rt * k), TM = Mp / 16, S = cin_splits(TM);
    int hmax = Fp, xtot = 0;
    for (int l = 1; l <= L; ++l) {
        hmax = max(hmax, a.H[l]);
        if (l < L) xtot += a.H[l] + kCinPad;
    }
    const int L0 = Fp + kCinPad, LG = hmax + kCinPad;
    float *X0 = reinterpret_cast<float *>(cin_lds);          // [Mp][L0]: the field sums, M-row (row, d), fields in natural order
    float *Xl = X0 + Mp * L0;                                // X^1 .. X^{L-1}, [Mp][H_l + pad] each
    float *GA = Xl + Mp * xtot;                              // [Mp][LG]: X^L, then G^L, G^{L-2}, ..
    float *GB = GA + Mp * LG;                                // [Mp][LG]: G^{L-1}, .. (a training launch's)
    float *Jp = GB + Mp * LG;                                // [S][Mp][L0]: the i splits' partials of J (likewise)
    float *rlin = TRAIN ? Jp + S * Mp * L0 : GB, *rcross = rlin + rt;          // [rt] each
    int *rp = reinterpret_cast<int *>(rcross + rt);          // [rt + 1] the rows' entry offsets from the tile's first entry
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, c = lane & 15;
    const float4 *V4 = reinterpret_cast<const float4 *>(b.V);
    const float w0 = *b.w0;
    const float *uvec = a.D + a.uoff;
    const bool store = TRAIN && a.train_d;
    double se = 0.0, sse = 0.0, nf = 0.0;    // thread j < rt: the rows j of every tile
    // X^l (l < L) in LDS, and its pitch
    auto xat = [&](int l, int &ld) -> float * {
        if (l == 0) {
            ld = L0;
            return X0;
        }
        int off = 0;
        for (int q = 1; q < l; ++q) off += a.H[q] + kCinPad;
        ld = a.H[l] + kCinPad;
        return Xl + Mp * off;
    };

    const int64_t row_lo = (int64_t)blockIdx.x * kCinRowsPerBlock;
    for (int t0 = 0; t0 < kCinRowsPerBlock; t0 += rt) {
        const int64_t r0 = row_lo + t0;
        if (r0 >= b.rows) break;             // (the same for every thread)
        const int nr = (int)min((int64_t)rt, b.rows - r0), nm = nr * k;
        const int64_t E0 = b.row_ptr[r0];
        __syncthreads();                     // the previous tile has been read
        for (int i = tid; i < Mp * L0 / 4; i += kCinBlock) reinterpret_cast<float4 *>(X0)[i] = f4zero();
        if (TRAIN)
            for (int i = tid; i < S * Mp * L0 / 4; i += kCinBlock) reinterpret_cast<float4 *>(Jp)[i] = f4zero();
        if (tid <= nr) rp[tid] = (int)(b.row_ptr[r0 + tid] - E0);
        __syncthreads();
        const int ne = rp[nr];
        // the field sums: a lane group per entry, the head of a same-field run sums its run in ascending order
        for (int it = tid; it < ne * Q; it += kCinBlock) {
            const int p = it / Q, q = it % Q;
            const int rb = b.run[E0 + p];
            if (rb == 0) continue;
            int j = 0;                       // the entry's row: the last j with rp[j] <= p
            for (int step = rt / 2; step >= 1; step >>= 1)
                if (j + step < nr && rp[j + step] <= p) j += step;
            float4 s = f4zero();
            for (int t = 0; t < rb; ++t) {
                const float x = b.val[E0 + p + t];
                const float4 v = V4[(int64_t)b.col[E0 + p + t] * Q + q];
                s.x = fmaf(x, v.x, s.x);
                s.y = fmaf(x, v.y, s.y);
                s.z = fmaf(x, v.z, s.z);
                s.w = fmaf(x, v.w, s.w);
            }
            float *dst = X0 + (j * k + 4 * q) * L0 + (int)b.fld[E0 + p];
            if (4 * q < k) dst[0] = s.x;
            if (4 * q + 1 < k) dst[L0] = s.y;
            if (4 * q + 2 < k) dst[2 * L0] = s.z;
            if (4 * q + 3 < k) dst[3 * L0] = s.w;
        }
        // the linear term: a wave per row, a lane per entry, a fixed tree
        for (int j = wave; j < nr; j += kCinWaves) {
            const int e0 = rp[j], n = rp[j + 1] - e0;
            float lin = 0.f;
            if (lane < n) lin = __fmul_rn(b.w[b.col[E0 + e0 + lane]], b.val[E0 + e0 + lane]);
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) lin += __shfl_xor(lin, m, 64);
            if (lane == 0) rlin[j] = lin;
        }
        __syncthreads();
        if (store) {                         // X^0 for the weight gradients
            float *out = a.xw[0] + r0 * k * Fp;
            for (int i = tid; i < nm * Fp; i += kCinBlock) out[i] = X0[i / Fp * L0 + i % Fp];
        }
        // the layers: X^l = (X^{l-1} (.) X^0) W_l^T, the last into GA
        for (int l = 1; l <= L; ++l) {
            int ldp, ldo = LG;
            const float *Xp = xat(l - 1, ldp);
            float *Xo = l < L ? xat(l, ldo) : GA;
            const int H = a.H[l];
            cin_product<MTW>(Xp, ldp, cin_ni(a, l), X0, L0, F, Fp, a.D + a.woff[l - 1], cin_hp(a, l), H, TM, wave, g, c, [&](int mt, int nt, const f32x4 &acc) {
#pragma unroll
                for (int r = 0; r < 4; ++r) Xo[(16 * mt + 4 * g + r) * ldo + 16 * nt + c] = acc[r];
            });
            __syncthreads();
            if (store && l < L) {
                float *out = a.xw[l] + r0 * k * H;
                for (int i = tid; i < nm * H; i += kCinBlock) out[i] = Xo[i / H * ldo + i % H];
            }
        }
        // p^l[h] = sum_d X^l[(row, d)][h] in ascending d, and the CIN term <p, u>: a wave per row, lane i the maps i, i + 64, a fixed tree
        for (int j = wave; j < nr; j += kCinWaves) {
            float t = 0.f;
            int uo = 0;
            for (int l = 1; l <= L; ++l) {
                int ld = LG;
                const float *X = l < L ? xat(l, ld) : GA;
                for (int h = lane; h < a.H[l]; h += 64) {
                    float p = 0.f;
                    for (int d = 0; d < k; ++d) p += X[(j * k + d) * ld + h];
                    if (store) a.pw[(r0 + j) * SH + uo + h] = p;
                    t = fmaf(p, uvec[uo + h], t);
                }
                uo += a.H[l];
            }
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) t += __shfl_xor(t, m, 64);
            if (lane == 0) rcross[j] = t;
        }
        __syncthreads();
        if (tid < nr) {
            const float yh = (w0 + rlin[tid]) + rcross[tid];
            b.yhat[r0 + tid] = yh;
            if (TRAIN) {
                float z;
                const float e = b.loss == kLossLogistic ? pair_sigma_residual(yh, b.y[r0 + tid] > 0.f, z) : yh - b.y[r0 + tid];
                b.e[r0 + tid] = e;
                se += (double)e;
                sse += (double)e * (double)e;
                nf += isfinite(yh) ? 0.0 : 1.0;
            }
        }
        if (!TRAIN) continue;
        // backwards, d yhat / d . per M-row: G^L = u^L in X^L's place
        {
            const int HL = a.H[L];
            const float *uL = uvec + SH - HL;
            for (int idx = tid; idx < Mp * HL; idx += kCinBlock) GA[idx / HL * LG + idx % HL] = uL[idx % HL];
        }
        __syncthreads();
        float *Gin = GA, *Gout = GB;
        int uo = SH - a.H[L];                // where u^l starts
        for (int l = L; l >= 1; --l) {
            const int H = a.H[l];
            if (store) {
                float *out = a.gw[l - 1] + r0 * k * H;
                for (int i = tid; i < nm * H; i += kCinBlock) out[i] = Gin[i / H * LG + i % H];
            }
            int ldp;
            const float *Xp = xat(l - 1, ldp);
            if (l >= 2) uo -= a.H[l - 1];
            for (int unit = wave; unit < TM * S; unit += kCinWaves) {
                const int mt = unit / S, sp = unit - mt * S;
                cin_backward_unit(Gin, LG, H, Xp, ldp, cin_ni(a, l), X0, L0, F, Fp, a.D + a.woff[l - 1], cin_hp(a, l), l >= 2 ? uvec + uo : nullptr, Gout,
                                  Jp + sp * Mp * L0, mt, sp, S, g, c);
            }
            __syncthreads();
            float *t = Gin;
            Gin = Gout;
            Gout = t;
        }
        // J = the splits' partials in split order + G^0 (now in Gin), into the first partial
        for (int idx = tid; idx < nm * F; idx += kCinBlock) {
            const int m = idx / F, j = idx - m * F;
            float t = Jp[m * L0 + j];
            for (int sp = 1; sp < S; ++sp) t += Jp[(sp * Mp + m) * L0 + j];
            Jp[m * L0 + j] = t + Gin[m * LG + j];
        }
        __syncthreads();
        // per entry x_a J[f_a]: a thread per (entry, d), 0 in the pad slots
        for (int it = tid; it < ne * KP; it += kCinBlock) {
            const int p = it / KP, d = it - p * KP;
            int j = 0;
            for (int step = rt / 2; step >= 1; step >>= 1)
                if (j + step < nr && rp[j + step] <= p) j += step;
            b.dz[(E0 + p - b.nnz0) * KP + d] = d < k ? Jp[(j * k + d) * L0 + (int)b.fld[E0 + p]] * b.val[E0 + p] : 0.f;
        }
    }
    if (TRAIN) {
        __syncthreads();                     // (sh is the kernel's own: nothing above touches it)
        if (tid < kCinMaxTile) {
            sh[tid][0] = tid < rt ? se : 0.0;
            sh[tid][1] = tid < rt ? sse : 0.0;
            sh[tid][2] = tid < rt ? nf : 0.0;
        }
        __syncthreads();
        if (tid < 3) {
            double t = sh[0][tid];
            for (int j = 1; j < rt; ++j) t += sh[j][tid];
            b.bsum[(int64_t)blockIdx.x * 4 + tid] = t;
        }
        if (tid == 3) b.bsum[(int64_t)blockIdx.x * 4 + 3] = 0.0;
    }
}

// The weight gradients on the same MFMA, the reduction over the M-rows of a row split.  A workgroup's output is every h of TI
// consecutive i (TI Fp = 64 columns, 48 at Fp = 48): wave w owns the h tiles w and w + 4 by all column tiles.  A stage is
// kCinGradStage M-rows in LDS: A[m][h] = e_m G^l[m][h], XP[m][TI] = X^{l-1}[m][i0 ..] and XZ[m][Fp] = X^0[m][.] in W's position order;
// the B element XP XZ is formed in registers ahead of its matrix instructions.  A's pitch of H + 16 floats puts the rows g and g + 1
// of a step 16 banks apart.
// The column sums' workgroups (u): thread (q, col) = (tid / 64, tid % 64) adds the rows q, q + 4, ... of its split in ascending order,
// the four q in a fixed tree.
constexpr int kGradLa = kCinMaxMaps + 16;

__host__ __device__ inline int cin_ti(int Fp) { return Fp == 16 ? 4 : (Fp == 32 ? 2 : 1); }

__global__ __launch_bounds__(kBlock) void k_cin_wgrad(CinArgs a) {
    __shared__ __attribute__((aligned(16))) float A[kCinGradStage * kGradLa], XP[kCinGradStage * 4], XZ[kCinGradStage * 64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, c = lane & 15;
    const int Fp = a.Fp, k = a.k, TI = cin_ti(Fp), NTc = TI * Fp / 16, SH = cin_hsum(a);
    const int row_lo = blockIdx.y * kCinGradRows, row_hi = min(a.b.rows, row_lo + kCinGradRows);
    const int64_t m_lo = (int64_t)row_lo * k, m_hi = (int64_t)row_hi * k;
    float *part = a.gpart + (int64_t)blockIdx.y * a.total;
    int rem = blockIdx.x;
    for (int l = 1; l <= a.L; ++l) {
        const int hp = cin_hp(a, l), tiles = hp / TI;
        if (rem >= tiles) {
            rem -= tiles;
            continue;
        }
        const int i0 = rem * TI, H = a.H[l], ldp = l == 1 ? Fp : a.H[l - 1];
        const float *gwl = a.gw[l - 1], *xp = a.xw[l - 1], *x0 = a.xw[0];
        const bool one = wave < H / 16, two = wave + 4 < H / 16;
        f32x4 acc[2][4];
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i >> 2][i & 3] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int64_t k0 = m_lo; k0 < m_hi; k0 += kCinGradStage) {
            __syncthreads();                 // the previous stage has been read
            for (int i = tid; i < kCinGradStage * (H / 4); i += kBlock) {
                const int rr = i / (H / 4), c4 = i - rr * (H / 4);
                const int64_t m = k0 + rr;
                float4 v = f4zero();
                if (m < m_hi) v = f4mul(*reinterpret_cast<const float4 *>(gwl + m * H + 4 * c4), a.b.e[m / k]);
                *reinterpret_cast<float4 *>(A + rr * kGradLa + 4 * c4) = v;
            }
            for (int i = tid; i < kCinGradStage * Fp; i += kBlock) {
                const int rr = i / Fp, pos = i - rr * Fp;
                const int64_t m = k0 + rr;
                const int j = (pos & ~15) + 4 * (pos & 3) + ((pos >> 2) & 3);
                XZ[rr * 64 + pos] = m < m_hi ? x0[m * Fp + j] : 0.f;
            }
            if (tid < kCinGradStage * TI) {
                const int rr = tid / TI, q = tid - rr * TI;
                const int64_t m = k0 + rr;
                XP[rr * 4 + q] = m < m_hi ? xp[m * ldp + i0 + q] : 0.f;
            }
            __syncthreads();
            if (one) {
#pragma unroll
                for (int kk = 0; kk < kCinGradStage; kk += 4) {
                    const int rr = kk + g;
                    const float a0 = A[rr * kGradLa + 16 * wave + c], a1 = two ? A[rr * kGradLa + 16 * (wave + 4) + c] : 0.f;
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct) {
                        if (ct >= NTc) break;          // (the same for every thread)
                        const int col = 16 * ct + c;
                        const float bv = XP[rr * 4 + col / Fp] * XZ[rr * 64 + col % Fp];
                        acc[0][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, bv, acc[0][ct], 0, 0, 0);
                        if (two) acc[1][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, bv, acc[1][ct], 0, 0, 0);
                    }
                }
            }
        }
        float *out = part + a.woff[l - 1];
#pragma unroll
        for (int hq = 0; hq < 2; ++hq)
#pragma unroll
            for (int ct = 0; ct < 4; ++ct)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int h = 16 * (wave + 4 * hq) + 4 * g + r, col = 16 * ct + c;
                    if (h < H && ct < NTc) out[((int64_t)h * hp + i0 + col / Fp) * Fp + col % Fp] = acc[hq][ct][r];
                }
        return;
    }
    // u's column sums of e p
    const int q = tid >> 6, col = rem * 64 + (tid & 63);
    float t = 0.f;
    if (col < SH)
        for (int row = row_lo + q; row < row_hi; row += 4) t = fmaf(a.b.e[row], a.pw[(int64_t)row * SH + col], t);
    A[tid] = t;
    __syncthreads();
    if (q == 0 && col < SH) part[a.uoff + col] = (A[tid] + A[64 + tid]) + (A[128 + tid] + A[192 + tid]);
}

// A thread per dense parameter: its partials — split s into accumulator s % 8 in split order, the eight in a fixed tree: eight loads
// in flight — then the step on g / |B| + regd theta.
template <bool ADAGRAD>
__global__ __launch_bounds__(kBlock) void k_cin_dupdate(CinArgs a) {
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

int wgrad_blocks(const CinArgs &a) {
    int n = (cin_hsum(a) + 63) / 64;
    for (int l = 1; l <= a.L; ++l) n += cin_hp(a, l) / cin_ti(a.Fp);
    return n;
}

template <int MTW>
hipError_t forward_instance(const CinArgs &a, bool train, hipStream_t s) {
    const size_t lds = cin_forward_lds(a.rt, a.k, a.Fp, a.L, a.H, train);
    if (lds + cin_forward_static() > 65536) {          // above the default: up to what the device gives a workgroup
        const void *fn = train ? reinterpret_cast<const void *>(&k_cin_forward<MTW, true>) : reinterpret_cast<const void *>(&k_cin_forward<MTW, false>);
        const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    dim3 g((unsigned)cin_forward_blocks(a.b.rows)), b(kCinBlock);
    if (train) hipLaunchKernelGGL((k_cin_forward<MTW, true>), g, b, lds, s, a);
    else hipLaunchKernelGGL((k_cin_forward<MTW, false>), g, b, lds, s, a);
    return hipGetLastError();
}

bool shape_ok(const CinArgs &a) {
    if (a.L < 1 || a.L > kCinMaxLayers || a.k < 1 || a.k > kCinMaxFactors || a.k > a.b.Kp || a.Fp != cin_round16(a.b.F) || a.Fp > 64) return false;
    int at = 0;
    for (int l = 1; l <= a.L; ++l) {
        if (a.H[l] < 16 || a.H[l] > kCinMaxMaps || a.H[l] % 16 || a.woff[l - 1] != at) return false;
        at += a.H[l] * cin_hp(a, l) * a.Fp;
    }
    return a.uoff == at && a.total > at;
}

}  // namespace

hipError_t launch_cin_forward(const CinArgs &a0, bool train, hipStream_t s) {
    const FwfmArgs &b = a0.b;
    if (b.rows <= 0) return hipSuccess;
    if (!b.V || !b.w || !b.w0 || !a0.D || !b.row_ptr || !b.yhat || b.F < 1 || (b.Kp != 4 && b.Kp != 8 && b.Kp != 16) || !shape_ok(a0))
        return hipErrorInvalidValue;
    if (train) {
        if (!b.y || !b.e || !b.bsum || !b.dz || (a0.train_d && !a0.pw)) return hipErrorInvalidValue;
        for (int l = 0; l < a0.L; ++l)
            if (a0.train_d && (!a0.xw[l] || !a0.gw[l])) return hipErrorInvalidValue;
    }
    CinArgs a = a0;
    a.rt = cin_row_tile(a.k, a.Fp, a.L, a.H, train, a.lds_limit);
    if (a.rt == 0) return hipErrorInvalidValue;          // not even one row fits the device's LDS
    return cin_round16(a.rt * a.k) / 16 >= 2 * kCinWaves ? forward_instance<2>(a, train, s) : forward_instance<1>(a, train, s);
}

hipError_t launch_cin_wgrad(const CinArgs &a, hipStream_t s) {
    if (a.b.rows <= 0) return hipSuccess;
    if (!a.gpart || !a.b.e || !a.pw || a.n_splits != cin_grad_splits(a.b.rows) || !shape_ok(a)) return hipErrorInvalidValue;
    for (int l = 0; l < a.L; ++l)
        if (!a.xw[l] || !a.gw[l]) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_cin_wgrad, dim3((unsigned)wgrad_blocks(a), (unsigned)a.n_splits), dim3(kBlock), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_cin_dupdate(const CinArgs &a, bool adagrad, hipStream_t s) {
    if (a.b.rows <= 0) return hipSuccess;
    if (!a.D || !a.gpart || (adagrad && !a.ND) || a.total < 1) return hipErrorInvalidValue;
    dim3 g((unsigned)((a.total + kBlock - 1) / kBlock)), b(kBlock);
    if (adagrad) hipLaunchKernelGGL(k_cin_dupdate<true>, g, b, 0, s, a);
    else hipLaunchKernelGGL(k_cin_dupdate<false>, g, b, 0, s, a);
    return hipGetLastError();
}

}  // namespace fmhip
