// fm_dcn.hip — the kernels of the low-rank cross network, DCN-V2 (include/fmhip_dcn.h; DESIGN.md, "DCN-V2"): gfx950, wave64.
//   k_dcn_forward  a workgroup owns kDcnRowsPerBlock rows and walks them in tiles of RT rows.  Three LDS tiles stay resident for a
//                  tile of rows: X0[RT][Pp] (the field sums x_0, never overwritten), X[RT][Pp] (the state x_l, then the running
//                  gradient g_l, both updated in place) and Tt[RT][r] (the bottleneck t_l, then m_l).  Per layer two products on
//                  the exact-f32 MFMA: t_l = X VT_l^T into Tt, then Tt UT_l^T, whose epilogue forms x_0 o (. + c_l) + x_l at the
//                  accumulator's own element of X.  A training launch goes on backwards over the same tiles: X = u broadcast,
//                  m_l = (X o X0) UT_l (the A operand is formed in registers) into Tt, then X += Tt VT_l, whose epilogue also
//                  carries J's second sum; at the end X holds J and a lane group per entry writes x_a J[f_a] to the workspace dz.
//                  Also the scorer
//   k_dcn_wgrad    a list of products sum_r e_r A_r^T B_r over the stored q_l, t_l, m_l, x_l: a workgroup per (64 x 64 output tile,
//                  split of kDcnGradRows rows) stages both operands through LDS and leaves one partial per split; behind the
//                  tiles' workgroups come those of the column sums sum_r e_r q_l (c_l) and sum_r e_r x_L (u)
//   k_dcn_dupdate  a thread per dense parameter: the splits' partials in split order, then the step
// v, w, w0 and the statistics: fm_fwfm.hip's backward and update launches over this forward's dz, e and bsum.
// No atomics: one writer per element, every sum in an order fixed by the data and by the constants of fm_dcn.h — never by the CU count.
#include "fm_device.h"
#include "fm_finish.h"      // pair_sigma_residual
#include "fm_dcn.h"

namespace fmhip {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// MFMA lane roles (v_mfma_f32_16x16x4_f32): lane (g, c) = (lane / 16, lane % 16) supplies A[c][g] and B[g][c] of a step and holds
// D[4g + i][c] in acc[i].
//
// OUT[RT][N] = A[RT][K] . B[K][N]: wave w takes the N tiles w, w + 4, ... and every row tile of them, so a fragment of B it loads is
// used MT times.  A 16-wide slice u of the reduction is four MFMA steps; step j takes k = 16u + 4g + j from lane group g — the same
// permutation on both operands — so that A is one ds_read_b128 of A[row c][16u + 4g ..].
//   MUL        the A operand is A o A2, the product of the two tiles' ds_read_b128 (q_l = g_{l+1} o x_0: no q tile exists in LDS)
//   BT = true  (the forward half): B[k][n] = W[n][k], W row-major [N][K]: one global_load_dwordx4 of W[16 nt + c][16u + 4g ..]
//   BT = false (the backward half, the same arrays): B[k][n] = W[k][n], W row-major [K][N]: four global_load_dword of
//              W[16u + 4g + j][16 nt + c], each 16 consecutive floats per lane group
// epi(nt, acc) is handed the finished N tile: the lane holds OUT[16 mt + 4g + i][16 nt + c] in acc[mt][i].  The N tiles a wave takes,
// and so the elements (row, n) a lane is handed, depend on N alone: every product of width Pp hands a lane the same elements of X.
template <int MT, bool BT, bool MUL, typename Epi>
__device__ __forceinline__ void dcn_product(const float *A, const float *A2, int lda, const float *__restrict__ W, int K, int N, int wave, int g, int c, Epi epi) {
    const float4 *arow = reinterpret_cast<const float4 *>(A + c * lda) + g;
    const float4 *brow = reinterpret_cast<const float4 *>(A2 + c * lda) + g;
    for (int nt = wave; nt < N / 16; nt += kBlock / 64) {
        f32x4 acc[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int u = 0; u < K / 16; ++u) {
            float4 bv;
            if (BT) {
                bv = reinterpret_cast<const float4 *>(W + (int64_t)(nt * 16 + c) * K)[4 * u + g];
            } else {
                const float *p = W + (int64_t)(16 * u + 4 * g) * N + nt * 16 + c;
                bv = make_float4(p[0], p[N], p[2 * N], p[3 * N]);
            }
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                float4 av = arow[mt * 4 * lda + 4 * u];
                if (MUL) {
                    const float4 a2 = brow[mt * 4 * lda + 4 * u];
                    av = make_float4(av.x * a2.x, av.y * a2.y, av.z * a2.z, av.w * a2.w);
                }
                acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, bv.x, acc[mt], 0, 0, 0);
                acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, bv.y, acc[mt], 0, 0, 0);
                acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, bv.z, acc[mt], 0, 0, 0);
                acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, bv.w, acc[mt], 0, 0, 0);
            }
        }
        epi(nt, acc);
    }
}

template <int KP, int MT, bool TRAIN>
__global__ __launch_bounds__(kBlock) void k_dcn_forward(DcnArgs a) {
    constexpr int Q = KP / 4, RT = 16 * MT;
    static_assert(RT <= 64 && kDcnRowsPerBlock % RT == 0, "the row tile");
    extern __shared__ float4 dcn_lds[];
    __shared__ double sh[RT][3];
    const FwfmArgs &b = a.b;
    const int Pp = a.Pp, L = a.L, R = a.r;
    const int LP = Pp + kDcnPad, LR = R + kDcnPad;
    float *X0 = reinterpret_cast<float *>(dcn_lds);          // [RT][LP]: x_0 = the field sums
    float *X = X0 + RT * LP;                                 // [RT][LP]: x_l, then g_l, then J
    float *Tt = X + RT * LP;                                 // [RT][LR]: t_l, then m_l
    float *rlin = Tt + RT * LR, *rcross = rlin + RT;         // [RT] each
    int *rp = reinterpret_cast<int *>(rcross + RT);          // [RT + 1] the rows' entry offsets from the tile's first entry
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, c = lane & 15;
    const float4 *V4 = reinterpret_cast<const float4 *>(b.V);
    const float w0 = *b.w0;
    const float *uvec = a.D + a.hoff;
    const bool store = TRAIN && a.train_d;
    double se = 0.0, sse = 0.0, nf = 0.0;    // thread j < RT: the rows j of every tile

    const int64_t row_lo = (int64_t)blockIdx.x * kDcnRowsPerBlock;
    for (int t0 = 0; t0 < kDcnRowsPerBlock; t0 += RT) {
        const int64_t r0 = row_lo + t0;
        if (r0 >= b.rows) break;             // (the same for every thread)
        const int nr = (int)min((int64_t)RT, b.rows - r0);
        const int64_t E0 = b.row_ptr[r0];
        __syncthreads();                     // the previous tile has been read
        for (int i = tid; i < RT * LP / 4; i += kBlock) reinterpret_cast<float4 *>(X0)[i] = f4zero();
        if (tid <= nr) rp[tid] = (int)(b.row_ptr[r0 + tid] - E0);
        __syncthreads();
        const int neQ = rp[nr] * Q;
        // the field sums: a lane group per entry, the head of a same-field run sums its run in ascending order
        for (int it = tid; it < neQ; it += kBlock) {
            const int p = it / Q, q = it % Q;
            const int rb = b.run[E0 + p];
            if (rb == 0) continue;
            int j = 0;                       // the entry's row: the last j with rp[j] <= p
            for (int step = RT / 2; step >= 1; step >>= 1)
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
            *reinterpret_cast<float4 *>(X0 + j * LP + (int)b.fld[E0 + p] * KP + 4 * q) = s;
        }
        __syncthreads();
        // x_0 is the first state; with the dense part trained it also goes to the workspace
        for (int i = tid; i < RT * LP / 4; i += kBlock) reinterpret_cast<float4 *>(X)[i] = reinterpret_cast<const float4 *>(X0)[i];
        if (store) {
            float4 *out = reinterpret_cast<float4 *>(a.sw) + r0 * (Pp / 4);
            for (int i = tid; i < nr * (Pp / 4); i += kBlock) {
                const int j = i / (Pp / 4), c4 = i - j * (Pp / 4);
                out[i] = reinterpret_cast<const float4 *>(X0 + j * LP)[c4];
            }
        }
        // the linear term: a wave per row, a lane per entry, a fixed tree
        for (int j = wave; j < nr; j += kBlock / 64) {
            const int e0 = rp[j], n = rp[j + 1] - e0;
            float lin = 0.f;
            if (lane < n) lin = __fmul_rn(b.w[b.col[E0 + e0 + lane]], b.val[E0 + e0 + lane]);
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) lin += __shfl_xor(lin, m, 64);
            if (lane == 0) rlin[j] = lin;
        }
        __syncthreads();
        // the layers, X in place: t_l = x_l V_l into Tt, then x_{l+1} = x_0 o (t_l U_l + c_l) + x_l at the accumulator's own element
        for (int l = 0; l < L; ++l) {
            const float *cl = a.D + a.coff[l];
            float *tw = a.tw[l], *pw = a.pw[l], *xw = a.xw[l];
            dcn_product<MT, true, false>(X, X, LP, a.D + a.voff[l], Pp, R, wave, g, c, [&](int nt, const f32x4 *acc) {
                const int n = nt * 16 + c;
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int j = mt * 16 + 4 * g + i;
                        Tt[j * LR + n] = acc[mt][i];
                        if (store && j < nr) tw[(r0 + j) * R + n] = acc[mt][i];
                    }
            });
            __syncthreads();                 // Tt is whole, and no wave reads X as an A operand any more
            dcn_product<MT, true, false>(Tt, Tt, LR, a.D + a.uoff[l], R, Pp, wave, g, c, [&](int nt, const f32x4 *acc) {
                const int n = nt * 16 + c;
                const float cn = cl[n];
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int j = mt * 16 + 4 * g + i;
                        const float p = acc[mt][i] + cn;
                        const float x = fmaf(X0[j * LP + n], p, X[j * LP + n]);
                        X[j * LP + n] = x;
                        if (TRAIN && j < nr) pw[(r0 + j) * Pp + n] = p;
                        if (store && j < nr) xw[(r0 + j) * Pp + n] = x;
                    }
            });
            __syncthreads();
        }
        // the cross term <x_L, u>: a wave per row, lane i the slots i, i + 64, ..., a fixed tree
        for (int j = wave; j < nr; j += kBlock / 64) {
            float t = 0.f;
            for (int i = lane; i < Pp; i += 64) t = fmaf(X[j * LP + i], uvec[i], t);
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
        // backwards, d yhat / d . per row: g_L = u in x_L's place
        for (int idx = tid; idx < RT * Pp; idx += kBlock) {
            const int j = idx / Pp, i = idx - j * Pp;
            X[j * LP + i] = uvec[i];
        }
        __syncthreads();
        for (int l = L - 1; l >= 0; --l) {
            float *mw = a.mw[l], *jw = a.jw;
            const float *pw = a.pw[l];
            if (store) {                     // q_l = g_{l+1} o x_0 for the weight gradients
                float4 *out = reinterpret_cast<float4 *>(a.qw[l]) + r0 * (Pp / 4);
                for (int i = tid; i < nr * (Pp / 4); i += kBlock) {
                    const int j = i / (Pp / 4), c4 = i - j * (Pp / 4);
                    const float4 gv = reinterpret_cast<const float4 *>(X + j * LP)[c4], xv = reinterpret_cast<const float4 *>(X0 + j * LP)[c4];
                    out[i] = make_float4(gv.x * xv.x, gv.y * xv.y, gv.z * xv.z, gv.w * xv.w);
                }
            }
            // m_l = q_l U_l^T into Tt, q_l formed in registers
            dcn_product<MT, false, true>(X, X0, LP, a.D + a.uoff[l], Pp, R, wave, g, c, [&](int nt, const f32x4 *acc) {
                const int n = nt * 16 + c;
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int j = mt * 16 + 4 * g + i;
                        Tt[j * LR + n] = acc[mt][i];
                        if (store && j < nr) mw[(r0 + j) * R + n] = acc[mt][i];
                    }
            });
            __syncthreads();
            // g_l = m_l V_l^T + g_{l+1} in place; J's second sum sum_l g_{l+1} o p_l rides in the epilogue: p_l is this lane's own
            // store of the forward half, the running sum this lane's own store of the layer above, and layer 0 adds it into X
            dcn_product<MT, false, false>(Tt, Tt, LR, a.D + a.voff[l], R, Pp, wave, g, c, [&](int nt, const f32x4 *acc) {
                const int n = nt * 16 + c;
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int j = mt * 16 + 4 * g + i;
                        const float gu = X[j * LP + n];
                        float s2 = 0.f;
                        if (j < nr) {
                            const int64_t at = (r0 + j) * Pp + n;
                            s2 = gu * pw[at];
                            if (l < L - 1) s2 += jw[at];
                            if (l > 0) jw[at] = s2;
                        }
                        X[j * LP + n] = l > 0 ? acc[mt][i] + gu : (acc[mt][i] + gu) + s2;
                    }
            });
            __syncthreads();
        }
        // per entry x_a J[f_a]: a lane group per entry
        for (int it = tid; it < neQ; it += kBlock) {
            const int p = it / Q, q = it % Q;
            int j = 0;
            for (int step = RT / 2; step >= 1; step >>= 1)
                if (j + step < nr && rp[j + step] <= p) j += step;
            const float4 jf = *reinterpret_cast<const float4 *>(X + j * LP + (int)b.fld[E0 + p] * KP + 4 * q);
            reinterpret_cast<float4 *>(b.dz)[(E0 + p - b.nnz0) * Q + q] = f4mul(jf, b.val[E0 + p]);
        }
    }
    if (TRAIN) {
        __syncthreads();                     // (sh is the kernel's own: nothing above touches it)
        if (tid < RT) {
            sh[tid][0] = se;
            sh[tid][1] = sse;
            sh[tid][2] = nf;
        }
        __syncthreads();
        if (tid < 3) {
            double t = sh[0][tid];
            for (int j = 1; j < RT; ++j) t += sh[j][tid];
            b.bsum[(int64_t)blockIdx.x * 4 + tid] = t;
        }
        if (tid == 3) b.bsum[(int64_t)blockIdx.x * 4 + 3] = 0.0;
    }
}

// The weight gradients on the same MFMA, the reduction over the rows.  Job 2l is UT_l's: A = q_l [rows][Pp], B = t_l [rows][r], the
// Pp x r sum_r e_r q_r^T t_r; job 2l + 1 is VT_l's: A = m_l [rows][r], B = x_l [rows][Pp] (x_0 = sw), r x Pp.  A stage is
// kDcnGradStage rows of both operands in LDS, the A side scaled by e on the way in; wave w owns the 32 x 32 corner (w / 2, w % 2) of
// the 64 x 64 tile as 2 x 2 MFMA tiles: two A and two B reads per four MFMAs.  The LDS pitch of 80 floats puts the four rows g of a
// step 16 banks apart.
// The column sums' workgroups: thread (q, col) = (tid / 64, tid % 64) adds the rows q, q + 4, ... of its split in ascending order, the
// four q in a fixed tree.
constexpr int kGradLd = kDcnGradTile + 16;

__host__ __device__ inline int dcn_tiles(int m, int n) { return (m + kDcnGradTile - 1) / kDcnGradTile * ((n + kDcnGradTile - 1) / kDcnGradTile); }

__global__ __launch_bounds__(kBlock) void k_dcn_wgrad(DcnArgs a) {
    __shared__ __attribute__((aligned(16))) float A[kDcnGradStage * kGradLd], B[kDcnGradStage * kGradLd];
    constexpr int TL = kDcnGradTile;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, c = lane & 15;
    const int row_lo = blockIdx.y * kDcnGradRows, row_hi = min(a.b.rows, row_lo + kDcnGradRows);
    float *part = a.gpart + (int64_t)blockIdx.y * a.total;
    int rem = blockIdx.x;
    for (int job = 0; job < 2 * a.L; ++job) {
        const int l = job >> 1, isv = job & 1;
        const int M = isv ? a.r : a.Pp, N = isv ? a.Pp : a.r, tn = (N + TL - 1) / TL, tiles = dcn_tiles(M, N);
        if (rem >= tiles) {
            rem -= tiles;
            continue;
        }
        const int ti = rem / tn, tj = rem - ti * tn;
        const float *ha = isv ? a.mw[l] : a.qw[l], *hb = isv ? (l == 0 ? a.sw : a.xw[l - 1]) : a.tw[l];
        const int m0 = 32 * (wave >> 1), n0 = 32 * (wave & 1);
        f32x4 acc[2][2];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i >> 1][i & 1] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int k0 = row_lo; k0 < row_hi; k0 += kDcnGradStage) {
            __syncthreads();                 // the previous stage has been read
            for (int i = tid; i < 2 * kDcnGradStage * (TL / 4); i += kBlock) {
                const int side = i / (kDcnGradStage * (TL / 4)), rr = i / (TL / 4) % kDcnGradStage, c4 = i % (TL / 4);
                const int row = k0 + rr, col = (side ? tj : ti) * TL + 4 * c4;
                float4 v = f4zero();
                if (row < row_hi && col < (side ? N : M)) {
                    v = *reinterpret_cast<const float4 *>((side ? hb : ha) + (int64_t)row * (side ? N : M) + col);
                    if (!side) v = f4mul(v, a.b.e[row]);
                }
                *reinterpret_cast<float4 *>((side ? B : A) + rr * kGradLd + 4 * c4) = v;
            }
            __syncthreads();
#pragma unroll
            for (int kk = 0; kk < kDcnGradStage; kk += 4) {
                const float *pa = A + (kk + g) * kGradLd + m0 + c, *pb = B + (kk + g) * kGradLd + n0 + c;
                const float a0 = pa[0], a1 = pa[16], b0 = pb[0], b1 = pb[16];
                acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
            }
        }
        float *out = part + (isv ? a.voff[l] : a.uoff[l]);
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int nj = 0; nj < 2; ++nj)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int p = ti * TL + m0 + 16 * mi + 4 * g + i, q = tj * TL + n0 + 16 * nj + c;
                    if (p < M && q < N) out[(int64_t)p * N + q] = acc[mi][nj][i];
                }
        return;
    }
    // the column sums: of e q_l for c_l, l = 0 .. L - 1, then of e x_L for u
    const int N = a.Pp, tn = (N + TL - 1) / TL;
    const int l = rem / tn;
    if (l > a.L) return;
    const float *x = l < a.L ? a.qw[l] : a.xw[a.L - 1];
    const int q = tid >> 6, col = (rem - l * tn) * TL + (tid & 63);
    float t = 0.f;
    if (col < N)
        for (int row = row_lo + q; row < row_hi; row += 4) t = fmaf(a.b.e[row], x[(int64_t)row * N + col], t);
    A[tid] = t;
    __syncthreads();
    if (q == 0 && col < N) part[(l < a.L ? a.coff[l] : a.hoff) + col] = (A[tid] + A[64 + tid]) + (A[128 + tid] + A[192 + tid]);
}

// A thread per dense parameter: its partials — split s into accumulator s % 8 in split order, the eight in a fixed tree: eight loads
// in flight — then the step on g / |B| + regd theta (c_l: on g / |B|).
template <bool ADAGRAD>
__global__ __launch_bounds__(kBlock) void k_dcn_dupdate(DcnArgs a) {
    const int idx = blockIdx.x * kBlock + threadIdx.x;
    if (idx >= a.total) return;
    const float *src = a.gpart + idx;
    float s8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < a.n_splits; s += 8)
#pragma unroll
        for (int j = 0; j < 8; ++j) s8[j] += s + j < a.n_splits ? src[(int64_t)(s + j) * a.total] : 0.f;
    const float sum = ((s8[0] + s8[1]) + (s8[2] + s8[3])) + ((s8[4] + s8[5]) + (s8[6] + s8[7]));
    float th = a.D[idx];
    const float gh = fmaf(idx < a.coff[0] ? a.regd : 0.f, th, sum * a.b.invb);
    if (ADAGRAD) {
        float n = a.ND[idx];
        adagrad_step(th, n, gh, a.b.eta, a.b.eps);
        a.ND[idx] = n;
    } else {
        th = th - a.b.eta * gh;
    }
    a.D[idx] = th;
}

int wgrad_blocks(const DcnArgs &a) { return a.L * (dcn_tiles(a.Pp, a.r) + dcn_tiles(a.r, a.Pp)) + (a.L + 1) * ((a.Pp + kDcnGradTile - 1) / kDcnGradTile); }

template <int KP, int MT>
hipError_t forward_instance(const DcnArgs &a, bool train, hipStream_t s) {
    const size_t lds = dcn_forward_lds(16 * MT, a.Pp, a.r);
    if (lds + dcn_forward_static(16 * MT) > 65536) {          // above the default: up to what the device gives a workgroup
        const void *fn = train ? reinterpret_cast<const void *>(&k_dcn_forward<KP, MT, true>) : reinterpret_cast<const void *>(&k_dcn_forward<KP, MT, false>);
        const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    dim3 g((unsigned)dcn_forward_blocks(a.b.rows)), b(kBlock);
    if (train) hipLaunchKernelGGL((k_dcn_forward<KP, MT, true>), g, b, lds, s, a);
    else hipLaunchKernelGGL((k_dcn_forward<KP, MT, false>), g, b, lds, s, a);
    return hipGetLastError();
}

template <int KP>
hipError_t forward_kp(const DcnArgs &a, bool train, hipStream_t s) {
    switch (dcn_row_tile(a.Pp, a.r, a.lds_limit)) {
        case 64: return forward_instance<KP, 4>(a, train, s);
        case 32: return forward_instance<KP, 2>(a, train, s);
        case 16: return forward_instance<KP, 1>(a, train, s);
        default: return hipErrorInvalidValue;          // not even 16 rows fit the device's LDS
    }
}

bool shape_ok(const DcnArgs &a) {
    return a.L >= 1 && a.L <= kDcnMaxLayers && a.Pp % 16 == 0 && a.Pp >= a.b.F * a.b.Kp && a.Pp <= kDcnMaxWidth && a.r % 16 == 0 && a.r >= 16 &&
           a.r <= kDcnMaxRank;
}

}  // namespace

hipError_t launch_dcn_forward(const DcnArgs &a, bool train, hipStream_t s) {
    const FwfmArgs &b = a.b;
    if (b.rows <= 0) return hipSuccess;
    if (!b.V || !b.w || !b.w0 || !a.D || !b.row_ptr || !b.yhat || b.F < 1 || !shape_ok(a)) return hipErrorInvalidValue;
    if (train) {
        if (!b.y || !b.e || !b.bsum || !b.dz || (a.L >= 2 && !a.jw) || (a.train_d && !a.sw)) return hipErrorInvalidValue;
        for (int l = 0; l < a.L; ++l)
            if (!a.pw[l] || (a.train_d && (!a.xw[l] || !a.qw[l] || !a.tw[l] || !a.mw[l]))) return hipErrorInvalidValue;
    }
    switch (b.Kp) {
        case 4: return forward_kp<4>(a, train, s);
        case 8: return forward_kp<8>(a, train, s);
        case 16: return forward_kp<16>(a, train, s);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_dcn_wgrad(const DcnArgs &a, hipStream_t s) {
    if (a.b.rows <= 0) return hipSuccess;
    if (!a.sw || !a.gpart || !a.b.e || a.n_splits != dcn_grad_splits(a.b.rows) || !shape_ok(a)) return hipErrorInvalidValue;
    for (int l = 0; l < a.L; ++l)
        if (!a.xw[l] || !a.qw[l] || !a.tw[l] || !a.mw[l]) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_dcn_wgrad, dim3((unsigned)wgrad_blocks(a), (unsigned)a.n_splits), dim3(kBlock), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_dcn_dupdate(const DcnArgs &a, bool adagrad, hipStream_t s) {
    if (a.b.rows <= 0) return hipSuccess;
    if (!a.D || !a.gpart || (adagrad && !a.ND) || a.total < 1) return hipErrorInvalidValue;
    dim3 g((unsigned)((a.total + kBlock - 1) / kBlock)), b(kBlock);
    if (adagrad) hipLaunchKernelGGL(k_dcn_dupdate<true>, g, b, 0, s, a);
    else hipLaunchKernelGGL(k_dcn_dupdate<false>, g, b, 0, s, a);
    return hipGetLastError();
}

}  // namespace fmhip
