// fm_deepfm.hip — DeepFM's kernels (include/fmhip_deepfm.h; DESIGN.md, "DeepFM"): gfx950, wave64.
//   k_deepfm_forward  a workgroup owns kDeepRowsPerBlock rows and walks them in tiles of RT rows.  The tile's concatenated field sums
//                     S[RT][Pp] go to LDS (the FmFM forward's run-head walk), and with them the plain FM's linear and pair terms.  The
//                     whole MLP is then carried for the tile without leaving the CU: h_l = relu(h_{l-1} W_l + b_l) on the exact-f32
//                     MFMA, h_{l-1} the A operand from one LDS tile, W_l streamed from L2 as B, h_l written to the other LDS tile.
//                     A training launch goes on backwards over the same two tiles: delta_L = u o [h_L > 0],
//                     delta_{l-1} = (delta_l W_l^T) o [h_{l-1} > 0], J = delta_1 W_1^T, and per entry x_a ((T - z_a) + J[f_a]) to the
//                     workspace dz.  It leaves h_l (the masks' source) and, when the dense part is trained, S and delta_l in the
//                     workspace.  Also the scorer
//   k_deepfm_wgrad    sum_r e_r h_{l-1,r}^T delta_{l,r}: a workgroup per (64 x 64 tile of a W_l, split of kDeepGradRows rows) stages
//                     (e h_{l-1})[rows][tile i] and delta_l[rows][tile j] through LDS and leaves one partial per split; behind the
//                     tiles' workgroups come those of the column sums sum_r e_r delta_l (b_l) and sum_r e_r h_L (u)
//   k_deepfm_dupdate  a thread per dense parameter: the splits' partials in split order, then the step
// v, w, w0 and the statistics: fm_fwfm.hip's backward and update launches over this forward's dz, e and bsum.
// No atomics: one writer per element, every sum in an order fixed by the data and by the constants of fm_deepfm.h — never by the CU count.
#include "fm_device.h"
#include "fm_finish.h"      // pair_sigma_residual
#include "fm_deepfm.h"

namespace fmhip {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// MFMA lane roles (v_mfma_f32_16x16x4_f32): lane (g, c) = (lane / 16, lane % 16) supplies A[c][g] and B[g][c] of a step and holds
// D[4g + i][c] in acc[i].
//
// OUT[RT][N] = A[RT][K] . B[K][N]: wave w takes the N tiles w, w + 4, ... and every row tile of them, so a fragment of B it loads is
// used MT times.  A 16-wide slice u of the reduction is four MFMA steps; step j takes k = 16u + 4g + j from lane group g — the same
// permutation on both operands — so that A is one ds_read_b128 of A[row c][16u + 4g ..].
//   BT = false (a layer forward): B[k][n] = W[k][n], W row-major [K][N]: four global_load_dword of W[16u + 4g + j][16 nt + c], each
//                                 16 consecutive floats per lane group
//   BT = true  (its transpose, backward): B[k][n] = W[n][k], W row-major [N][K]: one global_load_dwordx4 of W[16 nt + c][16u + 4g ..]
// epi(nt, acc) is handed the finished N tile: the lane holds OUT[16 mt + 4g + i][16 nt + c] in acc[mt][i].
template <int MT, bool BT, typename Epi>
__device__ __forceinline__ void tile_product(const float *A, int lda, const float *__restrict__ W, int K, int N, int wave, int g, int c, Epi epi) {
    const float4 *arow = reinterpret_cast<const float4 *>(A + c * lda) + g;
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
                const float4 av = arow[mt * 4 * lda + 4 * u];
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
__global__ __launch_bounds__(kBlock) void k_deepfm_forward(DeepfmArgs a) {
    constexpr int Q = KP / 4, RT = 16 * MT;
    static_assert(RT <= 64 && kDeepRowsPerBlock % RT == 0, "the row tile");
    extern __shared__ float4 deepfm_lds[];
    __shared__ double sh[RT][3];
    const FwfmArgs &b = a.b;
    const int F = b.F, Pp = a.Pp, L = a.L;
    const int LX = deepfm_max(Pp, L >= 2 ? a.n[2] : 0) + kDeepPad, LY = deepfm_max(a.n[1], L >= 3 ? a.n[3] : 0) + kDeepPad;
    float *X = reinterpret_cast<float *>(deepfm_lds);        // [RT][LX]: S = h_0, h_2, delta_2, J
    float *Y = X + RT * LX;                                  // [RT][LY]: h_1, h_3, delta_3, delta_1
    float *T = Y + RT * LY;                                  // [RT][KP]: the rows' sums over all their entries
    float *rlin = T + RT * KP, *rpair = rlin + RT, *rdeep = rpair + RT;          // [RT] each
    int *rp = reinterpret_cast<int *>(rdeep + RT);           // [RT + 1] the rows' entry offsets from the tile's first entry
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, c = lane & 15;
    const float4 *V4 = reinterpret_cast<const float4 *>(b.V);
    const float w0 = *b.w0;
    const float *uvec = a.D + a.uoff;
    double se = 0.0, sse = 0.0, nf = 0.0;    // thread j < RT: the rows j of every tile

    const int64_t row_lo = (int64_t)blockIdx.x * kDeepRowsPerBlock;
    for (int t0 = 0; t0 < kDeepRowsPerBlock; t0 += RT) {
        const int64_t r0 = row_lo + t0;
        if (r0 >= b.rows) break;             // (the same for every thread)
        const int nr = (int)min((int64_t)RT, b.rows - r0);
        const int64_t E0 = b.row_ptr[r0];
        __syncthreads();                     // the previous tile has been read
        for (int i = tid; i < RT * LX / 4; i += kBlock) reinterpret_cast<float4 *>(X)[i] = f4zero();
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
            *reinterpret_cast<float4 *>(X + j * LX + (int)b.fld[E0 + p] * KP + 4 * q) = s;
        }
        __syncthreads();
        // T = the sum of the row's field sums, field by field
        for (int i = tid; i < RT * KP; i += kBlock) {
            const int j = i / KP, d = i % KP;
            float t = 0.f;
            for (int f = 0; f < F; ++f) t += X[j * LX + f * KP + d];
            T[i] = t;
        }
        if (TRAIN && a.train_d) {
            float4 *out = reinterpret_cast<float4 *>(a.sw) + r0 * (Pp / 4);
            for (int i = tid; i < nr * (Pp / 4); i += kBlock) {
                const int j = i / (Pp / 4), c4 = i - j * (Pp / 4);
                out[i] = reinterpret_cast<const float4 *>(X + j * LX)[c4];
            }
        }
        __syncthreads();
        // the plain FM's terms: a wave per row, a lane per entry, fixed trees.  The pair term as 1/2 sum_a <z_a, T - z_a>, the products
        // and differences the rounded ones (no contraction): a row of one entry has T - z_a == 0 exactly.
        for (int j = wave; j < nr; j += kBlock / 64) {
            const int e0 = rp[j], n = rp[j + 1] - e0;
            float lin = 0.f, pr = 0.f;
            if (lane < n) {
                const float x = b.val[E0 + e0 + lane];
                const int64_t i = b.col[E0 + e0 + lane];
                lin = __fmul_rn(b.w[i], x);
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    const float4 v = V4[i * Q + q], t = *reinterpret_cast<const float4 *>(T + j * KP + 4 * q);
                    const float4 z = make_float4(__fmul_rn(x, v.x), __fmul_rn(x, v.y), __fmul_rn(x, v.z), __fmul_rn(x, v.w));
                    const float4 o = make_float4(__fsub_rn(t.x, z.x), __fsub_rn(t.y, z.y), __fsub_rn(t.z, z.z), __fsub_rn(t.w, z.w));
                    pr += f4dot(z, o);
                }
            }
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                lin += __shfl_xor(lin, m, 64);
                pr += __shfl_xor(pr, m, 64);
            }
            if (lane == 0) {
                rlin[j] = lin;
                rpair[j] = 0.5f * pr;
            }
        }
        // the layers: h_l = relu(h_{l-1} W_l + b_l), X -> Y -> X -> Y
        for (int l = 1; l <= L; ++l) {
            const float *in = (l & 1) ? X : Y;
            float *out = (l & 1) ? Y : X;
            const int ldi = (l & 1) ? LX : LY, ldo = (l & 1) ? LY : LX, N = a.n[l];
            const float *bias = a.D + a.boff[l - 1];
            float *hw = a.hw[l - 1] + r0 * N;
            tile_product<MT, false>(in, ldi, a.D + a.woff[l - 1], a.n[l - 1], N, wave, g, c, [&](int nt, const f32x4 *acc) {
                const int n = nt * 16 + c;
                const float bn = bias[n];
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int j = mt * 16 + 4 * g + i;
                        const float h = fmaxf(acc[mt][i] + bn, 0.f);
                        out[j * ldo + n] = h;
                        if (TRAIN && j < nr) hw[(int64_t)j * N + n] = h;
                    }
            });
            __syncthreads();
        }
        // y_deep = <h_L, u>: a wave per row, lane i the units i, i + 64, ..., a fixed tree
        {
            const float *hl = (L & 1) ? Y : X;
            const int ld = (L & 1) ? LY : LX, N = a.n[L];
            for (int j = wave; j < nr; j += kBlock / 64) {
                float t = 0.f;
                for (int i = lane; i < N; i += 64) t = fmaf(hl[j * ld + i], uvec[i], t);
#pragma unroll
                for (int m = 32; m >= 1; m >>= 1) t += __shfl_xor(t, m, 64);
                if (lane == 0) rdeep[j] = t;
            }
        }
        __syncthreads();
        if (tid < nr) {
            const float yh = ((w0 + rlin[tid]) + rpair[tid]) + rdeep[tid];
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
        // backwards, d yhat / d . per row: delta_L = u o [h_L > 0] in h_L's place
        {
            float *hl = (L & 1) ? Y : X;
            const int ld = (L & 1) ? LY : LX, N = a.n[L];
            float *dw = a.dw[L - 1] + r0 * N;
            for (int idx = tid; idx < RT * N; idx += kBlock) {
                const int j = idx / N, i = idx - j * N;
                const float d = hl[j * ld + i] > 0.f ? uvec[i] : 0.f;
                hl[j * ld + i] = d;
                if (a.train_d && j < nr) dw[idx] = d;
            }
        }
        __syncthreads();
        // delta_{l-1} = (delta_l W_l^T) o [h_{l-1} > 0], the mask from the workspace this workgroup wrote above
        for (int l = L; l >= 2; --l) {
            const float *in = (l & 1) ? Y : X;
            float *out = (l & 1) ? X : Y;
            const int ldi = (l & 1) ? LY : LX, ldo = (l & 1) ? LX : LY, N = a.n[l - 1];
            const float *hw = a.hw[l - 2] + r0 * N;
            float *dw = a.dw[l - 2] + r0 * N;
            tile_product<MT, true>(in, ldi, a.D + a.woff[l - 1], a.n[l], N, wave, g, c, [&](int nt, const f32x4 *acc) {
                const int n = nt * 16 + c;
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int j = mt * 16 + 4 * g + i;
                        const float d = (j < nr && hw[(int64_t)j * N + n] > 0.f) ? acc[mt][i] : 0.f;
                        out[j * ldo + n] = d;
                        if (a.train_d && j < nr) dw[(int64_t)j * N + n] = d;
                    }
            });
            __syncthreads();
        }
        // J = delta_1 W_1^T into X
        tile_product<MT, true>(Y, LY, a.D, a.n[1], Pp, wave, g, c, [&](int nt, const f32x4 *acc) {
            const int n = nt * 16 + c;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int i = 0; i < 4; ++i) X[(mt * 16 + 4 * g + i) * LX + n] = acc[mt][i];
        });
        __syncthreads();
        // per entry x_a D_a, D_a = (T - z_a) + J[f_a]: a lane group per entry
        for (int it = tid; it < neQ; it += kBlock) {
            const int p = it / Q, q = it % Q;
            int j = 0;
            for (int step = RT / 2; step >= 1; step >>= 1)
                if (j + step < nr && rp[j + step] <= p) j += step;
            const float x = b.val[E0 + p];
            const float4 v = V4[(int64_t)b.col[E0 + p] * Q + q];
            const float4 t = *reinterpret_cast<const float4 *>(T + j * KP + 4 * q);
            const float4 jf = *reinterpret_cast<const float4 *>(X + j * LX + (int)b.fld[E0 + p] * KP + 4 * q);
            const float4 D = make_float4(__fsub_rn(t.x, __fmul_rn(x, v.x)) + jf.x, __fsub_rn(t.y, __fmul_rn(x, v.y)) + jf.y,
                                         __fsub_rn(t.z, __fmul_rn(x, v.z)) + jf.z, __fsub_rn(t.w, __fmul_rn(x, v.w)) + jf.w);
            reinterpret_cast<float4 *>(b.dz)[(E0 + p - b.nnz0) * Q + q] = f4mul(D, x);
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

// A W_l's gradient on the same MFMA, the reduction over the rows: M = 64 of the layer's inputs (tile ti), N = 64 of its units (tile
// tj).  A stage is kDeepGradStage rows of both operands in LDS, the A side (h_{l-1}; the field sums for l = 1) scaled by e on the way
// in; wave w owns the 32 x 32 corner (w / 2, w % 2) of the tile as 2 x 2 MFMA tiles: two A and two B reads per four MFMAs.  The LDS
// pitch of 80 floats puts the four rows g of a step 16 banks apart.
// The column sums' workgroups: thread (q, col) = (tid / 64, tid % 64) adds the rows q, q + 4, ... of its split in ascending order, the
// four q in a fixed tree.
constexpr int kGradLd = kDeepGradTile + 16;

__global__ __launch_bounds__(kBlock) void k_deepfm_wgrad(DeepfmArgs a) {
    __shared__ __attribute__((aligned(16))) float A[kDeepGradStage * kGradLd], B[kDeepGradStage * kGradLd];
    constexpr int TL = kDeepGradTile;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, c = lane & 15;
    const int row_lo = blockIdx.y * kDeepGradRows, row_hi = min(a.b.rows, row_lo + kDeepGradRows);
    float *part = a.gpart + (int64_t)blockIdx.y * a.total;
    int rem = blockIdx.x;
    for (int l = 1; l <= a.L; ++l) {
        const int K = a.n[l - 1], N = a.n[l], tn = (N + TL - 1) / TL, tiles = (K + TL - 1) / TL * tn;
        if (rem >= tiles) {
            rem -= tiles;
            continue;
        }
        const int ti = rem / tn, tj = rem - ti * tn;
        const float *ha = l == 1 ? a.sw : a.hw[l - 2], *db = a.dw[l - 1];
        const int m0 = 32 * (wave >> 1), n0 = 32 * (wave & 1);
        f32x4 acc[2][2];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i >> 1][i & 1] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int k0 = row_lo; k0 < row_hi; k0 += kDeepGradStage) {
            __syncthreads();                 // the previous stage has been read
            for (int i = tid; i < 2 * kDeepGradStage * (TL / 4); i += kBlock) {
                const int side = i / (kDeepGradStage * (TL / 4)), rr = i / (TL / 4) % kDeepGradStage, c4 = i % (TL / 4);
                const int row = k0 + rr, col = (side ? tj : ti) * TL + 4 * c4;
                float4 v = f4zero();
                if (row < row_hi && col < (side ? N : K)) {
                    v = *reinterpret_cast<const float4 *>((side ? db : ha) + (int64_t)row * (side ? N : K) + col);
                    if (!side) v = f4mul(v, a.b.e[row]);
                }
                *reinterpret_cast<float4 *>((side ? B : A) + rr * kGradLd + 4 * c4) = v;
            }
            __syncthreads();
#pragma unroll
            for (int kk = 0; kk < kDeepGradStage; kk += 4) {
                const float *pa = A + (kk + g) * kGradLd + m0 + c, *pb = B + (kk + g) * kGradLd + n0 + c;
                const float a0 = pa[0], a1 = pa[16], b0 = pb[0], b1 = pb[16];
                acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
            }
        }
        float *out = part + a.woff[l - 1];
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int nj = 0; nj < 2; ++nj)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int p = ti * TL + m0 + 16 * mi + 4 * g + i, q = tj * TL + n0 + 16 * nj + c;
                    if (p < K && q < N) out[(int64_t)p * N + q] = acc[mi][nj][i];
                }
        return;
    }
    // the column sums: of e delta_l for b_l, l = 1 .. L, then of e h_L for u
    for (int l = 1; l <= a.L + 1; ++l) {
        const int N = a.n[l <= a.L ? l : a.L], tn = (N + TL - 1) / TL;
        if (rem >= tn) {
            rem -= tn;
            continue;
        }
        const float *x = l <= a.L ? a.dw[l - 1] : a.hw[a.L - 1];
        const int q = tid >> 6, col = rem * TL + (tid & 63);
        float t = 0.f;
        if (col < N)
            for (int row = row_lo + q; row < row_hi; row += 4) t = fmaf(a.b.e[row], x[(int64_t)row * N + col], t);
        A[tid] = t;
        __syncthreads();
        if (q == 0 && col < N) part[(l <= a.L ? a.boff[l - 1] : a.uoff) + col] = (A[tid] + A[64 + tid]) + (A[128 + tid] + A[192 + tid]);
        return;
    }
}

// A thread per dense parameter: its partials — split s into accumulator s % 8 in split order, the eight in a fixed tree: eight loads
// in flight — then the step on g / |B| + regd theta (a bias: on g / |B|).
template <bool ADAGRAD>
__global__ __launch_bounds__(kBlock) void k_deepfm_dupdate(DeepfmArgs a) {
    const int idx = blockIdx.x * kBlock + threadIdx.x;
    if (idx >= a.total) return;
    const float *src = a.gpart + idx;
    float s8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < a.n_splits; s += 8)
#pragma unroll
        for (int j = 0; j < 8; ++j) s8[j] += s + j < a.n_splits ? src[(int64_t)(s + j) * a.total] : 0.f;
    const float sum = ((s8[0] + s8[1]) + (s8[2] + s8[3])) + ((s8[4] + s8[5]) + (s8[6] + s8[7]));
    float th = a.D[idx];
    const float gh = fmaf(idx < a.boff[0] ? a.regd : 0.f, th, sum * a.b.invb);
    if (ADAGRAD) {
        float n = a.ND[idx];
        adagrad_step(th, n, gh, a.b.eta, a.b.eps);
        a.ND[idx] = n;
    } else {
        th = th - a.b.eta * gh;
    }
    a.D[idx] = th;
}

int wgrad_blocks(const DeepfmArgs &a) {
    int n = 0;
    for (int l = 1; l <= a.L; ++l) {
        const int tn = (a.n[l] + kDeepGradTile - 1) / kDeepGradTile;
        n += (a.n[l - 1] + kDeepGradTile - 1) / kDeepGradTile * tn + tn;
    }
    return n + (a.n[a.L] + kDeepGradTile - 1) / kDeepGradTile;
}

template <int KP, int MT>
hipError_t forward_instance(const DeepfmArgs &a, bool train, hipStream_t s) {
    const size_t lds = deepfm_forward_lds(16 * MT, deepfm_wx(a), deepfm_wy(a), KP);
    if (lds + 16 * MT * 3 * sizeof(double) > (size_t)kDeepLdsBudget) {          // the widest models' 16-row tile: up to the device's own limit
        int dev = 0, most = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e == hipSuccess) e = hipDeviceGetAttribute(&most, hipDeviceAttributeMaxSharedMemoryPerBlock, dev);
        if (e != hipSuccess) return e;
        if (lds + 16 * MT * 3 * sizeof(double) > (size_t)most) return hipErrorInvalidValue;
        const void *fn = train ? reinterpret_cast<const void *>(&k_deepfm_forward<KP, MT, true>) : reinterpret_cast<const void *>(&k_deepfm_forward<KP, MT, false>);
        e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    dim3 g((unsigned)deepfm_forward_blocks(a.b.rows)), b(kBlock);
    if (train) hipLaunchKernelGGL((k_deepfm_forward<KP, MT, true>), g, b, lds, s, a);
    else hipLaunchKernelGGL((k_deepfm_forward<KP, MT, false>), g, b, lds, s, a);
    return hipGetLastError();
}

template <int KP>
hipError_t forward_kp(const DeepfmArgs &a, bool train, hipStream_t s) {
    switch (deepfm_row_tile(deepfm_wx(a), deepfm_wy(a), KP)) {
        case 64: return forward_instance<KP, 4>(a, train, s);
        case 32: return forward_instance<KP, 2>(a, train, s);
        default: return forward_instance<KP, 1>(a, train, s);
    }
}

bool shape_ok(const DeepfmArgs &a) {
    if (a.L < 1 || a.L > kDeepMaxLayers || a.Pp % 16 || a.Pp < a.b.F * a.b.Kp || a.Pp > kDeepMaxWidth || a.n[0] != a.Pp) return false;
    for (int l = 1; l <= a.L; ++l)
        if (a.n[l] % 16 || a.n[l] < 16 || a.n[l] > kDeepMaxUnits) return false;
    return true;
}

}  // namespace

hipError_t launch_deepfm_forward(const DeepfmArgs &a, bool train, hipStream_t s) {
    const FwfmArgs &b = a.b;
    if (b.rows <= 0) return hipSuccess;
    if (!b.V || !b.w || !b.w0 || !a.D || !b.row_ptr || !b.yhat || b.F < 1 || !shape_ok(a)) return hipErrorInvalidValue;
    if (train) {
        if (!b.y || !b.e || !b.bsum || !b.dz || (a.train_d && !a.sw)) return hipErrorInvalidValue;
        for (int l = 0; l < a.L; ++l)
            if (!a.hw[l] || (a.train_d && !a.dw[l])) return hipErrorInvalidValue;
    }
    switch (b.Kp) {
        case 4: return forward_kp<4>(a, train, s);
        case 8: return forward_kp<8>(a, train, s);
        case 16: return forward_kp<16>(a, train, s);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_deepfm_wgrad(const DeepfmArgs &a, hipStream_t s) {
    if (a.b.rows <= 0) return hipSuccess;
    if (!a.sw || !a.gpart || !a.b.e || a.n_splits != deepfm_grad_splits(a.b.rows) || !shape_ok(a)) return hipErrorInvalidValue;
    for (int l = 0; l < a.L; ++l)
        if (!a.hw[l] || !a.dw[l]) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_deepfm_wgrad, dim3((unsigned)wgrad_blocks(a), (unsigned)a.n_splits), dim3(kBlock), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_deepfm_dupdate(const DeepfmArgs &a, bool adagrad, hipStream_t s) {
    if (a.b.rows <= 0) return hipSuccess;
    if (!a.D || !a.gpart || (adagrad && !a.ND) || a.total < 1) return hipErrorInvalidValue;
    dim3 g((unsigned)((a.total + kBlock - 1) / kBlock)), b(kBlock);
    if (adagrad) hipLaunchKernelGGL(k_deepfm_dupdate<true>, g, b, 0, s, a);
    else hipLaunchKernelGGL(k_deepfm_dupdate<false>, g, b, 0, s, a);
    return hipGetLastError();
}

}  // namespace fmhip
