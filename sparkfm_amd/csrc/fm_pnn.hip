// fm_pnn.hip — the kernels of the product-based neural network (include/fmhip_pnn.h; DESIGN.md, "PNN"): gfx950, wave64.
//   k_pnn_forward  a workgroup owns kPnnRowsPerBlock rows and walks them in tiles of RT rows.  Only the tile's field sums X0[RT][Pp]
//                  are resident; h_0's pair part never exists in LDS as a whole.  The first layer's accumulators live in registers
//                  across its whole reduction: first X0 . W_1[field rows], then, Gram tile by Gram tile, a wave per row forms the
//                  row's 16 x 16 block of S S^T on the MFMA into a staging tile, and the staging tile is consumed at once against the
//                  tile's rows of W_1.  Bias and ReLU in the epilogue, the remaining layers and yhat as DeepFM's.  A training launch
//                  goes on backwards: the delta chain down to delta_1, Jt = delta_1 W_1[field rows]^T, and per Gram tile
//                  dG = delta_1 W_1[tile rows]^T into the staging tile, from which the row's owner wave adds dG S and dG^T S to Jt
//                  on the MFMA; per entry x_a Jt[f_a] to the workspace dz.  Also the scorer
//   k_pnn_wgrad    DeepFM's scheme (fm_deepfm.hip's k_deepfm_wgrad, whose launcher refuses a first layer above 768 rows): a workgroup
//                  per (64 x 64 tile of a W_l, split of kDeepGradRows rows), one partial per split; then the column sums
// The dense update is fm_deepfm.hip's launch_deepfm_dupdate; v, w, w0 and the statistics: fm_fwfm.hip's backward and update launches.
// No atomics: one writer per element, every sum in an order fixed by the data and by the constants of fm_pnn.h and fm_deepfm.h.
#include "fm_device.h"
#include "fm_finish.h"      // pair_sigma_residual
#include "fm_pnn.h"

namespace fmhip {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int kWaves = kBlock / 64;
constexpr int kNQ = kDeepMaxUnits / 16 / kWaves;          // N tiles of layer 1 a wave owns at most

// MFMA lane roles (v_mfma_f32_16x16x4_f32): lane (g, c) = (lane / 16, lane % 16) supplies A[c][g] and B[g][c] of a step and holds
// D[4g + i][c] in acc[i].  A 16-wide slice u of a reduction is four steps; step j takes k = 16u + 4g + j from lane group g — the same
// permutation on both operands — so that an A operand from LDS is one ds_read_b128.
#define PNN_MFMA4(acc, av, bv)                                                   \
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, bv.x, acc, 0, 0, 0);        \
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, bv.y, acc, 0, 0, 0);        \
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, bv.z, acc, 0, 0, 0);        \
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, bv.w, acc, 0, 0, 0)

// OUT[RT][N] = A[RT][K] . B[K][N], DeepFM's: wave w takes the N tiles w, w + 4, ... and every row tile of them.
//   BT = false: B[k][n] = W[k][n], W row-major [K][N];  BT = true: B[k][n] = W[n][k], W row-major [N][K], one global_load_dwordx4
// epi(nt, acc): the lane holds OUT[16 mt + 4g + i][16 nt + c] in acc[mt][i].
template <int MT, bool BT, typename Epi>
__device__ __forceinline__ void tile_product(const float *A, int lda, const float *__restrict__ W, int K, int N, int wave, int g, int c, Epi epi) {
    const float4 *arow = reinterpret_cast<const float4 *>(A + c * lda) + g;
    for (int nt = wave; nt < N / 16; nt += kWaves) {
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
                PNN_MFMA4(acc[mt], av, bv);
            }
        }
        epi(nt, acc);
    }
}

// acc[q][mt] += A[RT][16 K16] . W[16 K16][N] for the wave's N tiles nt = wave + 4 q: the first layer's streamed reduction, the
// accumulators the caller's across every call
template <int MT>
__device__ __forceinline__ void accumulate(f32x4 (&acc)[kNQ][MT], const float *A, int lda, const float *__restrict__ W, int K16, int N, int wave, int g, int c) {
    const float4 *arow = reinterpret_cast<const float4 *>(A + c * lda) + g;
#pragma unroll
    for (int q = 0; q < kNQ; ++q) {
        const int nt = wave + kWaves * q;
        if (nt >= N / 16) continue;          // (the same for the whole wave)
        for (int u = 0; u < K16; ++u) {
            const float *p = W + (int64_t)(16 * u + 4 * g) * N + nt * 16 + c;
            const float4 bv = make_float4(p[0], p[N], p[2 * N], p[3 * N]);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const float4 av = arow[mt * 4 * lda + 4 * u];
                PNN_MFMA4(acc[q][mt], av, bv);
            }
        }
    }
}

// the KP / 4 floats [Q g, Q g + Q) of a field's sum: lane group g's share of the Gram product's reduction over the factors
template <int Q>
__device__ __forceinline__ void factors_of(const float *p, bool ok, float (&o)[Q]) {
    if (Q == 4) {
        const float4 v = ok ? *reinterpret_cast<const float4 *>(p) : f4zero();
        o[0] = v.x, o[1] = v.y, o[2 % Q] = v.z, o[3 % Q] = v.w;
    } else if (Q == 2) {
        const float2 v = ok ? *reinterpret_cast<const float2 *>(p) : make_float2(0.f, 0.f);
        o[0] = v.x, o[1 % Q] = v.y;
    } else {
        o[0] = ok ? p[0] : 0.f;
    }
}

template <int KP, int MT, bool TRAIN>
__global__ __launch_bounds__(kBlock) void k_pnn_forward(PnnArgs pa) {
    constexpr int Q = KP / 4, RT = 16 * MT;
    static_assert(RT <= 64 && kPnnRowsPerBlock % RT == 0, "the row tile");
    extern __shared__ float4 pnn_lds[];
    __shared__ double sh[RT][3];
    static_assert(sizeof(sh) <= kPnnStaticLds, "fm_pnn.h budgets the statistics' tree");
    const DeepfmArgs &a = pa.d;
    const FwfmArgs &b = a.b;
    const int F = b.F, Pp = a.Pp, L = a.L, n0p = a.n[0], n1 = a.n[1];
    const int LX = Pp + kDeepPad, LY = deepfm_max(a.n[1], L >= 3 ? a.n[3] : 0) + kDeepPad, LZ = deepfm_max(kPnnStage, L >= 2 ? a.n[2] : 0) + kDeepPad;
    float *X0 = reinterpret_cast<float *>(pnn_lds);          // [RT][LX]: the field sums S
    float *Y = X0 + RT * LX;                                 // [RT][LY]: h_1, h_3, delta_3, delta_1
    float *Z = Y + RT * LY;                                  // [RT][LZ]: the staging tile; h_2, delta_2
    float *Jt = Z + RT * LZ;                                 // [RT][LX], training: d yhat / d S
    float *rlin = Jt + (TRAIN ? RT * LX : 0), *rdeep = rlin + RT;          // [RT] each
    int *rp = reinterpret_cast<int *>(rdeep + RT);           // [RT + 1] the rows' entry offsets from the tile's first entry
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, c = lane & 15;
    const float4 *V4 = reinterpret_cast<const float4 *>(b.V);
    const float w0 = *b.w0;
    const float *W1 = a.D, *uvec = a.D + a.uoff;
    double se = 0.0, sse = 0.0, nf = 0.0;    // thread j < RT: the rows j of every tile

    const int64_t row_lo = (int64_t)blockIdx.x * kPnnRowsPerBlock;
    for (int t0 = 0; t0 < kPnnRowsPerBlock; t0 += RT) {
        const int64_t r0 = row_lo + t0;
        if (r0 >= b.rows) break;             // (the same for every thread)
        const int nr = (int)min((int64_t)RT, b.rows - r0);
        const int64_t E0 = b.row_ptr[r0];
        __syncthreads();                     // the previous tile has been read
        for (int i = tid; i < RT * LX / 4; i += kBlock) reinterpret_cast<float4 *>(X0)[i] = f4zero();
        if (tid <= nr) rp[tid] = (int)(b.row_ptr[r0 + tid] - E0);
        __syncthreads();
        const int neQ = rp[nr] * Q;
        // (1) the field sums: a lane group per entry, the head of a same-field run sums its run in ascending order
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
            *reinterpret_cast<float4 *>(X0 + j * LX + (int)b.fld[E0 + p] * KP + 4 * q) = s;
        }
        __syncthreads();
        if (TRAIN && a.train_d)
            for (int i = tid; i < nr * (Pp / 4); i += kBlock) {
                const int j = i / (Pp / 4), c4 = i - j * (Pp / 4);
                reinterpret_cast<float4 *>(a.sw + (r0 + j) * n0p)[c4] = reinterpret_cast<const float4 *>(X0 + j * LX)[c4];
            }
        // the linear term: a wave per row, a lane per entry, a fixed tree
        for (int j = wave; j < nr; j += kWaves) {
            const int e0 = rp[j], n = rp[j + 1] - e0;
            float lin = lane < n ? __fmul_rn(b.w[b.col[E0 + e0 + lane]], b.val[E0 + e0 + lane]) : 0.f;
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) lin += __shfl_xor(lin, m, 64);
            if (lane == 0) rlin[j] = lin;
        }
        // (2) layer 1 over the field sums' rows of W_1; the accumulators stay in registers until the last Gram tile
        f32x4 acc[kNQ][MT];
#pragma unroll
        for (int q = 0; q < kNQ; ++q)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) acc[q][mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
        accumulate<MT>(acc, X0, LX, W1, Pp / 16, n1, wave, g, c);
        // (3) the Gram tiles: produced into Z, consumed at once
        for (int t = 0; t < pa.t.n; ++t) {
            const int fm = 16 * pa.t.mt[t], fn = 16 * pa.t.nt[t], ns = pa.t.ns[t], off = Pp + pa.t.off[t];
            for (int j = wave; j < RT; j += kWaves) {          // (a row past nr has all-zero sums: its products are 0)
                const float *srow = X0 + j * LX + Q * g;
                float av[Q], bv[Q];
                factors_of<Q>(srow + (fm + c) * KP, fm + c < F, av);
                factors_of<Q>(srow + (fn + c) * KP, fn + c < F, bv);
                f32x4 gr = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int q = 0; q < Q; ++q) gr = __builtin_amdgcn_mfma_f32_16x16x4f32(av[q], bv[q], gr, 0, 0, 0);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int il = 4 * g + i;
                    const float v = (fm + il < fn + c && fn + c < F) ? gr[i] : 0.f;          // a pad slot is 0
                    Z[j * LZ + il * 16 + c] = v;
                    if (TRAIN && a.train_d && j < nr && il < ns) a.sw[(r0 + j) * n0p + off + il * 16 + c] = v;
                }
            }
            __syncthreads();
            accumulate<MT>(acc, Z, LZ, W1 + (int64_t)off * n1, ns, n1, wave, g, c);
            __syncthreads();
        }
        // (4) bias and ReLU: h_1 into Y
        {
            const float *bias = a.D + a.boff[0];
            float *hw = a.hw[0] + r0 * n1;
#pragma unroll
            for (int q = 0; q < kNQ; ++q) {
                const int n = (wave + kWaves * q) * 16 + c;
                if (n >= n1) continue;
                const float bn = bias[n];
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int j = mt * 16 + 4 * g + i;
                        const float h = fmaxf(acc[q][mt][i] + bn, 0.f);
                        Y[j * LY + n] = h;
                        if (TRAIN && j < nr) hw[(int64_t)j * n1 + n] = h;
                    }
            }
        }
        __syncthreads();
        // the layers above: h_l = relu(h_{l-1} W_l + b_l), Y -> Z -> Y
        for (int l = 2; l <= L; ++l) {
            const float *in = (l & 1) ? Z : Y;
            float *out = (l & 1) ? Y : Z;
            const int ldi = (l & 1) ? LZ : LY, ldo = (l & 1) ? LY : LZ, N = a.n[l];
            const float *bias = a.D + a.boff[l - 1];
            float *hw = a.hw[l - 1] + r0 * N;
            tile_product<MT, false>(in, ldi, a.D + a.woff[l - 1], a.n[l - 1], N, wave, g, c, [&](int nt, const f32x4 *pr) {
                const int n = nt * 16 + c;
                const float bn = bias[n];
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int j = mt * 16 + 4 * g + i;
                        const float h = fmaxf(pr[mt][i] + bn, 0.f);
                        out[j * ldo + n] = h;
                        if (TRAIN && j < nr) hw[(int64_t)j * N + n] = h;
                    }
            });
            __syncthreads();
        }
        // <h_L, u>: a wave per row, lane i the units i, i + 64, ..., a fixed tree
        {
            const float *hl = (L & 1) ? Y : Z;
            const int ld = (L & 1) ? LY : LZ, N = a.n[L];
            for (int j = wave; j < nr; j += kWaves) {
                float t = 0.f;
                for (int i = lane; i < N; i += 64) t = fmaf(hl[j * ld + i], uvec[i], t);
#pragma unroll
                for (int m = 32; m >= 1; m >>= 1) t += __shfl_xor(t, m, 64);
                if (lane == 0) rdeep[j] = t;
            }
        }
        __syncthreads();
        if (tid < nr) {
            const float yh = (w0 + rlin[tid]) + rdeep[tid];
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
        // (5) backwards, d yhat / d . per row: delta_L = u o [h_L > 0] in h_L's place
        {
            float *hl = (L & 1) ? Y : Z;
            const int ld = (L & 1) ? LY : LZ, N = a.n[L];
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
            const float *in = (l & 1) ? Y : Z;
            float *out = (l & 1) ? Z : Y;
            const int ldi = (l & 1) ? LY : LZ, ldo = (l & 1) ? LZ : LY, N = a.n[l - 1];
            const float *hw = a.hw[l - 2] + r0 * N;
            float *dw = a.dw[l - 2] + r0 * N;
            tile_product<MT, true>(in, ldi, a.D + a.woff[l - 1], a.n[l], N, wave, g, c, [&](int nt, const f32x4 *pr) {
                const int n = nt * 16 + c;
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int j = mt * 16 + 4 * g + i;
                        const float d = (j < nr && hw[(int64_t)j * N + n] > 0.f) ? pr[mt][i] : 0.f;
                        out[j * ldo + n] = d;
                        if (a.train_d && j < nr) dw[(int64_t)j * N + n] = d;
                    }
            });
            __syncthreads();
        }
        // Jt = delta_1 W_1[field rows]^T
        tile_product<MT, true>(Y, LY, W1, n1, Pp, wave, g, c, [&](int nt, const f32x4 *pr) {
            const int n = nt * 16 + c;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int i = 0; i < 4; ++i) Jt[(mt * 16 + 4 * g + i) * LX + n] = pr[mt][i];
        });
        // per Gram tile dG = delta_1 W_1[tile rows]^T into Z (slot il * 16 + jl; a pad slot's row of W_1 is 0, so is its dG), then
        // the row's owner wave: Jt[16 mt ..] += dG S[16 nt ..] and Jt[16 nt ..] += dG^T S[16 mt ..]
        for (int t = 0; t < pa.t.n; ++t) {
            const int fm = 16 * pa.t.mt[t], fn = 16 * pa.t.nt[t], ns = pa.t.ns[t];
            tile_product<MT, true>(Y, LY, W1 + (int64_t)(Pp + pa.t.off[t]) * n1, n1, 16 * ns, wave, g, c, [&](int nt, const f32x4 *pr) {
                const int n = nt * 16 + c;
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int i = 0; i < 4; ++i) Z[(mt * 16 + 4 * g + i) * LZ + n] = pr[mt][i];
            });
            __syncthreads();
            for (int j = wave; j < nr; j += kWaves) {
                const float *zr = Z + j * LZ, *sr = X0 + j * LX + c;
                // dG S: A[il = c][jl = 4g + ..] one ds_read_b128 of the slice c (a slice the tile does not store: 0)
                float4 a1 = *reinterpret_cast<const float4 *>(zr + c * 16 + 4 * g);
                if (c >= ns) a1 = f4zero();
                // dG^T S: A[jl = c][il = 4g + ..], the same tile read the other way round
                float4 a2 = make_float4(zr[(4 * g) * 16 + c], zr[(4 * g + 1) * 16 + c], zr[(4 * g + 2) * 16 + c], zr[(4 * g + 3) * 16 + c]);
                if (4 * g >= ns) a2.x = 0.f;
                if (4 * g + 1 >= ns) a2.y = 0.f;
                if (4 * g + 2 >= ns) a2.z = 0.f;
                if (4 * g + 3 >= ns) a2.w = 0.f;
                float4 b1, b2;               // B[field 4g + ..][factor c]
                const bool cok = c < KP;
                b1.x = (cok && fn + 4 * g < F) ? sr[(fn + 4 * g) * KP] : 0.f;
                b1.y = (cok && fn + 4 * g + 1 < F) ? sr[(fn + 4 * g + 1) * KP] : 0.f;
                b1.z = (cok && fn + 4 * g + 2 < F) ? sr[(fn + 4 * g + 2) * KP] : 0.f;
                b1.w = (cok && fn + 4 * g + 3 < F) ? sr[(fn + 4 * g + 3) * KP] : 0.f;
                b2.x = (cok && fm + 4 * g < F) ? sr[(fm + 4 * g) * KP] : 0.f;
                b2.y = (cok && fm + 4 * g + 1 < F) ? sr[(fm + 4 * g + 1) * KP] : 0.f;
                b2.z = (cok && fm + 4 * g + 2 < F) ? sr[(fm + 4 * g + 2) * KP] : 0.f;
                b2.w = (cok && fm + 4 * g + 3 < F) ? sr[(fm + 4 * g + 3) * KP] : 0.f;
                f32x4 d1 = (f32x4){0.f, 0.f, 0.f, 0.f}, d2 = d1;
                PNN_MFMA4(d1, a1, b1);
                PNN_MFMA4(d2, a2, b2);
                if (cok) {
                    float *jr = Jt + j * LX + c;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {          // (on a diagonal tile both land on the same element: one after the other)
                        if (fm + 4 * g + i < F) jr[(fm + 4 * g + i) * KP] += d1[i];
                        if (fn + 4 * g + i < F) jr[(fn + 4 * g + i) * KP] += d2[i];
                    }
                }
            }
            __syncthreads();
        }
        __syncthreads();                     // (a model without a pair: Jt is complete)
        // per entry x_a Jt[f_a]: a lane group per entry
        for (int it = tid; it < neQ; it += kBlock) {
            const int p = it / Q, q = it % Q;
            int j = 0;
            for (int step = RT / 2; step >= 1; step >>= 1)
                if (j + step < nr && rp[j + step] <= p) j += step;
            const float4 jf = *reinterpret_cast<const float4 *>(Jt + j * LX + (int)b.fld[E0 + p] * KP + 4 * q);
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

// A W_l's gradient, the reduction over the rows: M = 64 of the layer's inputs (tile ti), N = 64 of its units (tile tj).  A stage is
// kDeepGradStage rows of both operands in LDS, the A side (h_{l-1}; sw's h_0 in device order for l = 1) scaled by e on the way in;
// wave w owns the 32 x 32 corner (w / 2, w % 2) of the tile as 2 x 2 MFMA tiles.  The pitch of 80 floats puts the four rows g of a
// step 16 banks apart.  The column sums' workgroups: thread (q, col) adds the rows q, q + 4, ... of its split in ascending order, the
// four q in a fixed tree.
constexpr int kGradLd = kDeepGradTile + 16;

__global__ __launch_bounds__(kBlock) void k_pnn_wgrad(DeepfmArgs a) {
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

int wgrad_blocks(const DeepfmArgs &a) {
    int n = 0;
    for (int l = 1; l <= a.L; ++l) {
        const int tn = (a.n[l] + kDeepGradTile - 1) / kDeepGradTile;
        n += (a.n[l - 1] + kDeepGradTile - 1) / kDeepGradTile * tn + tn;
    }
    return n + (a.n[a.L] + kDeepGradTile - 1) / kDeepGradTile;
}

template <int KP, int MT>
hipError_t forward_instance(const PnnArgs &a, bool train, hipStream_t s) {
    const size_t lds = pnn_forward_lds(16 * MT, a.d.Pp, pnn_wy(a.d), pnn_wz(a.d), train);
    if (lds + kPnnStaticLds > 65536) {          // above the default limit: up to the device's own
        const void *fn = train ? reinterpret_cast<const void *>(&k_pnn_forward<KP, MT, true>) : reinterpret_cast<const void *>(&k_pnn_forward<KP, MT, false>);
        const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    dim3 g((unsigned)pnn_forward_blocks(a.d.b.rows)), b(kBlock);
    if (train) hipLaunchKernelGGL((k_pnn_forward<KP, MT, true>), g, b, lds, s, a);
    else hipLaunchKernelGGL((k_pnn_forward<KP, MT, false>), g, b, lds, s, a);
    return hipGetLastError();
}

template <int KP>
hipError_t forward_kp(const PnnArgs &a, bool train, hipStream_t s) {
    switch (pnn_row_tile(a.d.Pp, pnn_wy(a.d), pnn_wz(a.d), train, a.lds_limit)) {
        case 64: return forward_instance<KP, 4>(a, train, s);
        case 32: return forward_instance<KP, 2>(a, train, s);
        case 16: return forward_instance<KP, 1>(a, train, s);
        default: return hipErrorInvalidValue;          // (the handle refuses such a pairing before any launch)
    }
}

bool shape_ok(const PnnArgs &pa) {
    const DeepfmArgs &a = pa.d;
    PnnTiles t;
    if (a.b.F < 1 || !pnn_tiles(a.b.F, t) || t.n != pa.t.n || t.rows != pa.t.rows) return false;
    for (int i = 0; i < t.n; ++i)
        if (t.mt[i] != pa.t.mt[i] || t.nt[i] != pa.t.nt[i] || t.ns[i] != pa.t.ns[i] || t.off[i] != pa.t.off[i]) return false;
    if (a.L < 1 || a.L > kDeepMaxLayers || a.Pp % 16 || a.Pp < a.b.F * a.b.Kp || a.Pp > kPnnMaxWidth || a.n[0] != a.Pp + t.rows) return false;
    for (int l = 1; l <= a.L; ++l)
        if (a.n[l] % 16 || a.n[l] < 16 || a.n[l] > kDeepMaxUnits) return false;
    return true;
}

}  // namespace

hipError_t launch_pnn_forward(const PnnArgs &pa, bool train, hipStream_t s) {
    const DeepfmArgs &a = pa.d;
    const FwfmArgs &b = a.b;
    if (b.rows <= 0) return hipSuccess;
    if (!b.V || !b.w || !b.w0 || !a.D || !b.row_ptr || !b.yhat || !shape_ok(pa)) return hipErrorInvalidValue;
    if (train) {
        if (!b.y || !b.e || !b.bsum || !b.dz || (a.train_d && !a.sw)) return hipErrorInvalidValue;
        for (int l = 0; l < a.L; ++l)
            if (!a.hw[l] || (a.train_d && !a.dw[l])) return hipErrorInvalidValue;
    }
    switch (b.Kp) {
        case 4: return forward_kp<4>(pa, train, s);
        case 8: return forward_kp<8>(pa, train, s);
        case 16: return forward_kp<16>(pa, train, s);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_pnn_wgrad(const PnnArgs &pa, hipStream_t s) {
    const DeepfmArgs &a = pa.d;
    if (a.b.rows <= 0) return hipSuccess;
    if (!a.sw || !a.gpart || !a.b.e || a.n_splits != deepfm_grad_splits(a.b.rows) || !shape_ok(pa)) return hipErrorInvalidValue;
    for (int l = 0; l < a.L; ++l)
        if (!a.hw[l] || !a.dw[l]) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pnn_wgrad, dim3((unsigned)wgrad_blocks(a), (unsigned)a.n_splits), dim3(kBlock), 0, s, a);
    return hipGetLastError();
}

}  // namespace fmhip
