// fm_fmfm.hip — the field-matrixed FM's kernels (include/fmhip_fmfm.h; DESIGN.md, "Field-matrixed FM"): gfx950, wave64.
//   k_fmfm_forward   a workgroup owns kFmfmRowsPerBlock rows and walks them in tiles of RT rows: the tile's concatenated field sums
//                    S[RT][Pp] go to LDS, Z = S . MM is formed on the exact-f32 MFMA with S as the A operand and MM streamed from L2
//                    as B, and straight from the accumulators come the pair term 1/2 S o Z and x_a Z_{f_a} (to the workspace dz);
//                    when M is trained the tile's S rows also go to the workspace sw.  Also the scorer
//   k_fmfm_mgrad     G = sum_r e_r s_r s_r^T: a workgroup per (64 x 64 tile on or above the diagonal, split of kFmfmGradRows rows)
//                    stages (e sw)[rows][tile i] and sw[rows][tile j] through LDS and leaves one partial per split
//   k_fmfm_mupdate   a thread per element of the blocks f < g: the splits' partials in split order, the step, the element and its
//                    transpose mirror
// v, w, w0 and the statistics: fm_fwfm.hip's backward and update launches over this forward's dz, e and bsum.
// No atomics: one writer per element, every sum in an order fixed by the data and by the constants of fm_fmfm.h — never by the CU count.
#include "fm_device.h"
#include "fm_finish.h"      // pair_sigma_residual
#include "fm_fmfm.h"

namespace fmhip {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// MFMA lane roles (v_mfma_f32_16x16x4_f32): lane (g, c) = (lane / 16, lane % 16) supplies A[c][g] and B[g][c] of a step and holds
// D[4g + i][c] in acc[i].
//
// Z = S . MM: M = the tile's rows (RT / 16 tiles), N = the Pp columns, the reduction over Pp.  Wave w takes the N tiles w, w + 4, ...
// and every row tile of them, so a fragment of MM it loads is used RT / 16 times.  A 16-wide slice u of the reduction is four MFMA
// steps; step j takes k = 16u + 4g + j from lane group g — the same permutation on both operands — so that A is one ds_read_b128 of
// S[row c][16u + 4g ..] and B one global_load_dwordx4 of MM[16 nt + c][16u + 4g ..], which is MM[16u + 4g ..][16 nt + c]: MM is
// symmetric to the bit.
template <int KP, int RT, bool TRAIN>
__global__ __launch_bounds__(kBlock) void k_fmfm_forward(FmfmArgs a) {
    constexpr int Q = KP / 4, MT = RT / 16;
    static_assert(RT % 16 == 0 && RT <= 64 && kFmfmRowsPerBlock % RT == 0, "the row tile");
    extern __shared__ float4 fmfm_lds[];
    __shared__ double sh[RT][3];
    const FwfmArgs &b = a.b;
    const int F = b.F, Pp = a.Pp, LD = Pp + kFmfmPad;
    float *S = reinterpret_cast<float *>(fmfm_lds);          // [RT][LD]
    float *pairp = S + RT * LD;                              // [4][RT]: the waves' parts of the rows' sum S o Z
    float *rlin = pairp + 4 * RT;                            // [RT]
    int *rp = reinterpret_cast<int *>(rlin + RT);            // [RT + 1] the rows' entry offsets from the tile's first entry
    uint16_t *head = reinterpret_cast<uint16_t *>(rp + RT + 1);          // [RT][F] the run of (row, field): its first entry in the tile
    uint8_t *len = reinterpret_cast<uint8_t *>(head + RT * F);           // [RT][F] ... and its length, 0 for a field the row lacks
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, c = lane & 15;
    const float4 *V4 = reinterpret_cast<const float4 *>(b.V);
    const float w0 = *b.w0;
    double se = 0.0, sse = 0.0, nf = 0.0;    // thread j < RT: the rows j of every tile

    const int64_t row_lo = (int64_t)blockIdx.x * kFmfmRowsPerBlock;
    for (int t0 = 0; t0 < kFmfmRowsPerBlock; t0 += RT) {
        const int64_t r0 = row_lo + t0;
        if (r0 >= b.rows) break;             // (the same for every thread)
        const int nr = (int)min((int64_t)RT, b.rows - r0);
        const int64_t E0 = b.row_ptr[r0];
        __syncthreads();                     // the previous tile has been read
        for (int i = tid; i < RT * LD / 4; i += kBlock) reinterpret_cast<float4 *>(S)[i] = f4zero();
        for (int i = tid; i < RT * F / 4; i += kBlock) reinterpret_cast<uint32_t *>(len)[i] = 0u;
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
            const int f = b.fld[E0 + p];
            *reinterpret_cast<float4 *>(S + j * LD + f * KP + 4 * q) = s;
            if (q == 0) {
                head[j * F + f] = (uint16_t)p;
                len[j * F + f] = (uint8_t)rb;
            }
        }
        // the linear terms: a wave per row, a lane per entry, a fixed tree
        for (int j = wave; j < nr; j += kBlock / 64) {
            const int e0 = rp[j], n = rp[j + 1] - e0;
            float t = lane < n ? __fmul_rn(b.w[b.col[E0 + e0 + lane]], b.val[E0 + e0 + lane]) : 0.f;
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) t += __shfl_xor(t, m, 64);
            if (lane == 0) rlin[j] = t;
        }
        __syncthreads();
        if (TRAIN && a.train_m) {
            float4 *out = reinterpret_cast<float4 *>(a.sw) + r0 * (Pp / 4);
            for (int i = tid; i < nr * (Pp / 4); i += kBlock) {
                const int j = i / (Pp / 4), c4 = i - j * (Pp / 4);
                out[i] = reinterpret_cast<const float4 *>(S + j * LD)[c4];
            }
        }
        float pacc[MT][4];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int i = 0; i < 4; ++i) pacc[mt][i] = 0.f;
        for (int nt = wave; nt < Pp / 16; nt += kBlock / 64) {
            f32x4 acc[MT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) acc[mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
            const float4 *mrow = reinterpret_cast<const float4 *>(a.MM + (int64_t)(nt * 16 + c) * Pp) + g;
            const float4 *srow = reinterpret_cast<const float4 *>(S + c * LD) + g;
            for (int u = 0; u < Pp / 16; ++u) {
                const float4 bv = mrow[4 * u];
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
                    const float4 av = srow[mt * 4 * LD + 4 * u];
                    acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, bv.x, acc[mt], 0, 0, 0);
                    acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, bv.y, acc[mt], 0, 0, 0);
                    acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, bv.z, acc[mt], 0, 0, 0);
                    acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, bv.w, acc[mt], 0, 0, 0);
                }
            }
            // the lane holds Z[row 16 mt + 4g + i][column n]: column n is slot d of field f
            const int n = nt * 16 + c, f = n / KP, d = n % KP;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int j = mt * 16 + 4 * g + i;
                    const float z = acc[mt][i];
                    pacc[mt][i] = fmaf(S[j * LD + n], z, pacc[mt][i]);
                    if (TRAIN && f < F) {
                        const int rb = len[j * F + f];
                        const int64_t at = E0 + head[j * F + f];
                        for (int t = 0; t < rb; ++t) b.dz[(at + t - b.nnz0) * KP + d] = b.val[at + t] * z;
                    }
                }
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float v = pacc[mt][i];
#pragma unroll
                for (int m = 1; m <= 8; m <<= 1) v += __shfl_xor(v, m, 64);
                if (c == 0) pairp[wave * RT + mt * 16 + 4 * g + i] = v;
            }
        __syncthreads();
        if (tid < nr) {
            const float pair = (pairp[tid] + pairp[RT + tid]) + (pairp[2 * RT + tid] + pairp[3 * RT + tid]);
            const float yh = (w0 + rlin[tid]) + 0.5f * pair;
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

// G = sum_r (e_r s_r) s_r^T on the same MFMA, the reduction over the rows: M = the 64 columns of tile ti, N = those of tile tj >= ti.
// A stage is kFmfmGradStage rows of both operands in LDS, the A side scaled by e on the way in; wave w owns the 32 x 32 corner
// (w / 2, w % 2) of the tile as 2 x 2 MFMA tiles: two A and two B reads per four MFMAs.  The LDS pitch of 80 floats puts the four
// rows g of a step 16 banks apart.
constexpr int kGradLd = kFmfmGradTile + 16;

__global__ __launch_bounds__(kBlock) void k_fmfm_mgrad(FmfmArgs a) {
    __shared__ __attribute__((aligned(16))) float A[kFmfmGradStage * kGradLd], B[kFmfmGradStage * kGradLd];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, c = lane & 15;
    const int Pp = a.Pp, T = (Pp + kFmfmGradTile - 1) / kFmfmGradTile;
    int ti = 0, rem = blockIdx.x;
    while (rem >= T - ti) rem -= T - ti++;
    const int tj = ti + rem;
    const int row_lo = blockIdx.y * kFmfmGradRows, row_hi = min(a.b.rows, row_lo + kFmfmGradRows);
    const int m0 = 32 * (wave >> 1), n0 = 32 * (wave & 1);
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i >> 1][i & 1] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int k0 = row_lo; k0 < row_hi; k0 += kFmfmGradStage) {
        __syncthreads();                     // the previous stage has been read
        for (int i = tid; i < 2 * kFmfmGradStage * (kFmfmGradTile / 4); i += kBlock) {
            const int side = i / (kFmfmGradStage * (kFmfmGradTile / 4)), rr = i / (kFmfmGradTile / 4) % kFmfmGradStage, c4 = i % (kFmfmGradTile / 4);
            const int row = k0 + rr, col = (side ? tj : ti) * kFmfmGradTile + 4 * c4;
            float4 v = f4zero();
            if (row < row_hi && col < Pp) {
                v = *reinterpret_cast<const float4 *>(a.sw + (int64_t)row * Pp + col);
                if (!side) v = f4mul(v, a.b.e[row]);
            }
            *reinterpret_cast<float4 *>((side ? B : A) + rr * kGradLd + 4 * c4) = v;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < kFmfmGradStage; kk += 4) {
            const float *pa = A + (kk + g) * kGradLd + m0 + c, *pb = B + (kk + g) * kGradLd + n0 + c;
            const float a0 = pa[0], a1 = pa[16], b0 = pb[0], b1 = pb[16];
            acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
    float *out = a.mpart + (int64_t)blockIdx.y * Pp * Pp;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int nj = 0; nj < 2; ++nj)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int p = ti * kFmfmGradTile + m0 + 16 * mi + 4 * g + i, q = tj * kFmfmGradTile + n0 + 16 * nj + c;
                if (p < Pp && q < Pp) out[(int64_t)p * Pp + q] = acc[mi][nj][i];
            }
}

// A thread per element (p, q) of MM; those of a block f < g inside the k x k factors sum their partials — split s into accumulator
// s % 8 in split order, the eight in a fixed tree: eight loads in flight — step on g / |B| + regm theta and write the element and its
// mirror (q, p).  Diagonal blocks and pad slots are never written.
template <bool ADAGRAD>
__global__ __launch_bounds__(kBlock) void k_fmfm_mupdate(FmfmArgs a) {
    const int Pp = a.Pp, KP = a.b.Kp;
    const int idx = blockIdx.x * kBlock + threadIdx.x;
    if (idx >= Pp * Pp) return;
    const int p = idx / Pp, q = idx - p * Pp;
    if (p / KP >= q / KP || q / KP >= a.b.F || p % KP >= a.k || q % KP >= a.k) return;
    const float *src = a.mpart + idx;
    const int64_t rec = (int64_t)Pp * Pp;
    float s8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < a.n_splits; s += 8)
#pragma unroll
        for (int j = 0; j < 8; ++j) s8[j] += s + j < a.n_splits ? src[(s + j) * rec] : 0.f;
    const float sum = ((s8[0] + s8[1]) + (s8[2] + s8[3])) + ((s8[4] + s8[5]) + (s8[6] + s8[7]));
    float th = a.MM[idx];
    const float gh = fmaf(a.regm, th, sum * a.b.invb);
    if (ADAGRAD) {
        float n = a.NM[idx];
        adagrad_step(th, n, gh, a.b.eta, a.b.eps);
        a.NM[idx] = n;
        a.NM[q * Pp + p] = n;
    } else {
        th = th - a.b.eta * gh;
    }
    a.MM[idx] = th;
    a.MM[q * Pp + p] = th;
}

template <int KP, int RT>
hipError_t forward_instance(const FmfmArgs &a, bool train, hipStream_t s) {
    constexpr int PPMAX = fmfm_max_pp(RT), FMAX = PPMAX / KP < 64 ? PPMAX / KP : 64;
    static_assert(fmfm_forward_lds(RT, PPMAX, FMAX) + RT * 3 * sizeof(double) <= 65536, "the forward's LDS stays inside 64 KB");
    if (a.Pp > PPMAX || a.b.F > FMAX) return hipErrorInvalidValue;
    const size_t lds = fmfm_forward_lds(RT, a.Pp, a.b.F);
    dim3 g((unsigned)fmfm_forward_blocks(a.b.rows)), b(kBlock);
    if (train) hipLaunchKernelGGL((k_fmfm_forward<KP, RT, true>), g, b, lds, s, a);
    else hipLaunchKernelGGL((k_fmfm_forward<KP, RT, false>), g, b, lds, s, a);
    return hipGetLastError();
}

template <int KP>
hipError_t forward_kp(const FmfmArgs &a, bool train, hipStream_t s) {
    switch (fmfm_row_tile(a.Pp)) {
        case 64: return forward_instance<KP, 64>(a, train, s);
        case 32: return forward_instance<KP, 32>(a, train, s);
        default: return forward_instance<KP, 16>(a, train, s);
    }
}

}  // namespace

hipError_t launch_fmfm_forward(const FmfmArgs &a, bool train, hipStream_t s) {
    const FwfmArgs &b = a.b;
    if (b.rows <= 0) return hipSuccess;
    if (!b.V || !b.w || !b.w0 || !a.MM || !b.row_ptr || !b.yhat || b.F < 1 || a.Pp % 16 || a.Pp < b.F * b.Kp || a.Pp > kFmfmMaxWidth) return hipErrorInvalidValue;
    if (train && (!b.y || !b.e || !b.bsum || !b.dz || (a.train_m && !a.sw))) return hipErrorInvalidValue;
    switch (b.Kp) {
        case 4: return forward_kp<4>(a, train, s);
        case 8: return forward_kp<8>(a, train, s);
        case 16: return forward_kp<16>(a, train, s);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_fmfm_mgrad(const FmfmArgs &a, hipStream_t s) {
    if (a.b.rows <= 0) return hipSuccess;
    if (!a.sw || !a.mpart || !a.b.e || a.n_splits != fmfm_grad_splits(a.b.rows) || a.Pp % 16 || a.Pp > kFmfmMaxWidth) return hipErrorInvalidValue;
    const int T = (a.Pp + kFmfmGradTile - 1) / kFmfmGradTile;
    hipLaunchKernelGGL(k_fmfm_mgrad, dim3((unsigned)(T * (T + 1) / 2), (unsigned)a.n_splits), dim3(kBlock), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_fmfm_mupdate(const FmfmArgs &a, bool adagrad, hipStream_t s) {
    if (a.b.rows <= 0) return hipSuccess;
    if (!a.MM || !a.mpart || (adagrad && !a.NM)) return hipErrorInvalidValue;
    dim3 g((unsigned)((a.Pp * a.Pp + kBlock - 1) / kBlock)), b(kBlock);
    if (adagrad) hipLaunchKernelGGL(k_fmfm_mupdate<true>, g, b, 0, s, a);
    else hipLaunchKernelGGL(k_fmfm_mupdate<false>, g, b, 0, s, a);
    return hipGetLastError();
}

}  // namespace fmhip
