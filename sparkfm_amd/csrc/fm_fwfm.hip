// fm_fwfm.hip — the field-weighted FM's kernels (include/fmhip_fwfm.h; DESIGN.md, "Field-weighted FM"): gfx950, wave64.
//   k_fwfm_forward   a workgroup owns kFwfmRowsPerBlock rows and walks them in row tiles: the field sums S[f][row, d] of a tile go to
//                    LDS, Z0 = R0 . S is formed on the exact-f32 MFMA with R0 (r without its diagonal) as the stationary A operand,
//                    then per entry D_a, the pair term and x_a D_a (to the workspace dz); when r is trained a second MFMA product
//                    (e S) S^T is kept in registers over the whole block.  Also the scorer
//   k_fwfm_backward  a lane group of Kp/4 lanes per (column, chunk of 256 occurrences): sums e_r dz in occurrence order; a column of
//                    one chunk steps v[i] and w[i] in place (nothing in this launch reads them), a longer one leaves per-chunk partials
//   k_fwfm_update    the columns of several chunks, their partials in chunk order; a few more workgroups sum the forward's block
//                    partials in block order and step r (upper triangle, mirrored), a last one w0, and leaves the statistics
// No atomics: one writer per element, every sum in an order fixed by the data and by the constants of fm_fwfm.h — never by the CU count.
#include "fm_device.h"
#include "fm_finish.h"      // pair_sigma_residual
#include "fm_fwfm.h"

namespace fmhip {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// one parameter's step on g_hat = g + reg * theta (g: the batch's mean gradient); n: its AdaGrad accumulator, untouched under SGD
template <bool ADAGRAD>
__device__ __forceinline__ void fwfm_rule(float &th, float &n, float g, float reg, float eta, float eps) {
    const float gh = fmaf(reg, th, g);
    if (ADAGRAD) adagrad_step(th, n, gh, eta, eps);
    else th = th - eta * gh;
}

// MFMA lane roles (v_mfma_f32_16x16x4_f32): lane (g, c) = (lane / 16, lane % 16) supplies A[c][g] and B[g][c] of a step and holds
// D[4g + i][c] in acc[i].
//
// Z0 = R0 . S: M = the Fp fields (MT tiles), N = the tile's NC = rows * KP columns, the reduction over the Fp fields in steps of 4.
// Wave w of the 4 takes M tile w % MT and every NS-th N tile from w / MT, NS = 4 / MT (MT = 3: the fourth wave sits this phase out);
// its slice of R0, Fp / 4 floats a lane, stays in registers for the launch.
// (e S) S^T: M = N = the fields, the reduction over the tile's NC columns — lane group g takes the columns 16t + 4g .. + 3 of a
// 16-column step with one ds_read_b128 per operand, the same permutation on both sides — accumulated over every tile of the block in
// up to three 16 x 16 tiles a wave (the MT (MT + 1) / 2 tiles on and above the diagonal, dealt round-robin).
template <int KP, int MT, bool TRAIN>
__global__ __launch_bounds__(kBlock) void k_fwfm_forward(FwfmArgs a) {
    constexpr int FP = 16 * MT, NC = fwfm_cols(MT), LDN = fwfm_ld(MT), RT = NC / KP, RS = FP + 1, Q = KP / 4, NS = 4 / MT, NT2 = MT * (MT + 1) / 2;
    static_assert(RT <= 64 && RT + 1 <= kBlock && kFwfmRowsPerBlock % RT == 0, "the row tile");
    extern __shared__ float4 fwfm_lds[];
    __shared__ double sh[RT][3];
    float *S = reinterpret_cast<float *>(fwfm_lds);          // [FP][LDN]
    float *Z = S + FP * LDN;                                 // [FP][LDN]
    float *rlin = Z + FP * LDN, *rpair = rlin + RT * RS, *rdg = rpair + RT * RS;          // [RT][RS]: per (row, field)
    float *ev = rdg + RT * RS;                               // [RT] e_r (0 past the batch's rows)
    int *rp = reinterpret_cast<int *>(ev + RT);              // [RT + 1] the rows' entry offsets from the tile's first entry
    uint8_t *erow = reinterpret_cast<uint8_t *>(fwfm_lds) + (2 * FP * LDN + 3 * RT * RS + RT + (RT + 1) + 3) / 4 * 16;          // [RT * 64]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, c = lane & 15;
    const int F = a.F;
    const float4 *V4 = reinterpret_cast<const float4 *>(a.V);
    const float w0 = *a.w0;

    const int mt = wave % MT, ns = wave / MT;
    const bool zwave = wave < MT * NS;
    float A[FP / 4];
#pragma unroll
    for (int s = 0; s < FP / 4; ++s) {
        const int fr = mt * 16 + c, fc = 4 * s + g;
        A[s] = (fr < F && fc < F && fr != fc) ? a.r[fr * F + fc] : 0.f;
    }
    f32x4 gacc[3];
    int gmi[3], gmj[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        gacc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        int mi = 0, rem = wave + 4 * j;
        while (mi < MT && rem >= MT - mi) rem -= MT - mi++;
        gmi[j] = mi;
        gmj[j] = mi + rem;
    }
    float dgacc = 0.f;                       // thread f < F: r[f][f]'s gradient
    double se = 0.0, sse = 0.0, nf = 0.0;    // thread j < RT: the rows j of every tile

    const int64_t row_lo = (int64_t)blockIdx.x * kFwfmRowsPerBlock;
    for (int t0 = 0; t0 < kFwfmRowsPerBlock; t0 += RT) {
        const int64_t r0 = row_lo + t0;
        if (r0 >= a.rows) break;             // (the same for every thread)
        const int nr = (int)min((int64_t)RT, a.rows - r0);
        const int64_t E0 = a.row_ptr[r0];
        __syncthreads();                     // the previous tile has been read
        for (int i = tid; i < FP * LDN / 4; i += kBlock) reinterpret_cast<float4 *>(S)[i] = f4zero();
        for (int i = tid; i < 3 * RT * RS; i += kBlock) rlin[i] = 0.f;
        if (tid <= nr) rp[tid] = (int)(a.row_ptr[r0 + tid] - E0);
        __syncthreads();
        for (int j = wave; j < nr; j += kBlock / 64) {
            const int b = rp[j];
            if (lane < rp[j + 1] - b) erow[b + lane] = (uint8_t)j;
        }
        __syncthreads();
        const int neQ = rp[nr] * Q;
        // the field sums: a lane group per entry, the head of a same-field run sums its run in ascending order
        for (int it = tid; it < neQ; it += kBlock) {
            const int p = it / Q, q = it % Q;
            const int rb = a.run[E0 + p];
            if (rb == 0) continue;
            float4 s = f4zero();
            for (int t = 0; t < rb; ++t) {
                const float x = a.val[E0 + p + t];
                const float4 v = V4[(int64_t)a.col[E0 + p + t] * Q + q];
                s.x = fmaf(x, v.x, s.x);
                s.y = fmaf(x, v.y, s.y);
                s.z = fmaf(x, v.z, s.z);
                s.w = fmaf(x, v.w, s.w);
            }
            *reinterpret_cast<float4 *>(S + (int)a.fld[E0 + p] * LDN + (int)erow[p] * KP + 4 * q) = s;
        }
        __syncthreads();
        if (zwave) {
            for (int nt = ns; nt < NC / 16; nt += NS) {
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                const float *b = S + g * LDN + nt * 16 + c;
#pragma unroll
                for (int s = 0; s < FP / 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(A[s], b[4 * s * LDN], acc, 0, 0, 0);
                float *z = Z + (mt * 16 + 4 * g) * LDN + nt * 16 + c;
#pragma unroll
                for (int i = 0; i < 4; ++i) z[i * LDN] = acc[i];
            }
        }
        __syncthreads();
        // per run, its head's lane group again: D_a = Z0[f] + r[f][f] (S_f - u_a), the pair and linear terms, x_a D_a.  The products
        // and differences are the rounded ones (no contraction): a field of one entry has S_f - u_a == 0 exactly.
        for (int base = 0; base < neQ; base += kBlock) {
            const int it = base + tid;
            const bool ok = it < neQ;
            const int p = ok ? it / Q : 0, q = it % Q;
            const int rb = ok ? a.run[E0 + p] : 0;
            float pr = 0.f, dg = 0.f, ln = 0.f;
            int at = 0;
            if (rb > 0) {
                const int f = a.fld[E0 + p], j = erow[p];
                at = j * RS + f;
                const float rff = a.r[f * F + f];
                const float4 Sf = *reinterpret_cast<const float4 *>(S + f * LDN + j * KP + 4 * q);
                const float4 Zf = *reinterpret_cast<const float4 *>(Z + f * LDN + j * KP + 4 * q);
                for (int t = 0; t < rb; ++t) {
                    const float x = a.val[E0 + p + t];
                    const int64_t i = a.col[E0 + p + t];
                    const float4 v = V4[i * Q + q];
                    const float4 u = make_float4(__fmul_rn(x, v.x), __fmul_rn(x, v.y), __fmul_rn(x, v.z), __fmul_rn(x, v.w));
                    const float4 o = make_float4(__fsub_rn(Sf.x, u.x), __fsub_rn(Sf.y, u.y), __fsub_rn(Sf.z, u.z), __fsub_rn(Sf.w, u.w));
                    const float4 D = make_float4(fmaf(rff, o.x, Zf.x), fmaf(rff, o.y, Zf.y), fmaf(rff, o.z, Zf.z), fmaf(rff, o.w, Zf.w));
                    pr += f4dot(u, D);
                    dg += f4dot(u, o);
                    if (TRAIN) reinterpret_cast<float4 *>(a.dz)[(E0 + p + t - a.nnz0) * Q + q] = f4mul(D, x);
                    if (q == 0) ln = fmaf(a.w[i], x, ln);
                }
            }
#pragma unroll
            for (int m = Q / 2; m >= 1; m >>= 1) {
                pr += __shfl_xor(pr, m, 64);
                dg += __shfl_xor(dg, m, 64);
            }
            if (rb > 0 && q == 0) {
                rlin[at] = ln;
                rpair[at] = 0.5f * pr;
                rdg[at] = 0.5f * dg;
            }
        }
        __syncthreads();
        if (tid < RT) {
            float e = 0.f;
            if (tid < nr) {
                float lin = 0.f, pair = 0.f;
                for (int f = 0; f < F; ++f) {
                    lin += rlin[tid * RS + f];
                    pair += rpair[tid * RS + f];
                }
                const float yh = (w0 + lin) + pair;
                a.yhat[r0 + tid] = yh;
                if (TRAIN) {
                    float z;
                    e = a.loss == kLossLogistic ? pair_sigma_residual(yh, a.y[r0 + tid] > 0.f, z) : yh - a.y[r0 + tid];
                    a.e[r0 + tid] = e;
                    se += (double)e;
                    sse += (double)e * (double)e;
                    nf += isfinite(yh) ? 0.0 : 1.0;
                }
            }
            ev[tid] = e;
        }
        if (TRAIN && a.train_r) {
            __syncthreads();
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                if (wave + 4 * j >= NT2) continue;
                const float *pa = S + (gmi[j] * 16 + c) * LDN + 4 * g, *pb = S + (gmj[j] * 16 + c) * LDN + 4 * g;
                for (int n0 = 0; n0 < NC; n0 += 16) {
                    const float4 av = *reinterpret_cast<const float4 *>(pa + n0), bv = *reinterpret_cast<const float4 *>(pb + n0);
                    const float e = ev[(n0 + 4 * g) / KP];
                    gacc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x * e, bv.x, gacc[j], 0, 0, 0);
                    gacc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y * e, bv.y, gacc[j], 0, 0, 0);
                    gacc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z * e, bv.z, gacc[j], 0, 0, 0);
                    gacc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w * e, bv.w, gacc[j], 0, 0, 0);
                }
            }
            if (tid < F)
                for (int j = 0; j < nr; ++j) dgacc = fmaf(ev[j], rdg[j * RS + tid], dgacc);
        }
    }
    if (TRAIN) {
        if (a.train_r) {
            float *out = a.rpart + (int64_t)blockIdx.x * fwfm_rpart(FP);
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                if (wave + 4 * j >= NT2) continue;
#pragma unroll
                for (int i = 0; i < 4; ++i) out[(gmi[j] * 16 + 4 * g + i) * FP + gmj[j] * 16 + c] = gacc[j][i];
            }
            if (tid < FP) out[FP * FP + tid] = dgacc;
        }
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
            a.bsum[(int64_t)blockIdx.x * 4 + tid] = t;
        }
        if (tid == 3) a.bsum[(int64_t)blockIdx.x * 4 + 3] = 0.0;
    }
}

// the rule on quad q of v[i] and, from q == 0, on w[i]; g, gw: the batch's gradient sums
template <bool ADAGRAD>
__device__ __forceinline__ void fwfm_apply(const FwfmArgs &a, int64_t i, int Q, int q, float4 g, float gw) {
    const int64_t at = i * Q + q;
    float4 v = reinterpret_cast<float4 *>(a.V)[at];
    float4 n = ADAGRAD ? reinterpret_cast<float4 *>(a.NV)[at] : f4zero();
    fwfm_rule<ADAGRAD>(v.x, n.x, g.x * a.invb, a.regv, a.eta, a.eps);
    fwfm_rule<ADAGRAD>(v.y, n.y, g.y * a.invb, a.regv, a.eta, a.eps);
    fwfm_rule<ADAGRAD>(v.z, n.z, g.z * a.invb, a.regv, a.eta, a.eps);
    fwfm_rule<ADAGRAD>(v.w, n.w, g.w * a.invb, a.regv, a.eta, a.eps);
    reinterpret_cast<float4 *>(a.V)[at] = v;
    if (ADAGRAD) reinterpret_cast<float4 *>(a.NV)[at] = n;
    if (q == 0 && a.linear) {
        float th = a.w[i], nw = ADAGRAD ? a.Nw[i] : 0.f;
        fwfm_rule<ADAGRAD>(th, nw, gw * a.invb, a.regw, a.eta, a.eps);
        a.w[i] = th;
        if (ADAGRAD) a.Nw[i] = nw;
    }
}

// A thread per (chunk, float4 of the factor row): the chunk's occurrences one after the other, no V row read.
template <int KP, bool ADAGRAD>
__global__ __launch_bounds__(kBlock) void k_fwfm_backward(FwfmArgs a) {
    constexpr int Q = KP / 4;
    const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int ch = (int)(idx / Q), q = (int)(idx % Q);
    if (ch >= a.n_chunks) return;
    const int c = a.chunk_col[ch];
    const int lo = a.cptr[c] + kFwfmChunkLen * (ch - a.chunk0[c]);
    const int hi = min(lo + kFwfmChunkLen, a.cptr[c + 1]);
    const float4 *dz4 = reinterpret_cast<const float4 *>(a.dz);
    float4 g = f4zero();
    float gw = 0.f;
    for (int o = lo; o < hi; ++o) {
        const int r = a.occ_row[o];
        const int64_t at = a.row_ptr[r] + a.occ_pos[o];
        const float e = a.e[r];
        f4fma(g, dz4[(at - a.nnz0) * Q + q], e);
        gw = fmaf(e, a.val[at], gw);
    }
    if (a.chunk0[c + 1] - a.chunk0[c] == 1) {
        fwfm_apply<ADAGRAD>(a, a.cfeat[c], Q, q, g, gw);
    } else {
        float4 *rec = reinterpret_cast<float4 *>(a.part) + (int64_t)ch * (Q + kFwfmPartTail / 4);
        rec[q] = g;
        if (q == 0) rec[Q] = make_float4(gw, 0.f, 0.f, 0.f);
    }
}

// A thread per (column, float4): a column of several chunks sums their partials in chunk order and steps.  Behind the columns'
// workgroups come ceil(F^2 / 256) for r — a thread per element of its upper triangle: the forward's block partials, block b into
// accumulator b % 8 in block order, the eight in a fixed tree; it steps the element and mirrors it — and one last for w0: its first
// wave adds the statistics' block partials (lane l the blocks l, l + 64, ..., then a fixed tree), steps w0 and leaves the statistics.
template <bool ADAGRAD>
__global__ __launch_bounds__(kBlock) void k_fwfm_update(FwfmArgs a) {
    const int rblocks = (a.F * a.F + kBlock - 1) / kBlock;
    if (blockIdx.x + 1 + rblocks >= gridDim.x && blockIdx.x + 1 < gridDim.x) {
        const int F = a.F, FP = a.Fp, rec = fwfm_rpart(FP);
        const int idx = (int)(blockIdx.x + 1 + rblocks - gridDim.x) * kBlock + threadIdx.x;
        const int f = idx / F, h = idx - f * F;
        if (!a.train_r || idx >= F * F || f > h) return;
        const float *src = a.rpart + (f < h ? f * FP + h : FP * FP + f);
        float s8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};          // block b adds into s8[b % 8]: eight loads in flight
        for (int b = 0; b < a.n_blocks; b += 8)
#pragma unroll
            for (int j = 0; j < 8; ++j) s8[j] += b + j < a.n_blocks ? src[(int64_t)(b + j) * rec] : 0.f;
        const float s = ((s8[0] + s8[1]) + (s8[2] + s8[3])) + ((s8[4] + s8[5]) + (s8[6] + s8[7]));
        float th = a.r[idx], n = ADAGRAD ? a.Nr[idx] : 0.f;
        fwfm_rule<ADAGRAD>(th, n, s * a.invb, a.regr, a.eta, a.eps);
        a.r[idx] = th;
        a.r[h * F + f] = th;
        if (ADAGRAD) {
            a.Nr[idx] = n;
            a.Nr[h * F + f] = n;
        }
        return;
    }
    if (blockIdx.x == gridDim.x - 1) {
        if (threadIdx.x >= 64) return;
        double s[3] = {0.0, 0.0, 0.0};
        for (int b = threadIdx.x; b < a.n_blocks; b += 64)
#pragma unroll
            for (int i = 0; i < 3; ++i) s[i] += a.bsum[(int64_t)b * 4 + i];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) s[i] += __shfl_xor(s[i], m, 64);
        if (threadIdx.x == 0) {
            if (a.linear) {
                float th = *a.w0, n = ADAGRAD ? *a.N0 : 0.f;
                fwfm_rule<ADAGRAD>(th, n, (float)s[0] * a.invb, a.reg0, a.eta, a.eps);
                *a.w0 = th;
                if (ADAGRAD) *a.N0 = n;
            }
            const double st[4] = {s[0], s[1], (double)a.rows, s[2]};
            for (int i = 0; i < 4; ++i) {
                a.stats[i] = st[i];
                if (a.acc) a.acc[i] = a.acc_reset ? st[i] : a.acc[i] + st[i];
            }
        }
        return;
    }
    const int Q = a.Kp >> 2, stride = Q + kFwfmPartTail / 4;
    const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (idx >= (int64_t)a.n_cols * Q) return;
    const int c = (int)(idx / Q), q = (int)(idx - (int64_t)c * Q);
    const int ch0 = a.chunk0[c], ch1 = a.chunk0[c + 1];
    if (ch1 - ch0 < 2) return;          // (stepped by the backward launch)
    float4 g = f4zero();
    float gw = 0.f;
    for (int ch = ch0; ch < ch1; ++ch) {
        const float4 *rec = reinterpret_cast<const float4 *>(a.part) + (int64_t)ch * stride;
        f4add(g, rec[q]);
        gw += rec[Q].x;
    }
    fwfm_apply<ADAGRAD>(a, a.cfeat[c], Q, q, g, gw);
}

template <int KP, int MT>
hipError_t forward_instance(const FwfmArgs &a, bool train, hipStream_t s) {
    static_assert(fwfm_forward_lds(MT, KP) + 64 * 3 * sizeof(double) <= 65536, "the forward's LDS stays inside 64 KB");
    dim3 g((unsigned)fwfm_forward_blocks(a.rows)), b(kBlock);
    if (train) hipLaunchKernelGGL((k_fwfm_forward<KP, MT, true>), g, b, fwfm_forward_lds(MT, KP), s, a);
    else hipLaunchKernelGGL((k_fwfm_forward<KP, MT, false>), g, b, fwfm_forward_lds(MT, KP), s, a);
    return hipGetLastError();
}

template <int KP>
hipError_t forward_kp(const FwfmArgs &a, bool train, hipStream_t s) {
    switch (a.Fp) {
        case 16: return forward_instance<KP, 1>(a, train, s);
        case 32: return forward_instance<KP, 2>(a, train, s);
        case 48: return forward_instance<KP, 3>(a, train, s);
        case 64: return forward_instance<KP, 4>(a, train, s);
        default: return hipErrorInvalidValue;
    }
}

template <int KP>
void backward_kp(const FwfmArgs &a, bool adagrad, dim3 g, hipStream_t s) {
    if (adagrad) hipLaunchKernelGGL((k_fwfm_backward<KP, true>), g, dim3(kBlock), 0, s, a);
    else hipLaunchKernelGGL((k_fwfm_backward<KP, false>), g, dim3(kBlock), 0, s, a);
}

}  // namespace

hipError_t launch_fwfm_forward(const FwfmArgs &a, bool train, hipStream_t s) {
    if (a.rows <= 0) return hipSuccess;
    if (!a.V || !a.w || !a.w0 || !a.r || !a.row_ptr || !a.yhat || a.F < 1 || a.F > a.Fp) return hipErrorInvalidValue;
    if (train && (!a.y || !a.e || !a.bsum || !a.dz || !a.rpart)) return hipErrorInvalidValue;
    switch (a.Kp) {
        case 4: return forward_kp<4>(a, train, s);
        case 8: return forward_kp<8>(a, train, s);
        case 16: return forward_kp<16>(a, train, s);
        case 32: return forward_kp<32>(a, train, s);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_fwfm_backward(const FwfmArgs &a, bool adagrad, hipStream_t s) {
    if (a.n_chunks <= 0) return hipSuccess;
    if (!a.part || !a.e || !a.dz || !a.chunk_col || !a.occ_row || (adagrad && (!a.NV || !a.Nw))) return hipErrorInvalidValue;
    const int64_t items = (int64_t)a.n_chunks * (a.Kp / 4);
    dim3 g((unsigned)((items + kBlock - 1) / kBlock));
    switch (a.Kp) {
        case 4: backward_kp<4>(a, adagrad, g, s); break;
        case 8: backward_kp<8>(a, adagrad, g, s); break;
        case 16: backward_kp<16>(a, adagrad, g, s); break;
        case 32: backward_kp<32>(a, adagrad, g, s); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_fwfm_update(const FwfmArgs &a, bool adagrad, hipStream_t s) {
    if (!a.stats || !a.bsum || !a.rpart || (adagrad && (!a.NV || !a.Nw || !a.N0 || !a.Nr))) return hipErrorInvalidValue;
    const int64_t items = (int64_t)a.n_cols * (a.Kp / 4);
    dim3 g((unsigned)((items + kBlock - 1) / kBlock + (a.F * a.F + kBlock - 1) / kBlock + 1)), b(kBlock);
    if (adagrad) hipLaunchKernelGGL(k_fwfm_update<true>, g, b, 0, s, a);
    else hipLaunchKernelGGL(k_fwfm_update<false>, g, b, 0, s, a);
    return hipGetLastError();
}

}  // namespace fmhip
