// fm_ffm.hip — the field-aware FM's kernels (include/fmhip_ffm.h; DESIGN.md, "Field-aware FM"): gfx950, wave64.
//   k_ffm_forward   one wave per data row: the L x L vectors V[i_a][f_b] the row's pairs need go through a compact LDS tile, one
//                   factor quad at a time; lanes take the pairs a < b in a fixed order; also the scorer
//   k_ffm_backward  one wave per (column, chunk of 256 occurrences): the occurrences in order, per occurrence lane b = entry b of the
//                   row, run heads add into the wave's LDS accumulator acc[f_b][Kp]; one partial record per chunk.  Writes no parameter
//   k_ffm_update    per column present: the chunks' partials in chunk order, the rule on the touched (i, f) vectors and on w[i]; one
//                   more workgroup sums the forward's block partials and steps w0
// No atomics: one writer per element, every sum in an order the data fixes — the result does not depend on the CU count or the schedule.
// The pair products' operands are each used once (T[a][b] meets T[b][a] and nothing else): there is no matrix to reuse, so no MFMA.
#include "fm_device.h"
#include "fm_ffm.h"
#include "fm_finish.h"      // pair_sigma_residual

namespace fmhip {
namespace {

// LDS written by some lanes of a wave, read by others of the same wave
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// The workgroup is `waves` waves (1, 2 or 4: what fits 64 KB of tiles at the batch's longest row); wave w takes the rows w, w + waves,
// ... of the workgroup's kFfmRowsPerBlock.  The tile of a row of L entries is T[a * L + b] = V[i_a][f_b][4c .. 4c + 3]: the row's
// entries are sorted by (field, feature), so a walks the gathered feature rows and b ascends inside each.  A tile is its wave's
// own: the waves of a workgroup share nothing but the statistics partial at the end, and wait for each other only there.
template <bool TRAIN>
__global__ __launch_bounds__(kBlock) void k_ffm_forward(FfmArgs a) {
    extern __shared__ float4 ffm_tile[];
    __shared__ double sh[kBlock / 64][3];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, waves = blockDim.x >> 6;
    const int Q = a.Kp >> 2;
    float4 *T = ffm_tile + (size_t)wave * a.max_len * a.max_len;
    const float4 *V4 = reinterpret_cast<const float4 *>(a.V);
    const float w0 = *a.w0;
    double se = 0.0, sse = 0.0, nf = 0.0;
    for (int j = wave; j < kFfmRowsPerBlock; j += waves) {
        const int64_t r = (int64_t)blockIdx.x * kFfmRowsPerBlock + j;
        const bool valid = r < a.rows;
        const int64_t base = valid ? a.row_ptr[r] : 0;
        const int L = valid ? (int)(a.row_ptr[r + 1] - base) : 0, LL = L * L;
        const bool in = lane < L;
        const int ci = in ? a.col[base + lane] : 0, fi = in ? a.fld[base + lane] : 0;
        const float xi = in ? a.val[base + lane] : 0.f;
        float pair = 0.f;
        for (int c = 0; c < Q; ++c) {
            wave_lds_sync();      // the previous quad's reads of the tile are over
            for (int i0 = 0; i0 < LL; i0 += 64) {
                const int idx = i0 + lane;
                const bool ok = idx < LL;
                const int ia = ok ? idx / L : 0, ib = ok ? idx - ia * L : 0;
                const int i_a = __shfl(ci, ia, 64), f_b = __shfl(fi, ib, 64);      // (every lane takes part in the shuffles)
                if (ok && ia != ib) T[idx] = V4[((int64_t)i_a * a.F + f_b) * Q + c];
            }
            wave_lds_sync();
            for (int i0 = 0; i0 < LL; i0 += 64) {
                const int idx = i0 + lane;
                const bool ok = idx < LL;
                const int ia = ok ? idx / L : 0, ib = ok ? idx - ia * L : 0;
                const float xa = __shfl(xi, ia, 64), xb = __shfl(xi, ib, 64);
                if (ok && ia < ib) pair = fmaf(xa * xb, f4dot(T[idx], T[ib * L + ia]), pair);
            }
        }
        const float lin = wave_sum(in ? a.w[ci] * xi : 0.f);
        const float yh = (w0 + lin) + wave_sum(pair);
        if (lane == 0 && valid) {
            a.yhat[r] = yh;
            if (TRAIN) {
                float z;
                const float e = a.loss == kLossLogistic ? pair_sigma_residual(yh, a.y[r] > 0.f, z) : yh - a.y[r];
                a.e[r] = e;
                se += (double)e;
                sse += (double)e * (double)e;
                nf += isfinite(yh) ? 0.0 : 1.0;
            }
        }
    }
    if (TRAIN) {
        if (lane == 0) {
            sh[wave][0] = se;
            sh[wave][1] = sse;
            sh[wave][2] = nf;
        }
        __syncthreads();
        if (threadIdx.x < 3) {
            double t = sh[0][threadIdx.x];
            for (int v = 1; v < waves; ++v) t += sh[v][threadIdx.x];
            a.bsum[(int64_t)blockIdx.x * 4 + threadIdx.x] = t;
        }
        if (threadIdx.x == 3) a.bsum[(int64_t)blockIdx.x * 4 + 3] = 0.0;
    }
}

// Four waves a workgroup, each with a chunk and F * KP floats of LDS of its own (no workgroup barrier: a wave without a chunk leaves).
// Per occurrence (r, a) lane b holds entry b of row r; the head of a same-field run adds e_r x_a x_t V[i_t][f_a] for the t of its run
// (t != a, ascending) into acc[f_b] — one lane per accumulator and occurrence, the occurrences one after the other.
template <int KP>
__global__ __launch_bounds__(kBlock) void k_ffm_backward(FfmArgs a) {
    extern __shared__ float ffm_acc[];
    constexpr int Q = KP / 4;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ch = blockIdx.x * (kBlock / 64) + wave;
    if (ch >= a.n_chunks) return;
    const int width = a.F * KP;
    float *acc = ffm_acc + (size_t)wave * width;
    for (int i = lane; i < width; i += 64) acc[i] = 0.f;
    wave_lds_sync();
    const int c = a.chunk_col[ch];
    const int lo = a.cptr[c] + kFfmChunkLen * (ch - a.chunk0[c]);
    const int hi = min(lo + kFfmChunkLen, a.cptr[c + 1]);
    const float4 *V4 = reinterpret_cast<const float4 *>(a.V);
    uint64_t mask = 0;
    float wsum = 0.f;
    for (int o = lo; o < hi; ++o) {
        const int r = a.occ_row[o], pa = a.occ_pos[o];
        const int64_t base = a.row_ptr[r];
        const int L = (int)(a.row_ptr[r + 1] - base);
        const float s = a.e[r] * a.val[base + pa];
        const int f_a = a.fld[base + pa];
        wsum += s;
        const bool in = lane < L;
        const int rb = in ? a.run[base + lane] : 0;
        if (rb > 0) {
            const int fb = a.fld[base + lane];
            float4 *dst = reinterpret_cast<float4 *>(acc + fb * KP);
            bool any = false;
            for (int j = 0; j < rb; ++j) {
                const int t = lane + j;
                if (t == pa) continue;
                any = true;
                const float coef = s * a.val[base + t];
                const float4 *src = V4 + ((int64_t)a.col[base + t] * a.F + f_a) * Q;
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    float4 d = dst[q];
                    f4fma(d, src[q], coef);
                    dst[q] = d;
                }
            }
            if (any) mask |= 1ull << fb;
        }
        wave_lds_sync();
    }
    uint32_t mlo = (uint32_t)mask, mhi = (uint32_t)(mask >> 32);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        mlo |= (uint32_t)__shfl_xor((int)mlo, m, 64);
        mhi |= (uint32_t)__shfl_xor((int)mhi, m, 64);
    }
    float *out = a.part + (int64_t)ch * (width + kFfmPartTail);
    for (int i = lane; i < width / 4; i += 64) reinterpret_cast<float4 *>(out)[i] = reinterpret_cast<const float4 *>(acc)[i];
    if (lane == 0) reinterpret_cast<float4 *>(out)[width / 4] = make_float4(__uint_as_float(mlo), __uint_as_float(mhi), wsum, 0.f);
}

// one parameter's step on g_hat = g + reg * theta (g: the batch's mean gradient); n: its AdaGrad accumulator, untouched under SGD
template <bool ADAGRAD>
__device__ __forceinline__ void ffm_rule(float &th, float &n, float g, float reg, float eta, float eps) {
    const float gh = fmaf(reg, th, g);
    if (ADAGRAD) adagrad_step(th, n, gh, eta, eps);
    else th = th - eta * gh;
}

// A thread per (column, float4 of the feature's row); the last workgroup is w0's: its first wave adds the forward's block partials —
// lane l those of the blocks l, l + 64, ... in that order, then a fixed tree — steps w0 and leaves the step's statistics.
template <bool ADAGRAD>
__global__ __launch_bounds__(kBlock) void k_ffm_update(FfmArgs a) {
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
                ffm_rule<ADAGRAD>(th, n, (float)s[0] * a.invb, a.reg0, a.eta, a.eps);
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
    const int Q = a.Kp >> 2, per = a.F * Q;
    const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (idx >= (int64_t)a.n_cols * per) return;
    const int c = (int)(idx / per), slot = (int)(idx - (int64_t)c * per), f = slot / Q;
    const int stride = a.F * a.Kp + kFfmPartTail;
    float4 g = f4zero();
    float gw = 0.f;
    uint32_t bits = 0;
    for (int ch = a.chunk0[c]; ch < a.chunk0[c + 1]; ++ch) {
        const float *rec = a.part + (int64_t)ch * stride;
        f4add(g, reinterpret_cast<const float4 *>(rec)[slot]);
        bits |= __float_as_uint(rec[a.F * a.Kp + (f >> 5)]);
        if (slot == 0) gw += rec[a.F * a.Kp + 2];
    }
    const int64_t i = a.cfeat[c];
    if ((bits >> (f & 31)) & 1u) {
        const int64_t at = i * per + slot;
        float4 v = reinterpret_cast<float4 *>(a.V)[at];
        float4 n = ADAGRAD ? reinterpret_cast<float4 *>(a.NV)[at] : f4zero();
        ffm_rule<ADAGRAD>(v.x, n.x, g.x * a.invb, a.regv, a.eta, a.eps);
        ffm_rule<ADAGRAD>(v.y, n.y, g.y * a.invb, a.regv, a.eta, a.eps);
        ffm_rule<ADAGRAD>(v.z, n.z, g.z * a.invb, a.regv, a.eta, a.eps);
        ffm_rule<ADAGRAD>(v.w, n.w, g.w * a.invb, a.regv, a.eta, a.eps);
        reinterpret_cast<float4 *>(a.V)[at] = v;
        if (ADAGRAD) reinterpret_cast<float4 *>(a.NV)[at] = n;
    }
    if (slot == 0 && a.linear) {
        float th = a.w[i], n = ADAGRAD ? a.Nw[i] : 0.f;
        ffm_rule<ADAGRAD>(th, n, gw * a.invb, a.regw, a.eta, a.eps);
        a.w[i] = th;
        if (ADAGRAD) a.Nw[i] = n;
    }
}

}  // namespace

hipError_t launch_ffm_forward(const FfmArgs &a, bool train, hipStream_t s) {
    if (a.rows <= 0) return hipSuccess;
    if (!a.V || !a.w || !a.w0 || !a.row_ptr || !a.yhat || a.max_len < 0 || a.max_len > 64) return hipErrorInvalidValue;
    if (train && (!a.y || !a.e || !a.bsum)) return hipErrorInvalidValue;
    const size_t tile = (size_t)a.max_len * a.max_len * sizeof(float4);
    const int waves = tile * 4 <= 65536 ? 4 : (tile * 2 <= 65536 ? 2 : 1);
    const size_t lds = tile * waves > 16 ? tile * waves : 16;
    dim3 g((unsigned)ffm_forward_blocks(a.rows)), b((unsigned)(64 * waves));
    if (train) hipLaunchKernelGGL(k_ffm_forward<true>, g, b, lds, s, a);
    else hipLaunchKernelGGL(k_ffm_forward<false>, g, b, lds, s, a);
    return hipGetLastError();
}

hipError_t launch_ffm_backward(const FfmArgs &a, hipStream_t s) {
    if (a.n_chunks <= 0) return hipSuccess;
    if (!a.part || !a.e || !a.chunk_col || !a.occ_row) return hipErrorInvalidValue;
    dim3 g((unsigned)((a.n_chunks + kBlock / 64 - 1) / (kBlock / 64))), b(kBlock);
    const size_t lds = (size_t)(kBlock / 64) * a.F * a.Kp * sizeof(float);
    switch (a.Kp) {
        case 4: hipLaunchKernelGGL(k_ffm_backward<4>, g, b, lds, s, a); break;
        case 8: hipLaunchKernelGGL(k_ffm_backward<8>, g, b, lds, s, a); break;
        case 16: hipLaunchKernelGGL(k_ffm_backward<16>, g, b, lds, s, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_ffm_update(const FfmArgs &a, bool adagrad, hipStream_t s) {
    if (!a.stats || !a.bsum || (adagrad && (!a.NV || !a.Nw || !a.N0))) return hipErrorInvalidValue;
    const int64_t items = (int64_t)a.n_cols * a.F * (a.Kp / 4);
    dim3 g((unsigned)((items + kBlock - 1) / kBlock + 1)), b(kBlock);
    if (adagrad) hipLaunchKernelGGL(k_ffm_update<true>, g, b, 0, s, a);
    else hipLaunchKernelGGL(k_ffm_update<false>, g, b, 0, s, a);
    return hipGetLastError();
}

}  // namespace fmhip
