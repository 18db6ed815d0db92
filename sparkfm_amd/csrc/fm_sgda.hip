// fm_sgda.hip — the SGDA learner's kernels (include/fmhip_sgda.h): SGD whose regularisers, one per (feature group, factor), take
// gradient steps on a validation batch.
//   k_sgda_apply            the dense update of fm_apply.hip's k_apply<KP, kRuleSgd> with lambda looked up per row — the same operations
//                           in the same order on a table at scale 1 — which also keeps the parameters it replaces (the shadow tables)
//   k_sgda_lambda_partials  per chunk of the plan: sum of theta_old * h over its rows, h the validation gradient at the new parameters
//   k_sgda_lambda_step      per (group, slot): the chunks' partials added in chunk order in fp64, the step and the clamp
// No atomics: one writer per element, every sum in a fixed order — the result does not depend on the CU count or the schedule.
#include "fm_device.h"
#include "fm_sgda.h"

namespace fmhip {
namespace {

template <int KP>
__global__ __launch_bounds__(kBlock) void k_sgda_apply(SgdaArgs a) {
    constexpr int LPR = KP / 4;  // lanes per feature row (<= 64, divides the wave)
    const float rows = a.scal[2];
    const float invb = rows > 0.f ? 1.0f / rows : 0.f;
    const int64_t total = a.n1 * LPR;
    for (int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * kBlock) {
        const int64_t i = idx / LPR;
        const int c = (int)(idx % LPR);
        const int32_t ga = a.group[i];
        // the row's lanes read the float4 of lambda that matches their slice of V
        const float4 lam = reinterpret_cast<const float4 *>(a.L)[(int64_t)ga * LPR + c];
        float4 *V4 = reinterpret_cast<float4 *>(a.V) + idx;
        float4 *G4 = reinterpret_cast<float4 *>(a.GV) + idx;
        const float b = a.Gb[i];
        const float4 g = *G4, v = *V4;
        float4 u;
        float wslot = 0.f;
        const bool has_w = a.pack_k >= 0 && c == (a.pack_k >> 2);
        if (has_w) {   // packed rows: this float4 holds the linear weight in component pack_k & 3 (and lam its lambda_w)
            const float wi = f4pick(v, a.pack_k & 3), gi = f4pick(g, a.pack_k & 3) * invb;
            wslot = wi - a.eta * fmaf(f4pick(lam, a.pack_k & 3), wi, gi);
        }
        u.x = v.x - a.eta * fmaf(lam.x, v.x, (g.x - v.x * b) * invb);
        u.y = v.y - a.eta * fmaf(lam.y, v.y, (g.y - v.y * b) * invb);
        u.z = v.z - a.eta * fmaf(lam.z, v.z, (g.z - v.z * b) * invb);
        u.w = v.w - a.eta * fmaf(lam.w, v.w, (g.w - v.w * b) * invb);
        if (has_w) f4set(u, a.pack_k & 3, wslot);
        *V4 = u;
        reinterpret_cast<float4 *>(a.SV)[idx] = v;
        *G4 = f4zero();
        if (c == 0) {
            const float wi = a.w[i], gi = a.Gw[i] * invb;
            a.w[i] = wi - a.eta * fmaf(a.Lw[ga], wi, gi);
            a.Sw[i] = wi;
            a.Gw[i] = 0.f;
            a.Gb[i] = 0.f;  // the row's lanes share a wave: they hold their copy of b
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const float w0 = *a.w0;
        *a.w0 = w0 - a.eta * fmaf(a.reg0, w0, a.scal[0] * invb);
    }
}

// One workgroup per chunk; a row slot = LPR lanes, kBlock / LPR of them.  Slot s takes the chunk's rows s, s + slots, ... in that
// order, each lane its float4; the slots' sums are then added in slot order by the first LPR threads.
template <int KP>
__global__ __launch_bounds__(kBlock) void k_sgda_lambda_partials(SgdaArgs a) {
    constexpr int LPR = KP / 4, SLOTS = kBlock / LPR;
    __shared__ float4 sh[kBlock];
    __shared__ float shw[SLOTS];
    const int ch = blockIdx.x;
    const int lo = a.chunk_ptr[ch], hi = a.chunk_ptr[ch + 1];
    const int s = threadIdx.x / LPR, c = threadIdx.x % LPR;
    const bool has_w = a.pack_k >= 0 && c == (a.pack_k >> 2);
    float4 acc = f4zero();
    float accw = 0.f;
    for (int p = lo + s; p < hi; p += SLOTS) {
        const int64_t i = a.order[p];
        float4 *G4 = reinterpret_cast<float4 *>(a.GV) + i * LPR + c;
        const float4 g = *G4;
        const float4 vn = reinterpret_cast<const float4 *>(a.V)[i * LPR + c];
        const float4 vo = reinterpret_cast<const float4 *>(a.SV)[i * LPR + c];
        const float b = a.Gb[i];
        float4 h = make_float4(g.x - vn.x * b, g.y - vn.y * b, g.z - vn.z * b, g.w - vn.w * b);
        if (has_w) f4set(h, a.pack_k & 3, f4pick(g, a.pack_k & 3));     // the linear weight's gradient is the slot itself
        acc.x = fmaf(vo.x, h.x, acc.x);
        acc.y = fmaf(vo.y, h.y, acc.y);
        acc.z = fmaf(vo.z, h.z, acc.z);
        acc.w = fmaf(vo.w, h.w, acc.w);
        *G4 = f4zero();
        if (c == 0) {
            accw = fmaf(a.Sw[i], a.Gw[i], accw);
            a.Gw[i] = 0.f;
            a.Gb[i] = 0.f;  // the row's lanes share a wave: they hold their copy of b
        }
    }
    sh[threadIdx.x] = acc;
    if (c == 0) shw[s] = accw;
    __syncthreads();
    float *out = a.part + (int64_t)ch * (KP + kSgdaPartPad);
    if (threadIdx.x < LPR) {
        float4 t = sh[threadIdx.x];
        for (int j = 1; j < SLOTS; ++j) f4add(t, sh[j * LPR + threadIdx.x]);
        reinterpret_cast<float4 *>(out)[threadIdx.x] = t;
    }
    if (threadIdx.x == 0) {
        float t = shw[0];
        for (int j = 1; j < SLOTS; ++j) t += shw[j];
        reinterpret_cast<float4 *>(out)[LPR] = make_float4(t, 0.f, 0.f, 0.f);
    }
}

// slot < kp: factor slot of L; slot == kp: the w sum of unpacked rows (packed rows carry lambda_w in slot pack_k of L and its copy in Lw)
__global__ __launch_bounds__(kBlock) void k_sgda_lambda_step(SgdaArgs a, int kp) {
    const int width = kp + kSgdaSlots, stride = kp + kSgdaPartPad;
    const float rows = a.scal[2];
    const double invc = rows > 0.f ? 1.0 / (double)rows : 0.0;
    const int total = a.n_groups * width;
    for (int idx = blockIdx.x * kBlock + threadIdx.x; idx < total; idx += gridDim.x * kBlock) {
        const int ga = idx / width, slot = idx % width;
        // chunk order, sixteen loads in flight at a time (one load per add would pay the memory latency once per chunk)
        double sum = 0.0;
        int ch = a.group_chunks[ga];
        const int hi = a.group_chunks[ga + 1];
        for (; ch + 16 <= hi; ch += 16) {
            float t[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) t[j] = a.part[(int64_t)(ch + j) * stride + slot];
#pragma unroll
            for (int j = 0; j < 16; ++j) sum += (double)t[j];
        }
        for (; ch < hi; ++ch) sum += (double)a.part[(int64_t)ch * stride + slot];
        const double S = sum * invc;
        a.S[idx] = S;
        if (slot == kp && a.pack_k >= 0) continue;
        float *lam = slot < kp ? a.L + (int64_t)ga * kp + slot : a.Lw + ga;
        const double next = fma(a.rate, S, (double)*lam);
        const float out = next > 0.0 ? (float)next : 0.f;
        *lam = out;
        if (slot == a.pack_k) a.Lw[ga] = out;
    }
}

}  // namespace

#define FMHIP_SGDA_KP(KERNEL, g, b)                                                     \
    switch (Kp) {                                                                       \
        case 32: hipLaunchKernelGGL((KERNEL<32>), g, b, 0, s, a); break;                \
        case 64: hipLaunchKernelGGL((KERNEL<64>), g, b, 0, s, a); break;                \
        case 128: hipLaunchKernelGGL((KERNEL<128>), g, b, 0, s, a); break;              \
        case 256: hipLaunchKernelGGL((KERNEL<256>), g, b, 0, s, a); break;              \
        default: return hipErrorInvalidValue;                                           \
    }

hipError_t launch_sgda_apply(int Kp, const SgdaArgs &a, hipStream_t s) {
    if (!a.group || !a.L || !a.Lw || !a.SV || !a.Sw) return hipErrorInvalidValue;
    dim3 g((unsigned)grid_blocks(a.n1 * (Kp / 4), kBlock, 8192)), b(kBlock);
    FMHIP_SGDA_KP(k_sgda_apply, g, b);
    return hipGetLastError();
}

hipError_t launch_sgda_lambda_partials(int Kp, const SgdaArgs &a, hipStream_t s) {
    if (a.n_chunks <= 0) return hipSuccess;
    if (!a.order || !a.chunk_ptr || !a.part) return hipErrorInvalidValue;
    dim3 g((unsigned)a.n_chunks), b(kBlock);
    FMHIP_SGDA_KP(k_sgda_lambda_partials, g, b);
    return hipGetLastError();
}
#undef FMHIP_SGDA_KP

hipError_t launch_sgda_lambda_step(int Kp, const SgdaArgs &a, hipStream_t s) {
    if (!a.group_chunks || !a.S || a.n_groups < 1) return hipErrorInvalidValue;
    dim3 g((unsigned)grid_blocks((int64_t)a.n_groups * (Kp + kSgdaSlots), kBlock, 4096)), b(kBlock);
    hipLaunchKernelGGL(k_sgda_lambda_step, g, b, 0, s, a, Kp);
    return hipGetLastError();
}

}  // namespace fmhip
