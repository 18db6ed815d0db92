// fm_bpr.hip — the BPR trainer's device work (fm_bpr.h): k_bpr_sample draws a negative row per pair, and the k_bpr_inv_* kernels
// around one rocPRIM radix sort and two scans rebuild the candidates relation's inverse map of a batch.  Integer arithmetic only;
// every address has one writer and nothing depends on the launch shape.  k_bpr_sample_adaptive (include/fmhip_bpr_adaptive.h) draws
// several candidates per pair with the same integer code and keeps the one the model scores highest: the one place with fp32 in it,
// a dot product whose summation order the row width alone fixes.  k_bpr_sample_warp (include/fmhip_warp.h) scores the same candidates
// the same way and keeps the first one that violates the margin against the pair's positive, with the pair's rank weight beside it.
#include "fm_bpr.h"
#include "fm_device.h"      // f4dot; grid_blocks (fm_kernels.h)
#include "mcmc_rng.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

namespace fmhip {
namespace {

constexpr int kT = 256;
using u64 = unsigned long long;

inline unsigned blocks_of(int64_t n) { return (unsigned)((n + kT - 1) / kT); }

// the block's sums of N counters: an xor-shuffle inside every wave, one LDS word per wave, thread i < N adds counter i's words
// in wave order and writes out[i]
template <int N>
__device__ __forceinline__ void block_sums_u64(u64 (&v)[N], u64 *out) {
    __shared__ u64 sh[N][kT / 64];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] += __shfl_xor(v[i], m, 64);
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int i = 0; i < N; ++i) sh[i][threadIdx.x >> 6] = v[i];
    __syncthreads();
    if (threadIdx.x < N) {
        u64 s = 0;
        for (int w = 0; w < kT / 64; ++w) s += sh[threadIdx.x][w];
        out[threadIdx.x] = s;
    }
}

__global__ __launch_bounds__(kT) void k_bpr_sample(BprSampleArgs a) {
    u64 att = 0, forced = 0;
    for (int64_t p = (int64_t)blockIdx.x * kT + threadIdx.x; p < a.n_pairs; p += (int64_t)gridDim.x * kT) {
        const int32_t u = a.ictx[p / a.n_neg];
        const int64_t lo = a.pptr[u];
        int at = 0, f = 0;
        a.map[2 * p + 1] = rng::negative_row(a.seed, (uint32_t)p, a.t, (uint32_t)a.M, a.prow + lo, (int32_t)(a.pptr[u + 1] - lo), &at, &f);
        att += (u64)at;
        forced += (u64)f;
    }
    u64 v[2] = {att, forced};
    block_sums_u64<2>(v, a.part + 2 * (size_t)blockIdx.x);
}

// one block: the sums of the per-block partials of N counters each (integers: any order gives the same)
template <int N>
__global__ __launch_bounds__(kT) void k_bpr_total(const u64 *part, int n_blocks, u64 *total) {
    u64 s[N] = {};
    for (int b = threadIdx.x; b < n_blocks; b += kT)
#pragma unroll
        for (int i = 0; i < N; ++i) s[i] += part[N * (size_t)b + i];
    block_sums_u64<N>(s, total);
}

// ---- the adaptive sampler (fm_bpr.h: BprAdaptiveArgs) -----------------------------------------------------------------------------

constexpr int kCandChunk = 4;       // candidate rows a group has in flight before it reduces: the gathers' latency overlaps

// G lanes per pair, kT / G pairs per block and pass.  The trip count is the block's (`base` is uniform), and a group whose pair lies
// past the end works on the last pair again and writes nothing: no lane leaves before the block's last shuffle.  A score is
// yq_i + (the lanes' 4-term fmaf chains summed by the xor tree over G): the same in every lane of the group, whatever the grid.
template <int G, bool RECORD>
__global__ __launch_bounds__(kT) void k_bpr_sample_adaptive(BprAdaptiveArgs a) {
    constexpr int KP = 4 * G, GPB = kT / G;
    const int l = threadIdx.x & (G - 1), grp = threadIdx.x / G;
    const int64_t first = RECORD ? a.p0 : 0, end = RECORD ? a.p1 : a.s.n_pairs;
    const int C = a.n_cand;
    u64 att = 0, forced = 0, repl = 0;
    for (int64_t base = first + (int64_t)blockIdx.x * GPB; base < end; base += (int64_t)gridDim.x * GPB) {
        const bool live = base + grp < end;
        const int64_t p = live ? base + grp : end - 1;
        const int32_t u = a.s.ictx[p / a.s.n_neg];
        const int64_t lo = a.s.pptr[u];
        const int32_t len = (int32_t)(a.s.pptr[u + 1] - lo);
        float4 qu = reinterpret_cast<const float4 *>(a.Qu + (size_t)u * KP)[l];
        if (4 * l + 0 >= a.k) qu.x = 0.f;      // the packed slot and the padding are no factors
        if (4 * l + 1 >= a.k) qu.y = 0.f;
        if (4 * l + 2 >= a.k) qu.z = 0.f;
        if (4 * l + 3 >= a.k) qu.w = 0.f;
        int32_t keep = 0, keep_c = 0;
        float best = 0.f;
        for (int c0 = 0; c0 < C; c0 += G) {
            // the group's lanes draw candidates c0 .. c0 + G - 1 side by side
            int32_t mine = 0;
            if (c0 + l < C) {
                int at = 0, f = 0;
                mine = rng::negative_row(a.s.seed, (uint32_t)p, a.s.t, (uint32_t)a.s.M, a.s.prow + lo, len, &at, &f, (uint32_t)(c0 + l) << 4);
                if (live) {
                    att += (u64)at;
                    forced += (u64)f;
                }
            }
            const int n = C - c0 < G ? C - c0 : G;
            for (int j0 = 0; j0 < n; j0 += kCandChunk) {
                int32_t row[kCandChunk];
                float4 qi[kCandChunk];
                float yq[kCandChunk], d[kCandChunk];
#pragma unroll
                for (int jj = 0; jj < kCandChunk; ++jj) {
                    const int j = j0 + jj < n ? j0 + jj : n - 1;       // (past the last candidate: the last one again, not compared)
                    row[jj] = __shfl(mine, j, G);
                    qi[jj] = reinterpret_cast<const float4 *>(a.Qi + (size_t)row[jj] * KP)[l];
                    yq[jj] = a.yqi[row[jj]];
                }
#pragma unroll
                for (int jj = 0; jj < kCandChunk; ++jj) d[jj] = f4dot(qu, qi[jj]);
#pragma unroll
                for (int m = G >> 1; m >= 1; m >>= 1)
#pragma unroll
                    for (int jj = 0; jj < kCandChunk; ++jj) d[jj] += __shfl_xor(d[jj], m, G);
#pragma unroll
                for (int jj = 0; jj < kCandChunk; ++jj) {
                    const int c = c0 + j0 + jj;
                    if (j0 + jj >= n) break;
                    const float s = yq[jj] + d[jj];
                    if (RECORD && live && l == 0) {
                        const size_t at = (size_t)(p - a.p0) * (size_t)C + (size_t)c;
                        a.rec_rows[at] = row[jj];
                        a.rec_scores[at] = s;
                    }
                    if (c == 0 || s > best) {      // candidate 0 is the incumbent; a NaN is never greater
                        best = s;
                        keep = row[jj];
                        keep_c = c;
                    }
                }
            }
        }
        if (!RECORD && live && l == 0) {
            a.s.map[2 * p + 1] = keep;
            repl += keep_c != 0 ? 1u : 0u;
        }
    }
    if (RECORD) return;
    u64 v[3] = {att, forced, repl};
    block_sums_u64<3>(v, a.s.part + 3 * (size_t)blockIdx.x);
}

template <int G>
hipError_t launch_adaptive(const BprAdaptiveArgs &a, hipStream_t s) {
    const bool record = a.rec_rows != nullptr;
    const int64_t n = record ? (int64_t)a.p1 - a.p0 : a.s.n_pairs;
    const int blocks = bpr_adaptive_blocks(4 * G, n);
    if (record) {
        hipLaunchKernelGGL((k_bpr_sample_adaptive<G, true>), dim3((unsigned)blocks), dim3(kT), 0, s, a);
        return hipGetLastError();
    }
    hipLaunchKernelGGL((k_bpr_sample_adaptive<G, false>), dim3((unsigned)blocks), dim3(kT), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_bpr_total<3>, dim3(1), dim3(kT), 0, s, a.s.part, blocks, a.s.total);
    return hipGetLastError();
}

// ---- the WARP sampler (fm_bpr.h: BprWarpArgs) ---------------------------------------------------------------------------------------

// The adaptive kernel's lane layout, draws and score order.  The positive's row is gathered and scored first, by the code that
// scores a candidate; a candidate violates iff its score is strictly above thr (false for a NaN on either side).  Every lane of a
// group holds the same scores, so `n_first` and the early exit are uniform over the group: a group that leaves the candidate loops
// leaves whole, and the width-G shuffles of the groups still in them read only their own lanes.
template <int G, bool RECORD>
__global__ __launch_bounds__(kT) void k_bpr_sample_warp(BprWarpArgs w) {
    constexpr int KP = 4 * G, GPB = kT / G;
    const BprAdaptiveArgs &a = w.a;
    const int l = threadIdx.x & (G - 1), grp = threadIdx.x / G;
    const int64_t first = RECORD ? a.p0 : 0, end = RECORD ? a.p1 : a.s.n_pairs;
    const int C = a.n_cand;
    u64 violated = 0, trials = 0;
    for (int64_t base = first + (int64_t)blockIdx.x * GPB; base < end; base += (int64_t)gridDim.x * GPB) {
        const bool live = base + grp < end;
        const int64_t p = live ? base + grp : end - 1;
        const int32_t u = a.s.ictx[p / a.s.n_neg];
        const int64_t lo = a.s.pptr[u];
        const int32_t len = (int32_t)(a.s.pptr[u + 1] - lo);
        float4 qu = reinterpret_cast<const float4 *>(a.Qu + (size_t)u * KP)[l];
        if (4 * l + 0 >= a.k) qu.x = 0.f;      // the packed slot and the padding are no factors
        if (4 * l + 1 >= a.k) qu.y = 0.f;
        if (4 * l + 2 >= a.k) qu.z = 0.f;
        if (4 * l + 3 >= a.k) qu.w = 0.f;
        float thr;
        {
            const int32_t ipos = a.s.map[2 * p];      // (the positive: no sampler writes the even entries)
            const float4 qp = reinterpret_cast<const float4 *>(a.Qi + (size_t)ipos * KP)[l];
            const float yp = a.yqi[ipos];
            float dp = f4dot(qu, qp);
#pragma unroll
            for (int m = G >> 1; m >= 1; m >>= 1) dp += __shfl_xor(dp, m, G);
            const float spos = yp + dp;
            if (RECORD && live && l == 0) w.rec_pos[p - a.p0] = spos;
            thr = spos - w.margin;
        }
        int32_t keep = 0, n_first = 0;
        for (int c0 = 0; c0 < C && (RECORD || n_first == 0); c0 += G) {
            // the group's lanes draw candidates c0 .. c0 + G - 1 side by side
            int32_t mine = 0;
            if (c0 + l < C) {
                int at = 0, f = 0;
                mine = rng::negative_row(a.s.seed, (uint32_t)p, a.s.t, (uint32_t)a.s.M, a.s.prow + lo, len, &at, &f, (uint32_t)(c0 + l) << 4);
            }
            const int n = C - c0 < G ? C - c0 : G;
            for (int j0 = 0; j0 < n && (RECORD || n_first == 0); j0 += kCandChunk) {
                int32_t row[kCandChunk];
                float4 qi[kCandChunk];
                float yq[kCandChunk], d[kCandChunk];
#pragma unroll
                for (int jj = 0; jj < kCandChunk; ++jj) {
                    const int j = j0 + jj < n ? j0 + jj : n - 1;       // (past the last candidate: the last one again, not compared)
                    row[jj] = __shfl(mine, j, G);
                    qi[jj] = reinterpret_cast<const float4 *>(a.Qi + (size_t)row[jj] * KP)[l];
                    yq[jj] = a.yqi[row[jj]];
                }
#pragma unroll
                for (int jj = 0; jj < kCandChunk; ++jj) d[jj] = f4dot(qu, qi[jj]);
#pragma unroll
                for (int m = G >> 1; m >= 1; m >>= 1)
#pragma unroll
                    for (int jj = 0; jj < kCandChunk; ++jj) d[jj] += __shfl_xor(d[jj], m, G);
#pragma unroll
                for (int jj = 0; jj < kCandChunk; ++jj) {
                    const int c = c0 + j0 + jj;
                    if (j0 + jj >= n) break;
                    const float s = yq[jj] + d[jj];
                    if (RECORD && live && l == 0) {
                        const size_t at = (size_t)(p - a.p0) * (size_t)C + (size_t)c;
                        a.rec_rows[at] = row[jj];
                        a.rec_scores[at] = s;
                    }
                    if (c == 0) keep = row[jj];                        // no violator: candidate 0's row
                    if (n_first == 0 && s > thr) {                     // the first violator; a NaN is never greater
                        n_first = c + 1;
                        keep = row[jj];
                    }
                }
            }
        }
        if (!RECORD && live && l == 0) {
            a.s.map[2 * p + 1] = keep;
            const float cw = w.W[n_first];
            reinterpret_cast<float2 *>(w.c)[p] = make_float2(cw, cw);
            w.trials[p] = n_first;
            violated += n_first != 0 ? 1u : 0u;
            trials += (u64)n_first;
        }
    }
    if (RECORD) return;
    u64 v[2] = {violated, trials};
    block_sums_u64<2>(v, a.s.part + 2 * (size_t)blockIdx.x);
}

template <int G>
hipError_t launch_warp(const BprWarpArgs &w, hipStream_t s) {
    const bool record = w.a.rec_rows != nullptr;
    const int64_t n = record ? (int64_t)w.a.p1 - w.a.p0 : w.a.s.n_pairs;
    const int blocks = bpr_adaptive_blocks(4 * G, n);
    if (record) {
        hipLaunchKernelGGL((k_bpr_sample_warp<G, true>), dim3((unsigned)blocks), dim3(kT), 0, s, w);
        return hipGetLastError();
    }
    hipLaunchKernelGGL((k_bpr_sample_warp<G, false>), dim3((unsigned)blocks), dim3(kT), 0, s, w);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_bpr_total<2>, dim3(1), dim3(kT), 0, s, w.a.s.part, blocks, w.a.s.total);
    return hipGetLastError();
}

// ---- the inverse map --------------------------------------------------------------------------------------------------------------

// bits that hold every value of [0, n): at least 1
inline int bits_for(int64_t n) {
    int b = 1;
    while (((int64_t)1 << b) < n) ++b;
    return b;
}

// per touched list: work items, partial rows, long lists
struct Tri { int32_t w, p, l; };
struct TriPlus {
    __host__ __device__ Tri operator()(const Tri &x, const Tri &y) const { return Tri{x.w + y.w, x.p + y.p, x.l + y.l}; }
};

__global__ __launch_bounds__(kT) void k_bpr_inv_keys(const int32_t *map, int32_t rows, int rbits, u64 *key) {
    const int64_t i64 = (int64_t)blockIdx.x * kT + threadIdx.x;      // (64-bit: the grid's last block may reach past 2^31)
    const int32_t i = (int32_t)i64;
    if (i64 < rows) key[i] = ((u64)(uint32_t)map[i] << rbits) | (u64)(uint32_t)i;
}

// sorted words -> trow, and the flag of every position that starts a list
__global__ __launch_bounds__(kT) void k_bpr_inv_heads(const u64 *key, int32_t rows, int rbits, int32_t *trow, int32_t *head) {
    const int64_t i64 = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (i64 >= rows) return;
    const int32_t i = (int32_t)i64;
    const u64 w = key[i];
    trow[i] = (int32_t)(w & (((u64)1 << rbits) - 1));
    head[i] = i == 0 || (key[i - 1] >> rbits) != (w >> rbits) ? 1 : 0;
}

// tinc: the inclusive scan of the flags.  A head writes its list's block row and start; the last position closes tptr and counts the lists
__global__ __launch_bounds__(kT) void k_bpr_inv_touch(const u64 *key, const int32_t *head, const int32_t *tinc, int32_t rows, int rbits, int32_t *tj,
                                                      int32_t *tptr, int32_t *counts) {
    const int64_t i64 = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (i64 >= rows) return;
    const int32_t i = (int32_t)i64;
    const int32_t t = tinc[i] - 1;
    if (head[i]) {
        tj[t] = (int32_t)(key[i] >> rbits);
        tptr[t] = i;
    }
    if (i == rows - 1) {
        tptr[t + 1] = rows;
        counts[0] = t + 1;
    }
}

// per list (threads past the last list: zeros): what it adds to the work list
__global__ __launch_bounds__(kT) void k_bpr_inv_count(const int32_t *tptr, const int32_t *counts, int32_t rows, int32_t cut, Tri *tri) {
    const int64_t t64 = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (t64 >= rows) return;
    const int32_t t = (int32_t)t64;
    Tri v{0, 0, 0};
    if (t < counts[0]) {
        const int32_t len = tptr[t + 1] - tptr[t];
        if (len <= cut) v.w = 1;
        else v = Tri{(len + cut - 1) / cut, (len + cut - 1) / cut, 1};
    }
    tri[t] = v;
}

// trix: the exclusive scan of tri.  A list of up to `cut` rows is one item that writes its block row; a longer one is cut into
// chunks that write partial rows, plus one entry of the second pass (RelationInverse::append_batch)
__global__ __launch_bounds__(kT) void k_bpr_inv_fill(BprInverseArgs a, const Tri *tri, const Tri *trix) {
    const int64_t t64 = (int64_t)blockIdx.x * kT + threadIdx.x;
    const int32_t n_t = a.counts[0];
    if (t64 >= a.rows || t64 >= n_t) return;
    const int32_t t = (int32_t)t64;
    const Tri own = tri[t], at = trix[t];
    const int32_t beg = a.tptr[t];
    if (own.l == 0) {
        a.wt[at.w] = t;
        a.wbeg[at.w] = beg;
        a.wdst[at.w] = a.tj[t];
    } else {
        a.lt[at.l] = t;
        a.lfirst[at.l] = at.p;
        a.lcount[at.l] = own.p;
        for (int32_t c = 0; c < own.w; ++c) {
            a.wt[at.w + c] = t;
            a.wbeg[at.w + c] = beg + c * a.cut;
            a.wdst[at.w + c] = -1 - (at.p + c);
        }
    }
    if (t == n_t - 1) {
        a.counts[1] = at.w + own.w;
        a.counts[2] = at.l + own.l;
        a.counts[3] = at.p + own.p;
    }
}

struct InvLayout {
    size_t key = 0, sorted = 0, head = 0, tinc = 0, tri = 0, trix = 0, tmp = 0, tmp_bytes = 0, total = 0;
};

#define BPR_TRY(expr)                    \
    do {                                 \
        hipError_t _e = (expr);          \
        if (_e != hipSuccess) return _e; \
    } while (0)

hipError_t inv_layout(int32_t rows, int32_t block_rows, InvLayout *L) {
    if (rows < 1 || block_rows < 1) return hipErrorInvalidValue;
    const size_t N = (size_t)rows;
    const int end_bit = bits_for(rows) + bits_for(block_rows);
    size_t t = 0, tb = 0;
    BPR_TRY(rocprim::radix_sort_keys(nullptr, t, (u64 *)nullptr, (u64 *)nullptr, N, 0u, (unsigned)end_bit, (hipStream_t) nullptr));
    tb = t > tb ? t : tb;
    BPR_TRY(rocprim::inclusive_scan(nullptr, t, (int32_t *)nullptr, (int32_t *)nullptr, N, rocprim::plus<int32_t>(), (hipStream_t) nullptr));
    tb = t > tb ? t : tb;
    BPR_TRY(rocprim::exclusive_scan(nullptr, t, (Tri *)nullptr, (Tri *)nullptr, Tri{0, 0, 0}, N, TriPlus(), (hipStream_t) nullptr));
    tb = t > tb ? t : tb;
    size_t off = 0;
    const auto take = [&off](size_t bytes) {
        const size_t at = off;
        off += (bytes + 255) / 256 * 256;
        return at;
    };
    L->key = take(N * sizeof(u64));
    L->sorted = take(N * sizeof(u64));
    L->head = take(N * sizeof(int32_t));
    L->tinc = take(N * sizeof(int32_t));
    L->tri = take(N * sizeof(Tri));
    L->trix = take(N * sizeof(Tri));
    L->tmp = take(tb);
    L->tmp_bytes = tb;
    L->total = off;
    return hipSuccess;
}

}  // namespace

int bpr_sample_blocks(int64_t n_pairs) { return grid_blocks(n_pairs, kT, 4096); }

hipError_t launch_bpr_sample(const BprSampleArgs &a, hipStream_t s) {
    const int blocks = bpr_sample_blocks(a.n_pairs);
    hipLaunchKernelGGL(k_bpr_sample, dim3((unsigned)blocks), dim3(kT), 0, s, a);
    BPR_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_bpr_total<2>, dim3(1), dim3(kT), 0, s, a.part, blocks, a.total);
    return hipGetLastError();
}

int bpr_adaptive_blocks(int Kp, int64_t n_pairs) { return grid_blocks(n_pairs, kT / (Kp / 4), 4096); }      // a group of Kp / 4 lanes per pair

hipError_t launch_bpr_sample_adaptive(int Kp, const BprAdaptiveArgs &a, hipStream_t s) {
    if (a.n_cand < 1 || a.n_cand > kBprMaxCand || a.k < 0 || a.k > Kp) return hipErrorInvalidValue;
    if (a.rec_rows && (!a.rec_scores || a.p0 < 0 || a.p1 > a.s.n_pairs || a.p0 >= a.p1)) return hipErrorInvalidValue;
    switch (Kp) {
        case 32: return launch_adaptive<8>(a, s);
        case 64: return launch_adaptive<16>(a, s);
        case 128: return launch_adaptive<32>(a, s);
        case 256: return launch_adaptive<64>(a, s);
        default: return hipErrorInvalidValue;      // (padded_factors: a power of two in [32, 256])
    }
}

hipError_t launch_bpr_sample_warp(int Kp, const BprWarpArgs &w, hipStream_t s) {
    const BprAdaptiveArgs &a = w.a;
    if (a.n_cand < 1 || a.n_cand > kBprMaxCand || a.k < 0 || a.k > Kp || !(w.margin >= 0.f)) return hipErrorInvalidValue;
    if (a.rec_rows) {
        if (!a.rec_scores || !w.rec_pos || a.p0 < 0 || a.p1 > a.s.n_pairs || a.p0 >= a.p1) return hipErrorInvalidValue;
    } else if (!w.W || !w.c || !w.trials) return hipErrorInvalidValue;
    switch (Kp) {
        case 32: return launch_warp<8>(w, s);
        case 64: return launch_warp<16>(w, s);
        case 128: return launch_warp<32>(w, s);
        case 256: return launch_warp<64>(w, s);
        default: return hipErrorInvalidValue;      // (padded_factors: a power of two in [32, 256])
    }
}

hipError_t bpr_inverse_workspace(int32_t rows, int32_t block_rows, size_t *bytes) {
    InvLayout L;
    BPR_TRY(inv_layout(rows, block_rows, &L));
    *bytes = L.total;
    return hipSuccess;
}

hipError_t launch_bpr_inverse(const BprInverseArgs &a, void *workspace, size_t bytes, hipStream_t s) {
    InvLayout L;
    BPR_TRY(inv_layout(a.rows, a.block_rows, &L));
    if (!workspace || bytes < L.total || a.cut < 1) return hipErrorInvalidValue;
    char *base = static_cast<char *>(workspace);
    u64 *key = reinterpret_cast<u64 *>(base + L.key), *sorted = reinterpret_cast<u64 *>(base + L.sorted);
    int32_t *head = reinterpret_cast<int32_t *>(base + L.head), *tinc = reinterpret_cast<int32_t *>(base + L.tinc);
    Tri *tri = reinterpret_cast<Tri *>(base + L.tri), *trix = reinterpret_cast<Tri *>(base + L.trix);
    void *tmp = base + L.tmp;
    const size_t N = (size_t)a.rows;
    const int rbits = bits_for(a.rows), end_bit = rbits + bits_for(a.block_rows);
    const dim3 g(blocks_of(a.rows)), b(kT);
    hipLaunchKernelGGL(k_bpr_inv_keys, g, b, 0, s, a.map, a.rows, rbits, key);
    BPR_TRY(hipGetLastError());
    size_t t = L.tmp_bytes;
    BPR_TRY(rocprim::radix_sort_keys(tmp, t, key, sorted, N, 0u, (unsigned)end_bit, s));
    hipLaunchKernelGGL(k_bpr_inv_heads, g, b, 0, s, sorted, a.rows, rbits, a.trow, head);
    BPR_TRY(hipGetLastError());
    t = L.tmp_bytes;
    BPR_TRY(rocprim::inclusive_scan(tmp, t, head, tinc, N, rocprim::plus<int32_t>(), s));
    hipLaunchKernelGGL(k_bpr_inv_touch, g, b, 0, s, sorted, head, tinc, a.rows, rbits, a.tj, a.tptr, a.counts);
    BPR_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_bpr_inv_count, g, b, 0, s, a.tptr, a.counts, a.rows, a.cut, tri);
    BPR_TRY(hipGetLastError());
    t = L.tmp_bytes;
    BPR_TRY(rocprim::exclusive_scan(tmp, t, tri, trix, Tri{0, 0, 0}, N, TriPlus(), s));
    hipLaunchKernelGGL(k_bpr_inv_fill, g, b, 0, s, a, tri, trix);
    return hipGetLastError();
}

#undef BPR_TRY

}  // namespace fmhip
