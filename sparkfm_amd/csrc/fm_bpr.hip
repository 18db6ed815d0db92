// fm_bpr.hip — the BPR trainer's device work (fm_bpr.h): k_bpr_sample draws a negative row per pair, and the k_bpr_inv_* kernels
// around one rocPRIM radix sort and two scans rebuild the candidates relation's inverse map of a batch.  Integer arithmetic only;
// every address has one writer and nothing depends on the launch shape.  k_bpr_sample_walk draws several candidates per pair with
// the same integer code and scores them under the model: the one place with fp32 in it, a dot product whose summation order the row
// width alone fixes.  What a score does to the pair's choice is the walk's rule: BestOfC (include/fmhip_bpr_adaptive.h) keeps the
// candidate the model scores highest, FirstViolator (include/fmhip_warp.h) the first one that violates the margin against the pair's
// positive, with the pair's rank weight beside it.  Where a candidate row comes from is the proposal (include/fmhip_proposal.h), a
// compile-time parameter of both samplers: uniform, or an alias table read with one 8-byte load per attempt.
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

// One draw of pair p under the proposal: uniform (rng::negative_row) or WEIGHTED (rng::proposal_row: per attempt one dependent
// 8-byte load of the alias table in front of row_listed's binary search).  group0: the candidate's group offset, c << 4.
template <bool WEIGHTED>
__device__ __forceinline__ int32_t draw_row(const BprSampleArgs &s, int64_t p, const int32_t *list, int32_t len, int *at, int *f, uint32_t group0) {
    if constexpr (WEIGHTED) return rng::proposal_row(s.seed, (uint32_t)p, s.t, (uint32_t)s.M, s.tab, list, len, at, f, group0);
    else return rng::negative_row(s.seed, (uint32_t)p, s.t, (uint32_t)s.M, list, len, at, f, group0);
}

template <bool WEIGHTED>
__global__ __launch_bounds__(kT) void k_bpr_sample(BprSampleArgs a) {
    u64 att = 0, forced = 0;
    for (int64_t p = a.p0 + (int64_t)blockIdx.x * kT + threadIdx.x; p < a.p1; p += (int64_t)gridDim.x * kT) {
        const int32_t u = a.ictx[p / a.n_neg];
        const int64_t lo = a.pptr[u];
        int at = 0, f = 0;
        a.map[2 * p + 1] = draw_row<WEIGHTED>(a, p, a.prow + lo, (int32_t)(a.pptr[u + 1] - lo), &at, &f, 0u);
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

// ---- the scored samplers: one candidate walk (fm_bpr.h: BprAdaptiveArgs), a choice rule per sampler --------------------------------

constexpr int kCandChunk = 4;       // candidate rows a group has in flight before it reduces: the gathers' latency overlaps

// The scores of N rows of Qi, lane l of a group of G holding floats 4l .. 4l+3 of each and of the context's slice: yq_i + (the lanes'
// 4-term fmaf chains summed by the xor tree over G) — an order G alone fixes, the same in every lane of the group.
template <int G, int N>
__device__ __forceinline__ void group_scores(const float4 &qu, const float4 (&qi)[N], const float (&yq)[N], float (&s)[N]) {
#pragma unroll
    for (int i = 0; i < N; ++i) s[i] = f4dot(qu, qi[i]);
#pragma unroll
    for (int m = G >> 1; m >= 1; m >>= 1)
#pragma unroll
        for (int i = 0; i < N; ++i) s[i] += __shfl_xor(s[i], m, G);
#pragma unroll
    for (int i = 0; i < N; ++i) {
        s[i] = yq[i] + s[i];
        // (the sums are formed here, so the yq loads are issued beside the gathers: left free, the compiler sinks each load into
        // its candidate's branch of the caller, and a chunk pays four load latencies in a row)
        asm volatile("" : "+v"(s[i]));
    }
}

// A choice rule is the state of one pair's walk and what the walk calls on it: begin (before the first draw), drawn (per draw of a
// pair that exists, with the draw's {attempts, forced}), done (asked at the loop heads: may the group stop?), see (per candidate, in
// order, with its row and score) and finish (lane 0 of a pair that exists, not in record mode: the outputs and the pair's share of
// the N counters).

// Best of C: the first strict maximum.
struct BestOfC {
    using Args = BprAdaptiveArgs;
    static constexpr int N = 3;      // {attempts, forced, replaced pairs}
    static __host__ __device__ const BprAdaptiveArgs &walk_args(const Args &a) { return a; }
    static bool valid(const Args &, bool) { return true; }
    int32_t keep = 0, keep_c = 0;
    float best = 0.f;
    template <int G, bool RECORD>
    __device__ __forceinline__ void begin(const Args &, int64_t, const float4 &, int, bool) {}
    __device__ __forceinline__ void drawn(u64 (&v)[N], int at, int f) const {
        v[0] += (u64)at;
        v[1] += (u64)f;
    }
    static constexpr __device__ bool done() { return false; }
    __device__ __forceinline__ void see(int c, int32_t row, float s) {
        if (c == 0 || s > best) {      // candidate 0 is the incumbent; a NaN is never greater
            best = s;
            keep = row;
            keep_c = c;
        }
    }
    __device__ __forceinline__ void finish(const Args &a, int64_t p, u64 (&v)[N]) const {
        a.s.map[2 * p + 1] = keep;
        v[2] += keep_c != 0 ? 1u : 0u;
    }
};

// The first violator (WARP): the positive's row is scored first, by the code that scores a candidate; a candidate violates iff its
// score is strictly above thr (false for a NaN on either side).  Every lane of a group holds the same scores, so `n_first` and the
// early exit are uniform over the group: a group that leaves the candidate loops leaves whole, and the width-G shuffles of the
// groups still in them read only their own lanes.
struct FirstViolator {
    using Args = BprWarpArgs;
    static constexpr int N = 2;      // {violated pairs, sum of their trials}
    static __host__ __device__ const BprAdaptiveArgs &walk_args(const Args &w) { return w.a; }
    static bool valid(const Args &w, bool record) { return w.margin >= 0.f && (record ? w.rec_pos != nullptr : w.W && w.c && w.trials); }
    float thr = 0.f;
    int32_t keep = 0, n_first = 0;
    template <int G, bool RECORD>
    __device__ __forceinline__ void begin(const Args &w, int64_t p, const float4 &qu, int l, bool writes) {
        const int32_t ipos = w.a.s.map[2 * p];      // (the positive: no sampler writes the even entries)
        const float4 qp[1] = {reinterpret_cast<const float4 *>(w.a.Qi + (size_t)ipos * (4 * G))[l]};
        const float yp[1] = {w.a.yqi[ipos]};
        float spos[1];
        group_scores<G, 1>(qu, qp, yp, spos);
        if (RECORD && writes) w.rec_pos[p - w.a.s.p0] = spos[0];
        thr = spos[0] - w.margin;
    }
    __device__ __forceinline__ void drawn(u64 (&)[N], int, int) const {}
    __device__ __forceinline__ bool done() const { return n_first != 0; }
    __device__ __forceinline__ void see(int c, int32_t row, float s) {
        if (c == 0) keep = row;                        // no violator: candidate 0's row
        if (n_first == 0 && s > thr) {                 // the first violator; a NaN is never greater
            n_first = c + 1;
            keep = row;
        }
    }
    __device__ __forceinline__ void finish(const Args &w, int64_t p, u64 (&v)[N]) const {
        w.a.s.map[2 * p + 1] = keep;
        const float cw = w.W[n_first];
        reinterpret_cast<float2 *>(w.c)[p] = make_float2(cw, cw);
        w.trials[p] = n_first;
        v[0] += n_first != 0 ? 1u : 0u;
        v[1] += (u64)n_first;
    }
};

// G lanes per pair, kT / G pairs per block and pass, over the pairs [s.p0, s.p1) in either mode.  The trip count is the block's
// (`base` is uniform), and a group whose pair lies past the end works on the range's last pair again and writes nothing: no lane
// leaves before the block's last shuffle.
template <int G, class Rule, bool RECORD, bool WEIGHTED>
__global__ __launch_bounds__(kT) void k_bpr_sample_walk(typename Rule::Args ra) {
    constexpr int KP = 4 * G, GPB = kT / G;
    const BprAdaptiveArgs &a = Rule::walk_args(ra);
    const int l = threadIdx.x & (G - 1), grp = threadIdx.x / G;
    const int64_t first = a.s.p0, end = a.s.p1;
    const int C = a.n_cand;
    u64 v[Rule::N] = {};
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
        Rule r;
        r.template begin<G, RECORD>(ra, p, qu, l, live && l == 0);
        for (int c0 = 0; c0 < C && (RECORD || !r.done()); c0 += G) {
            // the group's lanes draw candidates c0 .. c0 + G - 1 side by side
            int32_t mine = 0;
            if (c0 + l < C) {
                int at = 0, f = 0;
                mine = draw_row<WEIGHTED>(a.s, p, a.s.prow + lo, len, &at, &f, (uint32_t)(c0 + l) << 4);
                if (live) r.drawn(v, at, f);
            }
            const int n = C - c0 < G ? C - c0 : G;
            for (int j0 = 0; j0 < n && (RECORD || !r.done()); j0 += kCandChunk) {
                int32_t row[kCandChunk];
                float4 qi[kCandChunk];
                float yq[kCandChunk], s[kCandChunk];
#pragma unroll
                for (int jj = 0; jj < kCandChunk; ++jj) {
                    const int j = j0 + jj < n ? j0 + jj : n - 1;       // (past the last candidate: the last one again, not compared)
                    row[jj] = __shfl(mine, j, G);
                    qi[jj] = reinterpret_cast<const float4 *>(a.Qi + (size_t)row[jj] * KP)[l];
                    yq[jj] = a.yqi[row[jj]];
                }
                group_scores<G, kCandChunk>(qu, qi, yq, s);
#pragma unroll
                for (int jj = 0; jj < kCandChunk; ++jj) {
                    const int c = c0 + j0 + jj;
                    if (j0 + jj >= n) break;
                    if (RECORD && live && l == 0) {
                        const size_t at = (size_t)(p - first) * (size_t)C + (size_t)c;
                        a.rec_rows[at] = row[jj];
                        a.rec_scores[at] = s[jj];
                    }
                    r.see(c, row[jj], s[jj]);
                }
            }
        }
        if (!RECORD && live && l == 0) r.finish(ra, p, v);
    }
    if (RECORD) return;
    block_sums_u64<Rule::N>(v, a.s.part + Rule::N * (size_t)blockIdx.x);
}

// record mode (rec_rows set): the walk alone; else the walk and the one-block sum of its partials
template <int G, class Rule, bool WEIGHTED>
hipError_t launch_walk_under(const typename Rule::Args &ra, hipStream_t s) {
    const BprAdaptiveArgs &a = Rule::walk_args(ra);
    const bool record = a.rec_rows != nullptr;
    const int blocks = bpr_adaptive_blocks(4 * G, (int64_t)a.s.p1 - a.s.p0);
    if (record) {
        hipLaunchKernelGGL((k_bpr_sample_walk<G, Rule, true, WEIGHTED>), dim3((unsigned)blocks), dim3(kT), 0, s, ra);
        return hipGetLastError();
    }
    hipLaunchKernelGGL((k_bpr_sample_walk<G, Rule, false, WEIGHTED>), dim3((unsigned)blocks), dim3(kT), 0, s, ra);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_bpr_total<Rule::N>, dim3(1), dim3(kT), 0, s, a.s.part, blocks, a.s.total);
    return hipGetLastError();
}

// the proposal picks the instantiation: a table, the weighted one
template <int G, class Rule>
hipError_t launch_walk(const typename Rule::Args &ra, hipStream_t s) {
    return Rule::walk_args(ra).s.tab ? launch_walk_under<G, Rule, true>(ra, s) : launch_walk_under<G, Rule, false>(ra, s);
}

template <class Rule>
hipError_t launch_scored(int Kp, const typename Rule::Args &ra, hipStream_t s) {
    const BprAdaptiveArgs &a = Rule::walk_args(ra);
    const bool record = a.rec_rows != nullptr;
    if (a.n_cand < 1 || a.n_cand > kBprMaxCand || a.k < 0 || a.k > Kp || !Rule::valid(ra, record)) return hipErrorInvalidValue;
    if (a.s.p0 < 0 || a.s.p1 > a.s.n_pairs || a.s.p0 >= a.s.p1 || (record && !a.rec_scores)) return hipErrorInvalidValue;
    switch (Kp) {
        case 32: return launch_walk<8, Rule>(ra, s);
        case 64: return launch_walk<16, Rule>(ra, s);
        case 128: return launch_walk<32, Rule>(ra, s);
        case 256: return launch_walk<64, Rule>(ra, s);
        default: return hipErrorInvalidValue;      // (padded_factors: a power of two in [32, 256])
    }
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
    if (a.p0 < 0 || a.p1 > a.n_pairs || a.p0 >= a.p1) return hipErrorInvalidValue;
    const int blocks = bpr_sample_blocks((int64_t)a.p1 - a.p0);
    if (a.tab) hipLaunchKernelGGL(k_bpr_sample<true>, dim3((unsigned)blocks), dim3(kT), 0, s, a);
    else hipLaunchKernelGGL(k_bpr_sample<false>, dim3((unsigned)blocks), dim3(kT), 0, s, a);
    BPR_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_bpr_total<2>, dim3(1), dim3(kT), 0, s, a.part, blocks, a.total);
    return hipGetLastError();
}

int bpr_adaptive_blocks(int Kp, int64_t n_pairs) { return grid_blocks(n_pairs, kT / (Kp / 4), 4096); }      // a group of Kp / 4 lanes per pair

hipError_t launch_bpr_sample_adaptive(int Kp, const BprAdaptiveArgs &a, hipStream_t s) { return launch_scored<BestOfC>(Kp, a, s); }
hipError_t launch_bpr_sample_warp(int Kp, const BprWarpArgs &w, hipStream_t s) { return launch_scored<FirstViolator>(Kp, w, s); }

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
