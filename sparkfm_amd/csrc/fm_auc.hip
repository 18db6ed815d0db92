// fm_auc.hip — ROC AUC and per-group AUC (GAUC) of a set of predictions, exactly: one 64-bit word per row, one stable radix sort
// (rocPRIM), two scans and two compactions over the sorted words, a thread per run and a thread per group.  Formulas: fm_auc.h.
// Every count is an integer (uint64, no atomics of any kind); the one floating-point sum (GAUC's numerator, fp64) is formed by
// a reduction whose shape is fixed by the constants below, not by the device or the launch.
#include "fm_auc.h"
#include "fm_score_key.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

namespace fmhip {
namespace {

typedef unsigned long long u64;
constexpr int kT = 256;     // threads of every kernel here; a group partial covers exactly kT groups (part of the sum's fixed shape)

__global__ __launch_bounds__(kT) void k_auc_key(const float *score, const float *y, const int32_t *group, int64_t rows, u64 *words) {
    const int64_t r = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (r >= rows) return;
    const u64 g = group ? (u64)(uint32_t)group[r] : 0ull;
    // s + 0.f: -0 ties with +0; NaN keys 0, below -Inf (top-K's rule, fm_score_key.h)
    words[r] = g << kAucGroupShift | (u64)score_key(score[r] + 0.f) << kAucScoreShift | (y[r] > 0.f ? 1ull : 0ull);
}

struct NegFlag {
    __device__ uint32_t operator()(u64 w) const { return (uint32_t)(~w & 1ull); }
};
// position i starts a stretch of equal (word >> shift)
struct HeadAt {
    const u64 *W;
    int shift;
    __device__ bool operator()(int32_t i) const { return i == 0 || (W[i] >> shift) != (W[i - 1] >> shift); }
};

// the negatives before position p (cinc: the inclusive scan of the negative flags)
__device__ __forceinline__ u64 neg_before(const uint32_t *cinc, int64_t p) { return p == 0 ? 0ull : (u64)cinc[p - 1]; }

// a thread per run: A_r = pos_r * (2 cneg(start) + neg_r)
__global__ __launch_bounds__(kT) void k_auc_runs(const int32_t *rstart, int32_t R, int64_t n, const uint32_t *cinc, u64 *A) {
    const int64_t r = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (r >= R) return;
    const int64_t s = rstart[r], e = r + 1 < R ? (int64_t)rstart[r + 1] : n;
    const u64 nb = neg_before(cinc, s), neg = neg_before(cinc, e) - nb, pos = (u64)(e - s) - neg;
    A[r] = pos * (2ull * nb + neg);
}

struct AucPart {
    double num;
    u64 u2, pairs, scored, rows;
};

__device__ __forceinline__ void part_add(AucPart &a, const AucPart &b) {
    a.num += b.num;
    a.u2 += b.u2;
    a.pairs += b.pairs;
    a.scored += b.scored;
    a.rows += b.rows;
}

// the block's sum, valid in thread 0: a butterfly inside each wave, then the waves in index order
__device__ __forceinline__ AucPart part_block_sum(AucPart v) {
    __shared__ AucPart sh[kT / 64];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        AucPart o;
        o.num = __shfl_xor(v.num, m, 64);
        o.u2 = __shfl_xor(v.u2, m, 64);
        o.pairs = __shfl_xor(v.pairs, m, 64);
        o.scored = __shfl_xor(v.scored, m, 64);
        o.rows = __shfl_xor(v.rows, m, 64);
        part_add(v, o);
    }
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    AucPart t = sh[0];
#pragma unroll
    for (int w = 1; w < kT / 64; ++w) part_add(t, sh[w]);
    return t;
}

// the first run that starts at row position `pos` (every group head is a run head)
__device__ __forceinline__ int32_t run_at(const int32_t *rstart, int32_t R, int32_t pos) {
    int32_t lo = 0, hi = R;
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (rstart[mid] < pos) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// a thread per group, kT groups per partial: 2 U_g = sum A_r - 2 cneg(start) pos_g; a group with one class adds nothing
__global__ __launch_bounds__(kT) void k_auc_groups(const int32_t *gstart, int32_t G, const int32_t *rstart, int32_t R, int64_t n,
                                                   const uint32_t *cinc, const u64 *SA, AucPart *parts) {
    const int64_t g = (int64_t)blockIdx.x * kT + threadIdx.x;
    AucPart v = {0.0, 0ull, 0ull, 0ull, 0ull};
    if (g < G) {
        const int32_t s = gstart[g];
        const bool last = g + 1 >= G;
        const int64_t e = last ? n : (int64_t)gstart[g + 1];
        const int32_t r0 = run_at(rstart, R, s), r1 = last ? R : run_at(rstart, R, (int32_t)e);
        const u64 sumA = SA[r1 - 1] - (r0 > 0 ? SA[r0 - 1] : 0ull);
        const u64 nb = neg_before(cinc, s), neg = neg_before(cinc, e) - nb, rows = (u64)(e - s), pos = rows - neg;
        if (pos > 0 && neg > 0) {
            v.u2 = sumA - 2ull * nb * pos;
            v.pairs = pos * neg;
            v.scored = 1ull;
            v.rows = rows;
            v.num = (double)rows * ((double)v.u2 / (2.0 * (double)v.pairs));
        }
    }
    const AucPart t = part_block_sum(v);
    if (threadIdx.x == 0) parts[blockIdx.x] = t;
}

// one workgroup: thread t adds partials t, t + kT, .. in that order, then the block's sum
__global__ __launch_bounds__(kT) void k_auc_final(const AucPart *parts, int32_t n_parts, int32_t G, int64_t n, const uint32_t *cinc,
                                                  AucSums *out) {
    AucPart v = {0.0, 0ull, 0ull, 0ull, 0ull};
    for (int32_t i = threadIdx.x; i < n_parts; i += kT) part_add(v, parts[i]);
    const AucPart t = part_block_sum(v);
    if (threadIdx.x == 0) {
        out->u2 = t.u2;
        out->pairs = t.pairs;
        out->groups = (uint64_t)G;
        out->groups_scored = t.scored;
        out->rows_scored = t.rows;
        out->negatives = neg_before(cinc, n);
        out->gauc_num = t.num;
    }
}

struct DevMem {
    void *p = nullptr;
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 1); }
    ~DevMem() {
        if (p) (void)hipFree(p);
    }
};

inline unsigned blocks_of(int64_t n) { return (unsigned)((n + kT - 1) / kT); }

}  // namespace

hipError_t launch_auc_keys(const float *score, const float *y, const int32_t *group, int64_t rows, unsigned long long *words,
                           hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_auc_key, dim3(blocks_of(rows)), dim3(kT), 0, s, score, y, group, rows, words);
    return hipGetLastError();
}

#define AUC_TRY(expr)                    \
    do {                                 \
        hipError_t _e = (expr);          \
        if (_e != hipSuccess) return _e; \
    } while (0)

hipError_t auc_from_words(unsigned long long *words, int64_t n, int end_bit, hipStream_t s, AucSums *out) {
    if (n < 1 || n > 0x7fffffffll || end_bit < kAucGroupShift || end_bit > 64) return hipErrorInvalidValue;
    const size_t N = (size_t)n;
    const rocprim::counting_iterator<int32_t> rows0(0);
    u64 *W = nullptr;            // the sorted words
    uint32_t *cinc = nullptr;    // inclusive scan of the negative flags
    int32_t *rstart = nullptr, *gstart = nullptr, *counts = nullptr;
    u64 *A = words;              // the sort reads `words` and writes W: from then on `words` holds A_r and its scan
    // temporary storage: the largest of the five rocPRIM calls' needs (the scan over runs is bounded by n)
    size_t tb = 0, t = 0;
    AUC_TRY(rocprim::radix_sort_keys(nullptr, t, words, W, N, 0u, (unsigned)end_bit, s));
    tb = t > tb ? t : tb;
    AUC_TRY(rocprim::inclusive_scan(nullptr, t, rocprim::make_transform_iterator(W, NegFlag()), cinc, N, rocprim::plus<uint32_t>(), s));
    tb = t > tb ? t : tb;
    AUC_TRY(rocprim::select(nullptr, t, rows0, rstart, counts, N, HeadAt{W, kAucScoreShift}, s));
    tb = t > tb ? t : tb;
    AUC_TRY(rocprim::inclusive_scan(nullptr, t, A, A, N, rocprim::plus<u64>(), s));
    tb = t > tb ? t : tb;

    // ONE allocation for the call (an allocation and its free cost more than any kernel here): the arrays, each 256-B aligned
    const size_t max_parts = blocks_of(n);
    size_t off = 0;
    const auto take = [&off](size_t bytes) {
        const size_t at = off;
        off += (bytes + 255) / 256 * 256;
        return at;
    };
    const size_t oW = take(N * sizeof(u64)), oc = take(N * sizeof(uint32_t)), orr = take(N * sizeof(int32_t)), og = take(N * sizeof(int32_t)),
                 ocount = take(2 * sizeof(int32_t)), oout = take(sizeof(AucSums)), oparts = take(max_parts * sizeof(AucPart)), otmp = take(tb);
    DevMem mem;
    AUC_TRY(mem.alloc(off));
    char *base = static_cast<char *>(mem.p);
    W = reinterpret_cast<u64 *>(base + oW);
    cinc = reinterpret_cast<uint32_t *>(base + oc);
    rstart = reinterpret_cast<int32_t *>(base + orr);
    gstart = reinterpret_cast<int32_t *>(base + og);
    counts = reinterpret_cast<int32_t *>(base + ocount);
    AucSums *d_out = reinterpret_cast<AucSums *>(base + oout);
    AucPart *parts = reinterpret_cast<AucPart *>(base + oparts);
    void *tmp = base + otmp;

    t = tb;
    AUC_TRY(rocprim::radix_sort_keys(tmp, t, words, W, N, 0u, (unsigned)end_bit, s));
    t = tb;
    AUC_TRY(rocprim::inclusive_scan(tmp, t, rocprim::make_transform_iterator(W, NegFlag()), cinc, N, rocprim::plus<uint32_t>(), s));
    t = tb;
    AUC_TRY(rocprim::select(tmp, t, rows0, rstart, counts, N, HeadAt{W, kAucScoreShift}, s));
    t = tb;
    AUC_TRY(rocprim::select(tmp, t, rows0, gstart, counts + 1, N, HeadAt{W, kAucGroupShift}, s));
    int32_t h_counts[2] = {0, 0};
    AUC_TRY(hipMemcpyAsync(h_counts, counts, sizeof h_counts, hipMemcpyDeviceToHost, s));
    AUC_TRY(hipStreamSynchronize(s));
    const int32_t R = h_counts[0], G = h_counts[1];
    if (R < 1 || G < 1 || G > R || (int64_t)R > n) return hipErrorUnknown;      // (n >= 1: position 0 heads a run and a group)

    hipLaunchKernelGGL(k_auc_runs, dim3(blocks_of(R)), dim3(kT), 0, s, rstart, R, n, cinc, A);
    AUC_TRY(hipGetLastError());
    t = tb;
    AUC_TRY(rocprim::inclusive_scan(tmp, t, A, A, (size_t)R, rocprim::plus<u64>(), s));
    const unsigned n_parts = blocks_of(G);
    hipLaunchKernelGGL(k_auc_groups, dim3(n_parts), dim3(kT), 0, s, gstart, G, rstart, R, n, cinc, A, parts);
    AUC_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_auc_final, dim3(1), dim3(kT), 0, s, parts, (int32_t)n_parts, G, n, cinc, d_out);
    AUC_TRY(hipGetLastError());
    AUC_TRY(hipMemcpyAsync(out, d_out, sizeof *out, hipMemcpyDeviceToHost, s));
    return hipStreamSynchronize(s);      // (the workspace is freed behind a drained stream)
}

#undef AUC_TRY

}  // namespace fmhip
