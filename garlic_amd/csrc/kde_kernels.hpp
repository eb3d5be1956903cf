// computeKDE's numbers on the device (src/garlic-kde.cpp:14-140): what nrd0 needs of the sorted feed, and the Gaussian
// sums at the 512 targets -- the plain sums that FIGTree (epsilon 1e-2) approximates, not FIGTree's output.
//
//   * moments, two passes over x in chunks of KDE_CHUNK (one workgroup per chunk): kde_moment_kernel writes one partial
//     per chunk -- pass 0 the sum, pass 1 the sum of (x - mean)^2 -- every thread adding its KDE_CHUNK / KDE_THREADS
//     elements in index order, then a binary tree over the threads in LDS.  kde_tree_kernel (one workgroup) adds the
//     chunks' partials the same way: thread t takes partials t, t + 256, ... in order, then the tree.  Pass 0 leaves the
//     mean on the device for pass 1; pass 1 also fetches the order statistics by index.  Both passes raise integer flags
//     per chunk (ordinary stores, OR-ed by the tree kernel): a value that is not finite; x[i] < x[i - 1], the element in
//     front of a chunk's first included.
//   * sums: kde_sum_kernel, one workgroup per slice of `chunks_per_slice` consecutive chunks.  A chunk's sources are
//     staged in LDS; thread t owns targets 2t and 2t + 1 and walks the chunk once, in index order, for both (two
//     independent exp chains per source), every lane of a wave reading the same LDS word (a broadcast, no bank
//     conflict).  exp() is the device library's FP64 exp; the argument is -((x - t) * (x - t)) * (1 / h^2), every
//     operation rounded on its own.  A chunk's sum is added to the slice's sum, the slice's sums go to
//     partial[slice][512], and kde_slice_kernel (one workgroup per target) adds the slices: thread t slices t, t + 256,
//     ... in order, then the tree.
//   * the partition is a function of n alone (kde_chunks_per_slice of the chunk count ceil(n / KDE_CHUNK)): not of the
//     device's CU count, not of timing.  No floating-point atomics anywhere.
//   * exact skipping: the sources are ascending, so a chunk is the interval [first, last].  For a target outside it the
//     argument of the nearer end, computed by the very operations of the loop, bounds every argument of the chunk from
//     above (subtraction, multiplication and negation are monotone under rounding); below KDE_SKIP_ARG every term is
//     exp(< -746) = +0.0 and the pair (chunk, target) is skipped.  Nothing nearer is.  A thread with one skippable
//     target walks the chunk for the other alone; a wave whose 64 lanes skip both enters no loop.  The count of
//     skipped pairs (integer adds) is what garlic_feed_kde_info reports.
//   * 64-bit element indices and counts; a chunk count fits 32 bits (checked by the caller).
//   * the bodies are __device__ functions of (feed, chunk / slice / target): the kernels here pass blockIdx.x, the batched
//     kernels of kde_multi_kernels.hpp the place of the workgroup in its feed -- one source, one result.  The host has
//     one driver per path; it launches the kernels here where a call holds ONE feed, because they take x and n as kernel
//     arguments: the batched kernels fetch them from the table, read x through flat loads and start every workgroup with
//     one more dependent scalar load, which shows in the event times of one feed (profiles/kde_one_driver_ab.txt).
//   * a feed split into parts (garlic_kde_parts): pass 1 is about the union's mean (the host writes it where pass 0
//     left the part's own), kde_slice_sum_kernel leaves a part's sums undivided, kde_rank_below counts the values below
//     a probe key (kde_rank_multi_kernel).  They run the lines of the whole feed, so one part gives its bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace garlic {

constexpr int KDE_CHUNK = 2048;            // sources per chunk (tests read this)
constexpr int KDE_THREADS = 256;
constexpr int KDE_POINTS = 512;            // GARLIC_KDE_POINTS
constexpr int KDE_PER_THREAD = KDE_POINTS / KDE_THREADS;
constexpr int KDE_MAX_SLICES = 2048;
constexpr double KDE_SKIP_ARG = -746.0;    // exp(a) = +0.0 for every a below (the smallest subnormal is exp(-744.44))

constexpr int KDE_FLAG_NOT_FINITE = 1, KDE_FLAG_NOT_ASCENDING = 2;

struct KdeMoments {
    double sum, mean, ssq;
    double stat[6];                        // x[0], x[n - 1], x[k25], x[k25 + 1], x[k75], x[k75 + 1]
    int32_t flags, pad;
};

__host__ __device__ inline int64_t kde_chunks_per_slice(int64_t n_chunks)
{
    return (n_chunks + KDE_MAX_SLICES - 1) / KDE_MAX_SLICES;
}

// binary tree over the workgroup's values: red[0] holds the total afterwards (every thread has passed the last barrier)
__device__ __forceinline__ double kde_block_tree(double v, double *red)
{
    red[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int o = KDE_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    return red[0];
}

// chunk `chunk`'s partial and flags: pass 0 the sum, pass 1 the sum of (x - mean)^2 (every moment kernel runs these lines,
// the single-feed ones with blockIdx.x for the chunk, kde_multi_kernels.hpp with the chunk of the workgroup's feed)
__device__ __forceinline__ void kde_moment_chunk(const double *x, int64_t n, int64_t chunk, int pass, double mean, double *partial,
                                                 int32_t *flags)
{
    __shared__ double red[KDE_THREADS];
    __shared__ int32_t flag;
    if (threadIdx.x == 0) flag = 0;
    __syncthreads();
    const int64_t i0 = chunk * KDE_CHUNK;
    double acc = 0.0;
    int32_t f = 0;
    for (int j = 0; j < KDE_CHUNK / KDE_THREADS; j++) {
        const int64_t i = i0 + (int64_t)j * KDE_THREADS + threadIdx.x;
        if (i >= n) break;
        const double v = x[i];
        if (((unsigned long long)__double_as_longlong(v) >> 52 & 0x7ffull) == 0x7ffull) f |= KDE_FLAG_NOT_FINITE;
        if (i > 0 && v < x[i - 1]) f |= KDE_FLAG_NOT_ASCENDING;
        if (pass) {
            const double d = v - mean;
            acc += d * d;
        } else {
            acc += v;
        }
    }
    if (f) atomicOr(&flag, f);             // (LDS, integer)
    const double total = kde_block_tree(acc, red);
    if (threadIdx.x == 0) {
        partial[chunk] = total;
        flags[chunk] = flag;
    }
}

// pass 0: partial[chunk] = sum of the chunk; pass 1: sum of (x - mean)^2 with mom->mean
__global__ void __launch_bounds__(KDE_THREADS)
kde_moment_kernel(const double *x, int64_t n, int pass, const KdeMoments *mom, double *partial, int32_t *flags)
{
    kde_moment_chunk(x, n, blockIdx.x, pass, pass ? mom->mean : 0.0, partial, flags);
}

// one workgroup: the chunks' partials and flags; pass 0 -> sum and mean, pass 1 -> ssq and the order statistics at idx[6]
struct KdeIdx { int64_t at[6]; };

// one feed's tree, by one workgroup (kde_tree_kernel; kde_tree_multi_kernel, one workgroup per feed)
__device__ __forceinline__ void kde_tree_feed(const double *x, int64_t n, int64_t n_chunks, int pass, const double *partial,
                                              const int32_t *flags, const KdeIdx &idx, KdeMoments *mom)
{
    __shared__ double red[KDE_THREADS];
    __shared__ int32_t flag;
    if (threadIdx.x == 0) flag = 0;
    __syncthreads();
    double acc = 0.0;
    int32_t f = 0;
    for (int64_t c = threadIdx.x; c < n_chunks; c += KDE_THREADS) {
        acc += partial[c];
        f |= flags[c];
    }
    if (f) atomicOr(&flag, f);
    const double total = kde_block_tree(acc, red);
    if (threadIdx.x == 0) {
        if (pass == 0) {
            mom->sum = total;
            mom->mean = total / (double)n;
            mom->flags = flag;
        } else {
            mom->ssq = total;
            mom->flags |= flag;
        }
    }
    if (pass == 1 && threadIdx.x < 6) {
        const int64_t i = idx.at[threadIdx.x];
        mom->stat[threadIdx.x] = x[i < 0 ? 0 : (i >= n ? n - 1 : i)];
    }
}

__global__ void __launch_bounds__(KDE_THREADS)
kde_tree_kernel(const double *x, int64_t n, int64_t n_chunks, int pass, const double *partial, const int32_t *flags,
                KdeIdx idx, KdeMoments *mom)
{
    kde_tree_feed(x, n, n_chunks, pass, partial, flags, idx, mom);
}

// slice `slice` of one feed, by one workgroup: its chunks' sums at the 512 targets into partial[slice][512] (kde_sum_kernel;
// kde_sum_multi_kernel with the slice, the targets and 1 / h^2 of the workgroup's feed)
__device__ __forceinline__ void kde_sum_slice(const double *x, int64_t n, int64_t n_chunks, int64_t chunks_per_slice, int64_t slice,
                                              const double *targets, double inv_h2, double *partial, unsigned long long *skipped)
{
    __shared__ double src[KDE_CHUNK];
    __shared__ unsigned int n_skipped;
    if (threadIdx.x == 0) n_skipped = 0;
    static_assert(KDE_PER_THREAD == 2, "the source loop below is written for two targets per thread");
    // thread t owns the neighbours 2t and 2t + 1: what one of them may skip the other mostly may too
    const double t0 = targets[2 * threadIdx.x], t1 = targets[2 * threadIdx.x + 1];
    double sum0 = 0.0, sum1 = 0.0;
    const int64_t c0 = slice * chunks_per_slice;
    const int64_t c1 = c0 + chunks_per_slice < n_chunks ? c0 + chunks_per_slice : n_chunks;
    unsigned int mine = 0;
    for (int64_t c = c0; c < c1; c++) {
        const int64_t i0 = c * KDE_CHUNK;
        const int cn = (int)(n - i0 < KDE_CHUNK ? n - i0 : KDE_CHUNK);
        __syncthreads();                   // the chunk before has been read by everyone
        for (int j = threadIdx.x; j < cn; j += KDE_THREADS) src[j] = x[i0 + j];
        __syncthreads();
        const double first = src[0], last = src[cn - 1];
        // the nearer end of the interval, when the target lies outside it, through the loop's own operations
        auto skippable = [&](double t) {
            if (!(t < first || t > last)) return false;
            const double d = (t < first ? first : last) - t;
            return -(d * d) * inv_h2 < KDE_SKIP_ARG;
        };
        const bool skip0 = skippable(t0), skip1 = skippable(t1);
        if (skip0 && skip1) {
            mine += 2;
        } else if (skip0 || skip1) {       // one target alone
            const double t = skip0 ? t1 : t0;
            double acc = 0.0;
            for (int i = 0; i < cn; i++) {
                const double d = src[i] - t;
                acc += exp(-(d * d) * inv_h2);
            }
            if (skip0) sum1 += acc; else sum0 += acc;
            mine++;
        } else {                           // both targets from one read of every source: two independent exp chains
            double acc0 = 0.0, acc1 = 0.0;
            for (int i = 0; i < cn; i++) {
                const double s = src[i];
                const double d0 = s - t0, d1 = s - t1;
                acc0 += exp(-(d0 * d0) * inv_h2);
                acc1 += exp(-(d1 * d1) * inv_h2);
            }
            sum0 += acc0;
            sum1 += acc1;
        }
    }
    if (mine) atomicAdd(&n_skipped, mine);
    __syncthreads();
    if (threadIdx.x == 0 && n_skipped) atomicAdd(skipped, (unsigned long long)n_skipped);
    partial[slice * KDE_POINTS + 2 * threadIdx.x] = sum0;
    partial[slice * KDE_POINTS + 2 * threadIdx.x + 1] = sum1;
}

__global__ void __launch_bounds__(KDE_THREADS)
kde_sum_kernel(const double *x, int64_t n, int64_t n_chunks, int64_t chunks_per_slice, const double *targets, double inv_h2,
               double *partial, unsigned long long *skipped)
{
    kde_sum_slice(x, n, n_chunks, chunks_per_slice, blockIdx.x, targets, inv_h2, partial, skipped);
}

// the slices' sums of target `target` in the fixed order: thread t slices t, t + 256, ..., then the tree
__device__ __forceinline__ double kde_slice_total(const double *partial, int64_t n_slices, int target)
{
    __shared__ double red[KDE_THREADS];
    double acc = 0.0;
    for (int64_t s = threadIdx.x; s < n_slices; s += KDE_THREADS) acc += partial[s * KDE_POINTS + target];
    return kde_block_tree(acc, red);
}

// workgroup j: raw[j] = (sum over the slices, in the fixed order) / n
__global__ void __launch_bounds__(KDE_THREADS)
kde_slice_kernel(const double *partial, int64_t n_slices, int64_t n, double *raw)
{
    const double total = kde_slice_total(partial, n_slices, blockIdx.x);
    if (threadIdx.x == 0) raw[blockIdx.x] = total / (double)n;
}

// workgroup j: sums[j] = the same total, undivided (a part of a split feed: the host adds the parts and divides by the union's n)
__global__ void __launch_bounds__(KDE_THREADS)
kde_slice_sum_kernel(const double *partial, int64_t n_slices, double *sums)
{
    const double total = kde_slice_total(partial, n_slices, blockIdx.x);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// garlic_feed_sort's key (garlic_hip.h): unsigned order of the keys is ascending order of the doubles, -0.0 before +0.0
__device__ __forceinline__ unsigned long long kde_key(double v)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return b ^ (b >> 63 ? 0xFFFFFFFFFFFFFFFFull : 0x8000000000000000ull);
}

// how many of x[0 .. n) have a key below `key` (x ascending in key order: a lower bound).  About log2(n) dependent loads.
// mid < hi <= n, so no read leaves the array; n = 0 reads nothing.  (kde_rank_multi_kernel on a feed of a set)
__device__ __forceinline__ int64_t kde_rank_below(const double *x, int64_t n, unsigned long long key)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (kde_key(x[mid]) < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// a rank launch holds at most KDE_RANK_MAX probes per feed (one round of the descent of host/kde_parts.hpp)
constexpr int KDE_RANK_MAX = 1024;

} // namespace garlic
