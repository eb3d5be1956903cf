// The KDE of several whole feeds in one set of launches (garlic_feed_kde_multi, garlic_lod_kde_multi): the four steps of
// kde_kernels.hpp, each once for all feeds -- a window-size sweep's feeds are a few hundred chunks each, and one workgroup
// per slice of one feed leaves most of the device idle.  The host driver is also the single calls'; for one feed it
// launches the kernels of kde_kernels.hpp, which take the feed as kernel arguments.
//
//   * a device table of KdeFeedDesc, one per feed, says where the feed lies, how it is partitioned, where its partials lie
//     in the shared arrays, and holds what the steps hand to each other: the moments, the targets with 1 / h^2, the count
//     of skipped pairs, the sums.  The host writes the targets between the moment part and the sums part and reads the
//     table back after either; nothing else crosses.
//   * which workgroup does what is host/kde_multi_plan.hpp: flat grids over the feeds' chunks and slices, the prefix tables
//     passed by value (a function of the feeds' lengths alone).  The tree and slice launches are one workgroup per feed and
//     per (feed, target).
//   * the arithmetic is kde_kernels.hpp's: every kernel here calls a __device__ body of that header with the feed's
//     pointers and the workgroup's place in the feed.  A feed's result does not depend on what else is in the batch.
//   * a feed that is not active (fewer than 2 values; refused after the moments) takes no part in the sums launches: its
//     workgroups leave before the first barrier.  No floating-point atomics.
//   * kde_rank_multi_kernel: the rank queries of F feeds in one launch, for the feeds of a part set (kde_part_set_kernels.hpp,
//     which also runs kde_sum_multi_kernel as it stands).
#pragma once
#include "kde_kernels.hpp"
#include "../host/kde_multi_plan.hpp"

namespace garlic {

using garlic_host::KdeMultiFirst;
using garlic_host::kdeMultiFind;

static_assert(garlic_host::KDE_MULTI_CHUNK == KDE_CHUNK && garlic_host::KDE_MULTI_MAX_SLICES == KDE_MAX_SLICES, "one partition");

struct KdeFeedDesc {
    const double *x;                       // n ascending values (device)
    int64_t n;
    int64_t n_chunks, chunks_per_slice, n_slices;
    int64_t chunk_off, slice_off;          // the feed's first entry of partial / flags, its first row of slices
    KdeIdx idx;                            // where the six order statistics lie
    KdeMoments mom;
    double inv_h2;
    unsigned long long skipped;
    int32_t active, pad;                   // the sums launches skip a feed that is not
    double targets[KDE_POINTS];
    double raw[KDE_POINTS];
};

// one workgroup per (feed, chunk): kde_moment_chunk; pass 1 about the feed's own mean
__global__ void __launch_bounds__(KDE_THREADS)
kde_moment_multi_kernel(const KdeFeedDesc *feeds, int n_feeds, KdeMultiFirst first, int pass, double *partial, int32_t *flags)
{
    const int f = kdeMultiFind(first, n_feeds, blockIdx.x);
    const KdeFeedDesc &d = feeds[f];
    const int64_t chunk = (int64_t)blockIdx.x - first.at[f];
    if (chunk >= d.n_chunks) return;       // (never: the grid is the plan's total)
    kde_moment_chunk(d.x, d.n, chunk, pass, pass ? d.mom.mean : 0.0, partial + d.chunk_off, flags + d.chunk_off);
}

// one workgroup per feed: kde_tree_feed into the feed's moments
__global__ void __launch_bounds__(KDE_THREADS)
kde_tree_multi_kernel(KdeFeedDesc *feeds, int pass, const double *partial, const int32_t *flags)
{
    KdeFeedDesc &d = feeds[blockIdx.x];
    if (d.n_chunks == 0) return;
    kde_tree_feed(d.x, d.n, d.n_chunks, pass, partial + d.chunk_off, flags + d.chunk_off, d.idx, &d.mom);
}

// one workgroup per (feed, slice): kde_sum_slice with the feed's targets and 1 / h^2, skipped pairs counted per feed
__global__ void __launch_bounds__(KDE_THREADS)
kde_sum_multi_kernel(KdeFeedDesc *feeds, int n_feeds, KdeMultiFirst first, double *slices)
{
    const int f = kdeMultiFind(first, n_feeds, blockIdx.x);
    KdeFeedDesc &d = feeds[f];
    const int64_t slice = (int64_t)blockIdx.x - first.at[f];
    if (!d.active || slice >= d.n_slices) return;
    kde_sum_slice(d.x, d.n, d.n_chunks, d.chunks_per_slice, slice, d.targets, d.inv_h2, slices + d.slice_off * KDE_POINTS, &d.skipped);
}

// one workgroup per (feed, target): kde_slice_total, divided by the feed's n
__global__ void __launch_bounds__(KDE_THREADS)
kde_slice_multi_kernel(KdeFeedDesc *feeds, const double *slices)
{
    KdeFeedDesc &d = feeds[blockIdx.x / KDE_POINTS];
    const int target = (int)(blockIdx.x % KDE_POINTS);
    if (!d.active) return;
    const double total = kde_slice_total(slices + d.slice_off * KDE_POINTS, d.n_slices, target);
    if (threadIdx.x == 0) d.raw[target] = total / (double)d.n;
}

// ---- The ranks of a part set's descent (garlic_kde_part_set_rank; the other kernels of a set: kde_part_set_kernels.hpp).
// thread t: probe t % m of feed t / m: below[t] = kde_rank_below on that feed's x, n (n = 0 reads nothing; a feed that is
// not active is not searched and its counts are left as they were).  Every thread is a chain of about log2(n) dependent
// loads with next to no arithmetic between them, so what a launch takes is one chain's latency as long as every wave
// has a SIMD to itself: workgroups of one wave, which the dispatcher spreads over the CUs -- 16 waves for one feed, 512
// for 32 feeds, on 1024 SIMDs.  Blocks of 256 threads would put four chains' waves on one CU and leave the CUs beside it
// idle for the same latency, no faster; registers and LDS do not limit anything here.  Neighbouring lanes hold
// neighbouring digits of one rank's probe, so the first steps of their searches load the same lines.
constexpr int KDE_RANK_SET_THREADS = 64;

__global__ void __launch_bounds__(KDE_RANK_SET_THREADS)
kde_rank_multi_kernel(const KdeFeedDesc *feeds, int n_feeds, const unsigned long long *keys, int m, long long *below)
{
    const int t = blockIdx.x * KDE_RANK_SET_THREADS + threadIdx.x;
    if (t >= n_feeds * m) return;
    const KdeFeedDesc &d = feeds[t / m];
    if (!d.active) return;
    below[t] = kde_rank_below(d.x, d.n, keys[t]);
}

} // namespace garlic
