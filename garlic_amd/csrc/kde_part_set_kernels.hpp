// One shard's parts of one or several split feeds (garlic_kde_part_set, garlic_kde_parts_multi; a garlic_kde_part of
// garlic_kde_parts is a set of one feed, whose sums the host launches as kde_sum_kernel and kde_slice_sum_kernel of
// kde_kernels.hpp): the steps of a part, each once for all F feeds of the set.
// The table, the flat grids and the sums launch are kde_multi_kernels.hpp's (kde_sum_multi_kernel runs unchanged, and
// kde_rank_multi_kernel lives there); the arithmetic is kde_kernels.hpp's __device__ bodies, so part i of a set gives the
// bits of a garlic_kde_part made of the same values.  No floating-point atomics.
//
// Feed f of the table is one PART of union f, whose other parts lie in other sets.  What differs from the whole-feed
// kernels of kde_multi_kernels.hpp is what a part may not decide alone:
//   * pass 1 is about the union's mean, which the host writes into mom.mean of every entry between the passes (one more
//     upload of the table, as the targets are written); pass 0's tree has left the part's own mean there;
//   * the tree also leaves the part's ends x[0], x[n - 1] in mom.stat[0 .. 2) after either pass (the union's lo and hi are
//     the extremes over the parts); idx is not used;
//   * the sums stay undivided: the host adds the parts' and divides by the union's n.
// `active` is the host's: a feed whose union is refused (fewer than 2 values, a NaN, not ascending, no bandwidth) is
// switched off in every set and takes no part in any later launch.  A part of one value has one chunk (the plan of a set
// counts from 1 value, not 2).
#pragma once
#include "kde_multi_kernels.hpp"

namespace garlic {

// one workgroup per (feed, chunk): pass 0 the sum; pass 1 the squared deviations about the mean the host wrote
__global__ void __launch_bounds__(KDE_THREADS)
kde_moment_set_kernel(const KdeFeedDesc *feeds, int n_feeds, KdeMultiFirst first, int pass, double *partial, int32_t *flags)
{
    const int f = kdeMultiFind(first, n_feeds, blockIdx.x);
    const KdeFeedDesc &d = feeds[f];
    const int64_t chunk = (int64_t)blockIdx.x - first.at[f];
    if (!d.active || chunk >= d.n_chunks) return;
    kde_moment_chunk(d.x, d.n, chunk, pass, pass ? d.mom.mean : 0.0, partial + d.chunk_off, flags + d.chunk_off);
}

// one workgroup per feed: kde_tree_feed, and the part's ends
__global__ void __launch_bounds__(KDE_THREADS)
kde_tree_set_kernel(KdeFeedDesc *feeds, int pass, const double *partial, const int32_t *flags)
{
    KdeFeedDesc &d = feeds[blockIdx.x];
    if (!d.active || d.n_chunks == 0) return;
    kde_tree_feed(d.x, d.n, d.n_chunks, pass, partial + d.chunk_off, flags + d.chunk_off, d.idx, &d.mom);
    if (threadIdx.x < 2) d.mom.stat[threadIdx.x] = d.x[threadIdx.x ? d.n - 1 : 0];
}

// one workgroup per (feed, target): kde_slice_total, undivided, into raw
__global__ void __launch_bounds__(KDE_THREADS)
kde_slice_sum_multi_kernel(KdeFeedDesc *feeds, const double *slices)
{
    KdeFeedDesc &d = feeds[blockIdx.x / KDE_POINTS];
    const int target = (int)(blockIdx.x % KDE_POINTS);
    if (!d.active || d.n_slices == 0) return;
    const double total = kde_slice_total(slices + d.slice_off * KDE_POINTS, d.n_slices, target);
    if (threadIdx.x == 0) d.raw[target] = total;
}

} // namespace garlic
