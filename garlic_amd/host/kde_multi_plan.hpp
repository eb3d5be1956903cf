// Which workgroup of a batched KDE launch (csrc/kde_multi_kernels.hpp) works on which (feed, chunk) or (feed, slice), and
// where every feed's partials lie in the shared arrays: a function of the feeds' lengths alone -- not of the device, not
// of the values, not of which feeds turn out to be usable.
//
//   * a feed of n >= 2 values has ceil(n / 2048) chunks, kde_chunks_per_slice(chunks) chunks per slice and
//     ceil(chunks / chunks_per_slice) <= 2048 slices: exactly the partition of the single-feed call, so a feed's sums are
//     added in the single call's order.  A feed of fewer than 2 values (refused before anything runs) has none.  The
//     feeds of a part set (kdePartSetPlan) are parts of unions: there one value is a chunk, and only an empty part has none.
//   * the launches are flat: workgroup b of the moment launch is chunk (b - chunk_first[f]) of the feed f with
//     chunk_first[f] <= b < chunk_first[f + 1]; the sums launch likewise over slice_first.  The tables are exclusive
//     prefix sums with the total at [n_feeds], padded with the total up to [KDE_MULTI_MAX_FEEDS]; kdeMultiFind is the
//     search (at most KDE_MULTI_MAX_FEEDS steps, the same on the host and in the kernels).
//   * chunk_first[f] is also feed f's offset into the shared per-chunk arrays (partial, flags) and slice_first[f] its
//     offset, in rows of 512, into the shared per-slice sums: no two feeds overlap, nothing is left between them.
//
// Plain C++ (tests/host_unit/kde_multi_plan_unit.cpp compiles it alone); the kernels include it for the table and the search.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GARLIC_KDE_PLAN_FN __host__ __device__ inline
#else
#define GARLIC_KDE_PLAN_FN inline
#endif

namespace garlic_host {

constexpr int KDE_MULTI_MAX_FEEDS = 32;       // GARLIC_KDE_MAX_FEEDS
constexpr int KDE_MULTI_CHUNK = 2048;         // garlic::KDE_CHUNK
constexpr int KDE_MULTI_MAX_SLICES = 2048;    // garlic::KDE_MAX_SLICES
constexpr int64_t KDE_MULTI_MAX_GRID = 0x7fffffff;

// exclusive prefix sums over the feeds, by value into the kernels
struct KdeMultiFirst {
    int64_t at[KDE_MULTI_MAX_FEEDS + 1];
};

struct KdeMultiFeedPlan {
    int64_t n;                   // values that take part (0 for a feed of fewer than 2)
    int64_t n_chunks, chunks_per_slice, n_slices;
};

struct KdeMultiPlan {
    int32_t n_feeds;
    KdeMultiFeedPlan feed[KDE_MULTI_MAX_FEEDS];
    KdeMultiFirst chunk_first, slice_first;
    int64_t total_chunks, total_slices;       // the grids of the moment and the sums launches
};

// the feed of flat workgroup b: first.at[f] <= b < first.at[f + 1] (feeds without work are passed over); b < first.at[n_feeds]
GARLIC_KDE_PLAN_FN int kdeMultiFind(const KdeMultiFirst &first, int n_feeds, int64_t b)
{
    int f = 0;
    while (f + 1 < n_feeds && first.at[f + 1] <= b) f++;
    return f;
}

// false: n_feeds out of range, or more chunks than one launch holds (nothing usable in *plan then).  min_n: the fewest
// values with which a feed takes part
inline bool kdeMultiPlanFrom(const int64_t *n, int n_feeds, int64_t min_n, KdeMultiPlan *plan)
{
    if (n_feeds < 1 || n_feeds > KDE_MULTI_MAX_FEEDS) return false;
    plan->n_feeds = n_feeds;
    int64_t chunks = 0, slices = 0;
    for (int f = 0; f < n_feeds; f++) {
        KdeMultiFeedPlan &p = plan->feed[f];
        p.n = n[f] >= min_n ? n[f] : 0;
        p.n_chunks = p.n / KDE_MULTI_CHUNK + (p.n % KDE_MULTI_CHUNK != 0);
        p.chunks_per_slice = (p.n_chunks + KDE_MULTI_MAX_SLICES - 1) / KDE_MULTI_MAX_SLICES;
        p.n_slices = p.chunks_per_slice ? (p.n_chunks + p.chunks_per_slice - 1) / p.chunks_per_slice : 0;
        plan->chunk_first.at[f] = chunks;
        plan->slice_first.at[f] = slices;
        if (p.n_chunks > KDE_MULTI_MAX_GRID - chunks) return false;
        chunks += p.n_chunks;
        slices += p.n_slices;
    }
    for (int f = n_feeds; f <= KDE_MULTI_MAX_FEEDS; f++) {
        plan->chunk_first.at[f] = chunks;
        plan->slice_first.at[f] = slices;
    }
    plan->total_chunks = chunks;
    plan->total_slices = slices;
    return true;
}

// whole feeds (garlic_feed_kde_multi): a KDE needs 2 values
inline bool kdeMultiPlan(const int64_t *n, int n_feeds, KdeMultiPlan *plan) { return kdeMultiPlanFrom(n, n_feeds, 2, plan); }

// the feeds of one shard (garlic_kde_part_set): a part of one value takes part, the union has the others
inline bool kdePartSetPlan(const int64_t *n, int n_feeds, KdeMultiPlan *plan) { return kdeMultiPlanFrom(n, n_feeds, 1, plan); }

} // namespace garlic_host
