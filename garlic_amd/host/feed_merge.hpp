// The sorted KDE feeds of individual shards merged into one ascending array (LodOptions::feed_sorted): what nrd0's
// gsl_sort (src/garlic-kde.cpp:132) leaves of the whole panel's feed.  Header-only, no GPU: tests/host_unit/feed_merge_unit.cpp
// runs it under the sanitizers.
#ifndef GARLIC_FEED_MERGE_HPP
#define GARLIC_FEED_MERGE_HPP

#include <cstdint>
#include <cstring>
#include <vector>

namespace garlic_host {

// the device sorter's key (include/garlic_hip.h): unsigned order = numeric order, -0.0 before +0.0, total over NaNs
inline uint64_t feedSortKey(double x)
{
    uint64_t b;
    memcpy(&b, &x, sizeof b);
    return b ^ ((b >> 63) ? 0xFFFFFFFFFFFFFFFFull : 0x8000000000000000ull);
}

// parts[k]: sizes[k] doubles, each ascending under feedSortKey (NULL allowed where sizes[k] == 0); out: room for the sum
// of the sizes.  A k-way merge: every output element is the smallest head, ties to the earlier part -- one pass, linear
// in the output for the handful of shards a node has.
inline void mergeSortedFeeds(const std::vector<const double *> &parts, const std::vector<int64_t> &sizes, double *out)
{
    struct Head { const double *p, *end; uint64_t key; };
    std::vector<Head> heads;
    for (size_t k = 0; k < parts.size(); k++)
        if (sizes[k] > 0) heads.push_back(Head{parts[k], parts[k] + sizes[k], feedSortKey(parts[k][0])});
    while (heads.size() > 1) {
        size_t best = 0;
        for (size_t k = 1; k < heads.size(); k++)
            if (heads[k].key < heads[best].key) best = k;
        // the run of the best part that stays below (or level with, for parts in front of) every other head
        uint64_t bound = UINT64_MAX;
        bool inclusive = true;
        for (size_t k = 0; k < heads.size(); k++) {
            if (k == best) continue;
            if (heads[k].key < bound) { bound = heads[k].key; inclusive = k > best; }
            else if (heads[k].key == bound && k < best) inclusive = false;
        }
        Head &h = heads[best];
        do {
            *out++ = *h.p++;
            if (h.p == h.end) break;
            h.key = feedSortKey(*h.p);
        } while (inclusive ? h.key <= bound : h.key < bound);
        if (h.p == h.end) heads.erase(heads.begin() + (long)best);
    }
    if (heads.size() == 1) {
        const size_t n = (size_t)(heads[0].end - heads[0].p);
        memcpy(out, heads[0].p, n * sizeof(double));
    }
}

} // namespace garlic_host
#endif
