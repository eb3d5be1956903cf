// Stand-alone check of garlic_amd/host/kde_multi_plan.hpp (tests/test_kde_multi_cpu.py builds it with the sanitizers):
// reads lists of feed lengths, one list per line on stdin, and for each list walks every workgroup of the moment and the
// sums launch through kdeMultiFind, marking what it covers in arrays of the plan's own size -- so a workgroup mapped
// outside its feed, or two feeds laid over each other, is an out-of-bounds or a double mark.
//   output per list: "feeds F chunks C slices S" then per feed "n chunks cps slices chunk_off slice_off"
#include <cstdio>
#include <cstdlib>
#include <sstream>
#include <string>
#include <iostream>
#include <vector>

#include "../../garlic_amd/host/kde_multi_plan.hpp"

namespace gh = garlic_host;

static int check_list(const std::vector<int64_t> &n)
{
    gh::KdeMultiPlan plan;
    if (!gh::kdeMultiPlan(n.data(), (int)n.size(), &plan)) {
        printf("refused\n");
        return 0;
    }
    printf("feeds %d chunks %lld slices %lld\n", plan.n_feeds, (long long)plan.total_chunks, (long long)plan.total_slices);
    // who owns every per-chunk entry and every row of slice sums: -1 nobody yet
    std::vector<int> chunk_owner((size_t)plan.total_chunks, -1), slice_owner((size_t)plan.total_slices, -1);
    std::vector<int64_t> chunk_seen((size_t)plan.n_feeds, 0), slice_seen((size_t)plan.n_feeds, 0), in_slices((size_t)plan.n_feeds, 0);
    for (int64_t b = 0; b < plan.total_chunks; b++) {
        const int f = gh::kdeMultiFind(plan.chunk_first, plan.n_feeds, b);
        const int64_t chunk = b - plan.chunk_first.at[f];
        if (f < 0 || f >= plan.n_feeds || chunk < 0 || chunk >= plan.feed[f].n_chunks) {
            fprintf(stderr, "workgroup %lld of the moment launch: feed %d chunk %lld\n", (long long)b, f, (long long)chunk);
            return 1;
        }
        if (chunk * gh::KDE_MULTI_CHUNK >= plan.feed[f].n) { fprintf(stderr, "feed %d: chunk %lld begins past the feed\n", f, (long long)chunk); return 1; }
        int &owner = chunk_owner.at((size_t)(plan.chunk_first.at[f] + chunk));
        if (owner != -1) { fprintf(stderr, "chunk entry %lld taken twice\n", (long long)b); return 1; }
        owner = f;
        chunk_seen[(size_t)f]++;
    }
    for (int64_t b = 0; b < plan.total_slices; b++) {
        const int f = gh::kdeMultiFind(plan.slice_first, plan.n_feeds, b);
        const int64_t slice = b - plan.slice_first.at[f];
        if (f < 0 || f >= plan.n_feeds || slice < 0 || slice >= plan.feed[f].n_slices) {
            fprintf(stderr, "workgroup %lld of the sums launch: feed %d slice %lld\n", (long long)b, f, (long long)slice);
            return 1;
        }
        int &owner = slice_owner.at((size_t)(plan.slice_first.at[f] + slice));
        if (owner != -1) { fprintf(stderr, "slice row %lld taken twice\n", (long long)b); return 1; }
        owner = f;
        slice_seen[(size_t)f]++;
        // the slice's chunks, as the sums kernel walks them
        const int64_t c0 = slice * plan.feed[f].chunks_per_slice;
        const int64_t c1 = c0 + plan.feed[f].chunks_per_slice < plan.feed[f].n_chunks ? c0 + plan.feed[f].chunks_per_slice : plan.feed[f].n_chunks;
        if (c1 <= c0) { fprintf(stderr, "feed %d: slice %lld is empty\n", f, (long long)slice); return 1; }
        in_slices[(size_t)f] += c1 - c0;
    }
    for (int f = 0; f < plan.n_feeds; f++) {
        const gh::KdeMultiFeedPlan &p = plan.feed[f];
        if (chunk_seen[(size_t)f] != p.n_chunks || slice_seen[(size_t)f] != p.n_slices || in_slices[(size_t)f] != p.n_chunks) {
            fprintf(stderr, "feed %d: %lld of %lld chunks, %lld of %lld slices, %lld chunks in slices\n", f, (long long)chunk_seen[(size_t)f],
                    (long long)p.n_chunks, (long long)slice_seen[(size_t)f], (long long)p.n_slices, (long long)in_slices[(size_t)f]);
            return 1;
        }
        if (p.n_slices > gh::KDE_MULTI_MAX_SLICES) { fprintf(stderr, "feed %d: %lld slices\n", f, (long long)p.n_slices); return 1; }
        printf("%lld %lld %lld %lld %lld %lld\n", (long long)p.n, (long long)p.n_chunks, (long long)p.chunks_per_slice, (long long)p.n_slices,
               (long long)plan.chunk_first.at[f], (long long)plan.slice_first.at[f]);
    }
    for (int f = plan.n_feeds; f <= gh::KDE_MULTI_MAX_FEEDS; f++)
        if (plan.chunk_first.at[f] != plan.total_chunks || plan.slice_first.at[f] != plan.total_slices) {
            fprintf(stderr, "the tables are not padded with the totals at %d\n", f);
            return 1;
        }
    return 0;
}

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::vector<int64_t> n;
        long long v;
        while (in >> v) n.push_back(v);
        if (check_list(n)) return 1;
    }
    printf("kde_multi_plan_unit ok\n");
    return 0;
}
