// The order in which lod_chain_kernel's persistent workgroups pull their items, chosen by simulating the queue.
// Header-only, no GPU: garlic_hip.hip (plan_lod) and tests/host_unit/chain_order_unit.cpp compile the same lines.
//
// The model of one pass.  An item is a run of valid windows x one 64-individual block; a workgroup (one per CU) that
// has finished its item pulls the next one of the list.  An item of `len` windows takes
//     CHAIN_ITEM_US + len / CHAIN_WINDOWS_PER_US   microseconds,
// both constants from the per-item stamps of the 1M x 1000, W = 100 pass (profiles/chain_onepass_ab.txt, "item stamps"):
//   * the pace is the CHAIN wave's, alone on its CU: 48.7 windows/us inside the loop with all 256 CUs storing and 45
//     with 99 of them left, so the HBM share of the active CUs is not in the model -- it never binds before the cap does;
//   * the rows of the block are not in it either: the last block's 40-row items run at 50.3 windows/us, a full item's time;
//   * least squares of (end - begin) over the 1056 items: 17.2 us + len / 49.6 (of the 17.2 the prologue up to the first
//     loop tile is 12.2, the rest the loop's fill and drain and the tail tile).  Replaying the measured durations through
//     this queue gives the measured end within 3 us, and the model with these constants within 7 us.
// Longest first (LPT) leaves the CUs going idle over 77 us there (40 us each on average, 3 % of the pass): the runs come
// in groups of equal items, one per block, and the middle-sized groups are handed out too late for the few short ones to
// level.  MULTIFIT (first-fit decreasing into one bin per workgroup, bisection on the bin size) packs the same whole items
// to within 0.5 % of the balanced load; the list is then that packing read by planned start time, which is the order a
// queue replays it in.  Under the scatter the stamps show (2 % of an item's time) about half of the gain survives, so the
// packing is taken only where the model sees more than 1 % in it; elsewhere the list stays longest first.
#ifndef GARLIC_CHAIN_ORDER_HPP
#define GARLIC_CHAIN_ORDER_HPP

#include <algorithm>
#include <cstdint>
#include <functional>
#include <queue>
#include <utility>
#include <vector>

namespace garlic_host {

constexpr double CHAIN_ITEM_US = 17.2;              // profiles/chain_onepass_ab.txt
constexpr double CHAIN_WINDOWS_PER_US = 49.6;       // profiles/chain_onepass_ab.txt

inline double chainItemUs(int32_t len) { return CHAIN_ITEM_US + (double)len / CHAIN_WINDOWS_PER_US; }

// the pass simulated: `workers` workgroups pull the items of `order` (indices into len) from one queue; the time the last one ends
inline double chainMakespan(const std::vector<int32_t> &len, const std::vector<int> &order, int workers)
{
    typedef std::pair<double, int> Free;      // (time the workgroup is free, workgroup)
    std::priority_queue<Free, std::vector<Free>, std::greater<Free>> heap;
    for (int w = 0; w < workers; w++) heap.push(Free(0.0, w));
    double end = 0.0;
    for (int i : order) {
        Free f = heap.top();
        heap.pop();
        f.first += chainItemUs(len[(size_t)i]);
        end = std::max(end, f.first);
        heap.push(f);
    }
    return end;
}

// The order of the list: a permutation of 0 .. len.size() - 1, a pure function of (len, workers).  `len` is given longest
// first (the order the list has had so far: ties in chromosome and position order), and that is what comes back
// unless the packing is simulated more than 1 % shorter.
inline std::vector<int> chainOrder(const std::vector<int32_t> &len, int workers)
{
    const size_t n = len.size();
    std::vector<int> lpt(n);
    for (size_t i = 0; i < n; i++) lpt[i] = (int)i;
    // (no more items than workgroups: one each; very many: whatever order they finish in, the chip stays full)
    if (workers < 2 || n <= (size_t)workers || n > (size_t)32 * (size_t)workers) return lpt;
    std::vector<int> dec = lpt;
    std::stable_sort(dec.begin(), dec.end(), [&](int x, int y) { return len[(size_t)x] > len[(size_t)y]; });
    const double t_lpt = chainMakespan(len, lpt, workers);
    double sum = 0.0, longest = 0.0;
    for (size_t i = 0; i < n; i++) {
        sum += chainItemUs(len[i]);
        longest = std::max(longest, chainItemUs(len[i]));
    }
    // first-fit decreasing: bin[i] for every item, or false when a bin size of `cap` does not take them all
    std::vector<int> bin(n), best;
    std::vector<double> load((size_t)workers);
    auto ffd = [&](double cap) {
        std::fill(load.begin(), load.end(), 0.0);
        int first_open = 0;
        for (int i : dec) {
            const double c = chainItemUs(len[(size_t)i]);
            int w = first_open;
            while (w < workers && load[(size_t)w] + c > cap) w++;
            if (w == workers) return false;
            load[(size_t)w] += c;
            bin[(size_t)i] = w;
            while (first_open < workers && load[(size_t)first_open] + CHAIN_ITEM_US > cap) first_open++;
        }
        return true;
    };
    double lo = std::max(sum / workers, longest), hi = t_lpt;
    if (!ffd(hi)) return lpt;
    best = bin;
    for (int it = 0; it < 16; it++) {
        const double mid = 0.5 * (lo + hi);
        if (ffd(mid)) {
            hi = mid;
            best = bin;
        } else
            lo = mid;
    }
    // the packing by planned start time: a workgroup's items longest first, so that what it pulls last is its shortest
    struct Slot { double start; int bin, item; };
    std::vector<Slot> slots;
    slots.reserve(n);
    std::fill(load.begin(), load.end(), 0.0);
    for (int i : dec) {
        const int w = best[(size_t)i];
        slots.push_back(Slot{load[(size_t)w], w, i});
        load[(size_t)w] += chainItemUs(len[(size_t)i]);
    }
    std::stable_sort(slots.begin(), slots.end(), [](const Slot &a, const Slot &b) {
        return a.start != b.start ? a.start < b.start : a.bin < b.bin;
    });
    std::vector<int> order(n);
    for (size_t i = 0; i < n; i++) order[i] = slots[i].item;
    return chainMakespan(len, order, workers) < 0.99 * t_lpt ? order : lpt;
}

}  // namespace garlic_host

#endif
