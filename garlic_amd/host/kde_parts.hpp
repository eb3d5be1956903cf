// The host arithmetic of a KDE over a feed that is split into sorted parts (garlic_kde_parts): the exact order statistics
// of the union by a radix descent over garlic_feed_sort's 64-bit key, and the rules that combine the parts' sums.
// Header-only, no GPU: the rank query is a callback, so libgarlic_hip.so (kde_rank_multi_kernel on every set) and
// tests/host_unit/kde_parts_unit.cpp (std::lower_bound, under the sanitizers) run the same lines.  Built with
// -ffp-contract=off like kde_select.hpp: every operation rounds on its own, in the association written.
#ifndef GARLIC_KDE_PARTS_HPP
#define GARLIC_KDE_PARTS_HPP

#include <cstdint>
#include <cstring>
#include <vector>

namespace garlic_host {

constexpr int KDE_DESCENT_ROUNDS = 8;      // one per byte of the key, most significant first
constexpr int KDE_DESCENT_RANKS = 4;       // x[k25], x[k25 + 1], x[k75], x[k75 + 1]
constexpr int KDE_DESCENT_PROBES = KDE_DESCENT_RANKS * 256;

// garlic_feed_sort's key order (include/garlic_hip.h): unsigned order of the keys is ascending order of the doubles
inline uint64_t kdeKey(double v)
{
    uint64_t b;
    std::memcpy(&b, &v, sizeof b);
    return b ^ (b >> 63 ? 0xFFFFFFFFFFFFFFFFull : 0x8000000000000000ull);
}

inline double kdeKeyValue(uint64_t key)
{
    const uint64_t b = key >> 63 ? key ^ 0x8000000000000000ull : ~key;
    double v;
    std::memcpy(&v, &b, sizeof v);
    return v;
}

// round `round` (0 = the most significant byte): probe 256 q + d is rank q's prefix with digit d, the bytes below zero
inline void kdeDescentProbes(const uint64_t *prefix, int round, uint64_t *probes)
{
    const int shift = 8 * (KDE_DESCENT_ROUNDS - 1 - round);
    for (int q = 0; q < KDE_DESCENT_RANKS; q++)
        for (int d = 0; d < 256; d++) probes[256 * q + d] = prefix[q] | (uint64_t)d << shift;
}

// below[256 q + d]: how many values of the union have a key below that probe.  Rank q keeps the largest digit whose
// count is <= rank[q] (digit 0 always qualifies: its probe is the prefix itself, which the round before chose so)
inline void kdeDescentChoose(uint64_t *prefix, int round, const int64_t *rank, const int64_t *below)
{
    const int shift = 8 * (KDE_DESCENT_ROUNDS - 1 - round);
    for (int q = 0; q < KDE_DESCENT_RANKS; q++) {
        int digit = 0;
        for (int d = 1; d < 256; d++)
            if (below[256 * q + d] <= rank[q]) digit = d;
        prefix[q] |= (uint64_t)digit << shift;
    }
}

// The descent for n_feeds unions at once (garlic_kde_parts_multi; garlic_kde_parts with one): feed f has the ranks
// rank[4 f .. 4 f + 4), 0 <= rank < n_f, and gets the values at those 0-based ranks of its union in value[4 f .. 4 f + 4).
// rank_below(probes, m, below) fills below[1024 f + i] with the number of values of union f whose key is below
// probes[1024 f + i] (m = 1024 probes per feed) and returns 0, or an error code that ends the descent and is returned.
// The count of keys below K never decreases with K, and the value at rank r is the largest K with count(K) <= r, so
// choosing the largest qualifying digit byte by byte arrives at it: after the eighth round the key is the value.  One
// rank query per round carries every feed's probes: eight queries in all, not eight per feed (*rounds: the queries
// made).  A feed with active[f] == 0 is carried along: its probes are zeros, its counts are not read, its values are
// not written.  Every feed's probes and choices are kdeDescentProbes and kdeDescentChoose on its own prefixes, so its
// values do not depend on what else is in the batch.
template <class RankBelow>
inline int kdeSelectRanksMulti(int n_feeds, const int64_t *rank, const uint8_t *active, RankBelow rank_below, double *value, int *rounds)
{
    std::vector<uint64_t> prefix((size_t)n_feeds * KDE_DESCENT_RANKS, 0), probes((size_t)n_feeds * KDE_DESCENT_PROBES, 0);
    std::vector<int64_t> below((size_t)n_feeds * KDE_DESCENT_PROBES, 0);
    if (rounds) *rounds = 0;
    for (int round = 0; round < KDE_DESCENT_ROUNDS; round++) {
        for (int f = 0; f < n_feeds; f++)
            if (active[f]) kdeDescentProbes(&prefix[(size_t)f * KDE_DESCENT_RANKS], round, &probes[(size_t)f * KDE_DESCENT_PROBES]);
        const int rc = rank_below(probes.data(), KDE_DESCENT_PROBES, below.data());
        if (rc) return rc;
        if (rounds) ++*rounds;
        for (int f = 0; f < n_feeds; f++)
            if (active[f])
                kdeDescentChoose(&prefix[(size_t)f * KDE_DESCENT_RANKS], round, rank + (size_t)f * KDE_DESCENT_RANKS,
                                 &below[(size_t)f * KDE_DESCENT_PROBES]);
    }
    for (int f = 0; f < n_feeds; f++)
        for (int q = 0; q < KDE_DESCENT_RANKS && active[f]; q++)
            value[(size_t)f * KDE_DESCENT_RANKS + q] = kdeKeyValue(prefix[(size_t)f * KDE_DESCENT_RANKS + q]);
    return 0;
}

// one union: the batch of one
template <class RankBelow>
inline int kdeSelectRanks(const int64_t *rank, RankBelow rank_below, double *value, int *rounds)
{
    const uint8_t active = 1;
    return kdeSelectRanksMulti(1, rank, &active, rank_below, value, rounds);
}

// ((0.0 + s[0]) + s[1]) + ... in part order: the parts' sums, and their sums of squared deviations
inline double kdeCombine(const double *s, int n_parts)
{
    double total = 0.0;
    for (int p = 0; p < n_parts; p++) total = total + s[p];
    return total;
}

// raw[j] = (((0.0 + S_0[j]) + S_1[j]) + ...) / (double)n; sums[p] holds part p's `points` undivided sums
inline void kdeCombineSums(const double *const *sums, int n_parts, int points, int64_t n, double *raw)
{
    for (int j = 0; j < points; j++) {
        double total = 0.0;
        for (int p = 0; p < n_parts; p++) total = total + sums[p][j];
        raw[j] = total / (double)n;
    }
}

} // namespace garlic_host
#endif
