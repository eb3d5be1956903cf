// garlic_amd/host/kde_parts.hpp without a device: the descent for F feeds at once (kdeSelectRanksMulti) against the
// single-feed kdeSelectRanks (the same descent as a batch of one: what else is in the batch changes nothing) and against
// the sorted union (the independent check), with std::lower_bound on keys as the rank query.
// tests/test_kde_parts_multi_cpu.py builds this under -fsanitize=address,undefined and runs it.
//
//   kde_parts_multi_unit <file> ...      (every file is one batch, in order)
//     <file>   int64 F, then per feed: int64 active, int64 P, then per part: int64 n, n doubles (ascending in key order)
//   an active feed's union holds at least 2 values; a feed that is not active may hold anything
//   prints "feeds <F> rounds <r>" per batch and "kde_parts_multi_unit ok" at the end
//
// Per batch: every active feed's four values equal kdeSelectRanks's on that feed alone and the sorted union's, bit for
// bit; the batch makes 8 rank queries of F x 1024 probes; with every second active feed switched off the others' values
// do not change and nothing is written for the ones that are off.
#include "../../garlic_amd/host/kde_select.hpp"
#include "../../garlic_amd/host/kde_parts.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace gh = garlic_host;

static void die(const char *what)
{
    fprintf(stderr, "kde_parts_multi_unit: %s\n", what);
    exit(1);
}

static std::vector<char> slurp(const std::string &path)
{
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) die(("cannot open " + path).c_str());
    std::vector<char> buf;
    char tmp[1 << 16];
    size_t got;
    while ((got = fread(tmp, 1, sizeof tmp, f)) > 0) buf.insert(buf.end(), tmp, tmp + got);
    fclose(f);
    return buf;
}

static bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof a) == 0; }

struct Feed {
    bool active = false;
    std::vector<std::vector<uint64_t>> parts;      // keys
    std::vector<uint64_t> all;                     // the sorted union
    int64_t rank[4] = {0, 0, 0, 0};
};

static int64_t below_of(const Feed &f, uint64_t probe)
{
    int64_t below = 0;
    for (const auto &part : f.parts) below += std::lower_bound(part.begin(), part.end(), probe) - part.begin();
    return below;
}

static void run(const std::string &path)
{
    const std::vector<char> raw = slurp(path);
    size_t at = 0;
    auto take = [&](void *to, size_t bytes) {
        if (at + bytes > raw.size()) die("the batch file is short");
        memcpy(to, raw.data() + at, bytes);
        at += bytes;
    };
    int64_t F = 0;
    take(&F, sizeof F);
    if (F < 1 || F > 32) die("F out of range");
    std::vector<Feed> feeds((size_t)F);
    for (Feed &f : feeds) {
        int64_t active = 0, P = 0;
        take(&active, sizeof active);
        take(&P, sizeof P);
        if (P < 1 || P > 64) die("P out of range");
        f.active = active != 0;
        f.parts.resize((size_t)P);
        for (auto &part : f.parts) {
            int64_t n = 0;
            take(&n, sizeof n);
            if (n < 0) die("negative part size");
            std::vector<double> x((size_t)n);
            if (n) take(x.data(), sizeof(double) * (size_t)n);
            for (double v : x) part.push_back(gh::kdeKey(v));
            if (!std::is_sorted(part.begin(), part.end())) die("a part is not in key order");
            f.all.insert(f.all.end(), part.begin(), part.end());
        }
        std::sort(f.all.begin(), f.all.end());
        const int64_t n = (int64_t)f.all.size();
        if (!f.active) continue;
        if (n < 2) die("an active feed holds fewer than 2 values");
        int64_t k25, k75;
        double d25, d75;
        gh::kdeQuantileIndex(n, 0.25, &k25, &d25);
        gh::kdeQuantileIndex(n, 0.75, &k75, &d75);
        const int64_t want_at[4] = {k25, k25 + 1, k75, k75 + 1};
        for (int q = 0; q < 4; q++) f.rank[q] = std::min<int64_t>(want_at[q], n - 1);
    }

    const double untouched = -12345.5;
    auto descend = [&](const std::vector<uint8_t> &active, std::vector<double> &value, int *rounds) {
        std::vector<int64_t> rank((size_t)F * 4);
        for (int64_t f = 0; f < F; f++)
            for (int q = 0; q < 4; q++) rank[(size_t)f * 4 + q] = feeds[(size_t)f].rank[q];
        value.assign((size_t)F * 4, untouched);
        int calls = 0;
        const int rc = gh::kdeSelectRanksMulti((int)F, rank.data(), active.data(), [&](const uint64_t *probes, int m, int64_t *below) {
            if (m != gh::KDE_DESCENT_PROBES) die("a round does not probe 4 x 256 keys per feed");
            calls++;
            for (int64_t f = 0; f < F; f++) {
                if (!active[(size_t)f]) {                  // what comes back for a feed that is off must not matter
                    for (int i = 0; i < m; i++) below[(size_t)f * m + i] = -7 - i;
                    continue;
                }
                for (int i = 0; i < m; i++) below[(size_t)f * m + i] = below_of(feeds[(size_t)f], probes[(size_t)f * m + i]);
            }
            return 0;
        }, value.data(), rounds);
        if (rc) die("the descent failed");
        if (*rounds != calls) die("rounds is not the number of rank queries");
    };

    std::vector<uint8_t> active((size_t)F);
    for (int64_t f = 0; f < F; f++) active[(size_t)f] = feeds[(size_t)f].active;
    std::vector<double> value;
    int rounds = -1;
    descend(active, value, &rounds);
    printf("feeds %lld rounds %d\n", (long long)F, rounds);
    if (rounds != gh::KDE_DESCENT_ROUNDS) die("not 8 rounds in all");
    for (int64_t f = 0; f < F; f++) {
        const Feed &feed = feeds[(size_t)f];
        const double *got = &value[(size_t)f * 4];
        if (!feed.active) {
            for (int q = 0; q < 4; q++)
                if (!same_bits(got[q], untouched)) die("a value of a feed that is off was written");
            continue;
        }
        double single[4];
        int single_rounds = -1;
        if (gh::kdeSelectRanks(feed.rank, [&](const uint64_t *probes, int m, int64_t *below) {
                for (int i = 0; i < m; i++) below[i] = below_of(feed, probes[i]);
                return 0;
            }, single, &single_rounds) != 0 || single_rounds != gh::KDE_DESCENT_ROUNDS)
            die("the single-feed descent failed");
        for (int q = 0; q < 4; q++) {
            if (!same_bits(got[q], single[q])) {
                fprintf(stderr, "feed %lld rank %lld: %.17g in the batch, %.17g alone\n", (long long)f, (long long)feed.rank[q], got[q], single[q]);
                die("a feed's value in the batch differs from kdeSelectRanks's");
            }
            if (!same_bits(got[q], gh::kdeKeyValue(feed.all[(size_t)feed.rank[q]]))) die("an order statistic differs from the sorted union's");
        }
    }
    // every second active feed off: the others keep their values
    std::vector<uint8_t> fewer = active;
    bool off = true;
    for (int64_t f = 0; f < F; f++)
        if (fewer[(size_t)f]) {
            if (off) fewer[(size_t)f] = 0;
            off = !off;
        }
    std::vector<double> again;
    int rounds_again = -1;
    descend(fewer, again, &rounds_again);
    if (rounds_again != gh::KDE_DESCENT_ROUNDS) die("not 8 rounds with feeds switched off");
    for (int64_t f = 0; f < F; f++)
        for (int q = 0; q < 4; q++)
            if (!same_bits(again[(size_t)f * 4 + q], fewer[(size_t)f] ? value[(size_t)f * 4 + q] : untouched))
                die("switching feeds off changed another feed's value, or wrote one that is off");
    // an error code of the rank query ends the descent and comes back
    int failing = -1;
    std::vector<int64_t> rank((size_t)F * 4, 0);
    if (gh::kdeSelectRanksMulti((int)F, rank.data(), active.data(), [&](const uint64_t *, int, int64_t *) { return 7; }, again.data(), &failing) != 7 ||
        failing != 0)
        die("the rank query's error code is not returned");
}

int main(int argc, char **argv)
{
    if (argc < 2) die("usage: kde_parts_multi_unit <file> ...");
    for (int i = 1; i < argc; i++) run(argv[i]);
    printf("kde_parts_multi_unit ok\n");
    return 0;
}
