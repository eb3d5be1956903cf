// garlic_amd/host/kde_parts.hpp without a device: the radix descent with std::lower_bound on keys as the rank query, and
// the two combination rules.  tests/test_kde_parts_cpu.py builds this under -fsanitize=address,undefined and runs it.
//
//   kde_parts_unit <dir> ...      (for every directory, in order)
//     <dir>/parts.bin   int64 P, then per part: int64 n, n doubles (ascending in key order)
//     <dir>/sums.f64    P * 8 doubles: part p's 8 "sums" (the combination rules run on them)
//   writes <dir>/out.f64: the four order statistics, kdeCombine of every part's first sum, the 8 combined raw values
//   prints "rounds <r>" per directory and "kde_parts_unit ok" at the end
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
    fprintf(stderr, "kde_parts_unit: %s\n", what);
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

static void run(const std::string &dir)
{
    const std::vector<char> raw = slurp(dir + "/parts.bin");
    size_t at = 0;
    auto take = [&](void *to, size_t bytes) {
        if (at + bytes > raw.size()) die("parts.bin is short");
        memcpy(to, raw.data() + at, bytes);
        at += bytes;
    };
    int64_t P = 0;
    take(&P, sizeof P);
    if (P < 1 || P > 64) die("P out of range");
    std::vector<std::vector<uint64_t>> keys((size_t)P);
    std::vector<uint64_t> all;
    for (int64_t p = 0; p < P; p++) {
        int64_t n = 0;
        take(&n, sizeof n);
        if (n < 0) die("negative part size");
        std::vector<double> x((size_t)n);
        if (n) take(x.data(), sizeof(double) * (size_t)n);
        for (double v : x) {
            if (!same_bits(gh::kdeKeyValue(gh::kdeKey(v)), v)) die("key -> value is not the inverse of value -> key");
            keys[(size_t)p].push_back(gh::kdeKey(v));
        }
        if (!std::is_sorted(keys[(size_t)p].begin(), keys[(size_t)p].end())) die("a part is not in key order");
        all.insert(all.end(), keys[(size_t)p].begin(), keys[(size_t)p].end());
    }
    std::sort(all.begin(), all.end());
    const int64_t n = (int64_t)all.size();
    if (n < 2) die("fewer than 2 values");

    int64_t k25, k75;
    double d25, d75;
    gh::kdeQuantileIndex(n, 0.25, &k25, &d25);
    gh::kdeQuantileIndex(n, 0.75, &k75, &d75);
    const int64_t want_at[4] = {k25, k25 + 1, k75, k75 + 1};
    int64_t rank[4];
    for (int q = 0; q < 4; q++) rank[q] = std::min<int64_t>(want_at[q], n - 1);
    int calls = 0;
    auto rank_below = [&](const uint64_t *probes, int m, int64_t *below) {
        if (m != gh::KDE_DESCENT_PROBES) die("a round does not probe 4 x 256 keys");
        calls++;
        for (int i = 0; i < m; i++) {
            below[i] = 0;
            for (const auto &part : keys) below[i] += std::lower_bound(part.begin(), part.end(), probes[i]) - part.begin();
        }
        return 0;
    };
    double stat[4];
    int rounds = -1;
    if (gh::kdeSelectRanks(rank, rank_below, stat, &rounds) != 0) die("the descent failed");
    printf("rounds %d\n", rounds);
    if (rounds != calls) die("rounds is not the number of rank queries");
    for (int q = 0; q < 4; q++)
        if (!same_bits(stat[q], gh::kdeKeyValue(all[(size_t)rank[q]]))) {
            fprintf(stderr, "rank %lld: got %.17g, the sorted union holds %.17g\n", (long long)rank[q], stat[q],
                    gh::kdeKeyValue(all[(size_t)rank[q]]));
            die("an order statistic differs from the sorted union's");
        }
    // an error code of the rank query ends the descent and comes back
    int failing_rounds = -1;
    if (gh::kdeSelectRanks(rank, [&](const uint64_t *, int, int64_t *) { return 7; }, stat + 0, &failing_rounds) != 7 || failing_rounds != 0)
        die("the rank query's error code is not returned");
    if (gh::kdeSelectRanks(rank, rank_below, stat, nullptr) != 0) die("the descent without a rounds pointer failed");

    // the combination rules
    const std::vector<char> sraw = slurp(dir + "/sums.f64");
    const int points = 8;
    if (sraw.size() != sizeof(double) * (size_t)P * points) die("sums.f64 has the wrong size");
    std::vector<double> sums((size_t)P * points);
    memcpy(sums.data(), sraw.data(), sraw.size());
    std::vector<double> first((size_t)P);
    std::vector<const double *> rows((size_t)P);
    for (int64_t p = 0; p < P; p++) {
        first[(size_t)p] = sums[(size_t)p * points];
        rows[(size_t)p] = &sums[(size_t)p * points];
    }
    double out[4 + 1 + points];
    for (int q = 0; q < 4; q++) out[q] = stat[q];
    out[4] = gh::kdeCombine(first.data(), (int)P);
    gh::kdeCombineSums(rows.data(), (int)P, points, n, out + 5);
    FILE *f = fopen((dir + "/out.f64").c_str(), "wb");
    if (!f || fwrite(out, sizeof(double), 4 + 1 + points, f) != (size_t)(4 + 1 + points)) die("cannot write out.f64");
    fclose(f);
}

int main(int argc, char **argv)
{
    if (argc < 2) die("usage: kde_parts_unit <dir> ...");
    for (int i = 1; i < argc; i++) run(argv[i]);
    printf("kde_parts_unit ok\n");
    return 0;
}
