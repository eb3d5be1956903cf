// CPU unit check of the host's k-way merge of sorted shard feeds (garlic_amd/host/feed_merge.hpp; no GPU, no library):
// against std::sort of the concatenation under the same key, bit for bit -- equal values across shards, empty shards,
// one shard, none, -0.0 / +0.0 and infinities.
#include "../../garlic_amd/host/feed_merge.hpp"

#include <algorithm>
#include <cmath>
#include <iostream>
#include <limits>
#include <random>

using namespace garlic_host;

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { std::cerr << "FAILED " << __LINE__ << ": " #cond "\n"; return 1; } \
    } while (0)

static bool by_key(double a, double b) { return feedSortKey(a) < feedSortKey(b); }

static int check(const std::vector<std::vector<double>> &shards)
{
    std::vector<const double *> parts;
    std::vector<int64_t> sizes;
    std::vector<double> all;
    for (const auto &s : shards) {
        CHECK(std::is_sorted(s.begin(), s.end(), by_key));
        parts.push_back(s.empty() ? nullptr : s.data());
        sizes.push_back((int64_t)s.size());
        all.insert(all.end(), s.begin(), s.end());
    }
    std::sort(all.begin(), all.end(), by_key);
    std::vector<double> out(all.size());       // exactly the sum of the sizes: a write past it is the sanitizer's to find
    mergeSortedFeeds(parts, sizes, out.data());
    for (size_t i = 0; i < all.size(); i++) CHECK(feedSortKey(out[i]) == feedSortKey(all[i]));
    return 0;
}

int main()
{
    std::mt19937_64 gen(12345);
    std::normal_distribution<double> normal;
    auto draw = [&](size_t n, bool coarse) {
        std::vector<double> v(n);
        for (auto &x : v) x = coarse ? std::round(normal(gen) * 2.0) / 2.0 : normal(gen);     // coarse: many equal values
        std::sort(v.begin(), v.end(), by_key);
        return v;
    };
    const double inf = std::numeric_limits<double>::infinity();
    if (check({})) return 1;
    if (check({{}, {}})) return 1;
    if (check({draw(1000, false)})) return 1;
    if (check({draw(1000, false), draw(333, false), draw(1, false)})) return 1;
    if (check({{}, draw(500, true), {}, draw(700, true), draw(64, true), {}})) return 1;
    if (check({{1.0, 1.0, 1.0}, {1.0, 1.0}, {0.5, 1.0, 7.0}})) return 1;
    if (check({{-inf, -1.0, -0.0, 0.0, 5e-324, inf}, {-inf, -0.0, -0.0, 0.0, 1.0, inf, inf}, {0.0}})) return 1;
    for (int k = 2; k <= 8; k++) {
        std::vector<std::vector<double>> shards;
        for (int s = 0; s < k; s++) shards.push_back(draw((size_t)(gen() % 400), s % 2));
        if (check(shards)) return 1;
    }
    std::cout << "feed_merge_unit ok\n";
    return 0;
}
