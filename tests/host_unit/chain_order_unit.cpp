// CPU unit check of the chain kernel's queue order (garlic_amd/host/chain_order.hpp; no GPU, no library): the order is a
// permutation of the items, the same at every call, never simulated slower than longest first -- on lists of equal
// items, on the run structure of a 22-chromosome panel (three runs per chromosome x sixteen blocks, where packing pays),
// on random lists, and at the sizes where the function leaves the list alone.
#include "../../garlic_amd/host/chain_order.hpp"

#include <iostream>
#include <numeric>
#include <random>

using namespace garlic_host;

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { std::cerr << "FAILED " << __LINE__ << ": " #cond "\n"; return 1; } \
    } while (0)

// longest first, ties in input order: how the lists reach chainOrder
static std::vector<int32_t> longest_first(std::vector<int32_t> len)
{
    std::stable_sort(len.begin(), len.end(), std::greater<int32_t>());
    return len;
}

static int check(const std::vector<int32_t> &len, int workers, double *gain = nullptr)
{
    const std::vector<int> order = chainOrder(len, workers);
    CHECK(order.size() == len.size());
    std::vector<int> seen(len.size(), 0);
    for (int i : order) {
        CHECK(i >= 0 && (size_t)i < len.size());
        seen[(size_t)i]++;
    }
    for (int s : seen) CHECK(s == 1);
    CHECK(chainOrder(len, workers) == order);                       // deterministic
    const std::vector<int32_t> copy(len);
    CHECK(chainOrder(copy, workers) == order);                      // ... a function of the values alone
    std::vector<int> lpt(len.size());
    std::iota(lpt.begin(), lpt.end(), 0);
    if (workers >= 1 && !len.empty()) {
        const double t = chainMakespan(len, order, workers), t_lpt = chainMakespan(len, lpt, workers);
        CHECK(t <= t_lpt);
        if (gain) *gain = 1.0 - t / t_lpt;
    }
    return 0;
}

int main()
{
    // equal items: every count around the workgroups' multiples, short and long items
    for (int workers : {1, 2, 7, 256})
        for (int n : {0, 1, workers - 1, workers, workers + 1, 2 * workers, 4 * workers + 3, 33 * workers})
            for (int32_t l : {1, 100, 50000})
                if (n >= 0 && check(std::vector<int32_t>((size_t)n, l), workers)) return 1;
    // three runs per chromosome (a hole, a centromere) x sixteen blocks on 256 workgroups: the shape the order was made
    // for; the model must see a gain there, or the function does nothing
    {
        std::mt19937 rng(20260101);
        std::vector<int32_t> len;
        for (int c = 0; c < 22; c++) {
            const int32_t n = 20000 + (int32_t)(rng() % 60000);
            const int32_t a = n / 4 + (int32_t)(rng() % (uint32_t)(n / 2)), b = (int32_t)(rng() % (uint32_t)(n - a));
            for (int32_t l : {a, b, n - a - b})
                for (int k = 0; k < 16; k++) len.push_back(std::max<int32_t>(1, l - 99));
        }
        double gain = 0.0;
        if (check(longest_first(len), 256, &gain)) return 1;
        std::cout << "22 x 3 runs x 16 blocks on 256 workgroups: simulated gain " << gain << "\n";
        CHECK(gain > 0.01);
    }
    // random lists
    {
        std::mt19937 rng(7);
        for (int rep = 0; rep < 40; rep++) {
            const int workers = 1 + (int)(rng() % 64);
            std::vector<int32_t> len((size_t)(rng() % 700));
            for (int32_t &l : len) l = 1 + (int32_t)(rng() % ((rep & 1) ? 300 : 40000));
            if (check(longest_first(len), workers)) return 1;
        }
    }
    std::cout << "chain_order_unit ok\n";
    return 0;
}
