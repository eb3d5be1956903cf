// One thread of std::sort over doubles, timed: the host stand-in of tools/bench_variants.py --modes feed_sort for nrd0's
// gsl_sort (src/garlic-kde.cpp:132; GSL itself is not among this project's dependencies).  Built by the leg with g++ -O2
// -shared and called through ctypes.
#include <algorithm>
#include <chrono>
#include <cstdint>

extern "C" double host_std_sort_seconds(double *x, int64_t n)
{
    const auto t0 = std::chrono::steady_clock::now();
    std::sort(x, x + n);
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}
