// Single-thread host restatement of GMM::update (src/gmm.cpp:276-331) for timing against garlic_gmm_fit's EM loop:
//   g++ -O3 -ffp-contract=off -o gmm_host_time gmm_host_time.cpp && ./gmm_host_time lengths.f64 K iterations
// Starts from selectSizeClasses' initial guess (host/size_classes.hpp) and prints the milliseconds of `iterations`
// updates and the final log likelihood.
#include "../../garlic_amd/host/size_classes.hpp"

#include <chrono>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <limits>

int main(int argc, char **argv)
{
    if (argc != 4) { std::cerr << "usage: gmm_host_time <lengths.f64> <K> <iterations>\n"; return 2; }
    std::ifstream f(argv[1], std::ios::binary);
    f.seekg(0, std::ios::end);
    std::vector<double> x((size_t)f.tellg() / sizeof(double));
    f.seekg(0);
    f.read(reinterpret_cast<char *>(x.data()), (std::streamsize)(x.size() * sizeof(double)));
    const int K = atoi(argv[2]), iters = atoi(argv[3]);
    const int64_t n = (int64_t)x.size();
    if (n < 1 || K < 1 || K > garlic_host::GMM_MAX_K) return 2;
    double a[8], mean[8], var[8], resp[8], s0[8], s1[8], s2[8];
    garlic_host::sizeClassInit(x.data(), n, K, a, mean, var);
    const double C = -0.5 * std::log(2 * M_PI);
    double L = 0;
    const auto t0 = std::chrono::steady_clock::now();
    for (int it = 0; it < iters; it++) {
        for (int k = 0; k < K; k++) s0[k] = s1[k] = s2[k] = 0;
        L = 0;
        for (int64_t j = 0; j < n; j++) {
            double l_max = -std::numeric_limits<double>::max();
            for (int i = 0; i < K; i++) {
                resp[i] = std::log(a[i]) + (C - 0.5 * std::log(var[i]) - (x[j] - mean[i]) * (x[j] - mean[i]) / (2.0 * var[i]));
                if (resp[i] > l_max) l_max = resp[i];
            }
            double sum = 0;
            for (int i = 0; i < K; i++) sum += std::exp(resp[i] - l_max);
            const double tmp = l_max + std::log(sum);
            L += tmp;
            double den = 0;
            for (int i = 0; i < K; i++) {
                resp[i] = std::exp(resp[i] - tmp);
                den += resp[i];
            }
            for (int k = 0; k < K; k++) {
                s0[k] += resp[k] / den;
                s1[k] += x[j] * resp[k] / den;
                s2[k] += x[j] * x[j] * resp[k] / den;
            }
        }
        for (int k = 0; k < K; k++) {
            a[k] = s0[k] / double(n);
            mean[k] = s1[k] / s0[k];
            var[k] = s2[k] / s0[k] - mean[k] * mean[k];
        }
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    printf("host n=%lld K=%d iterations=%d ms=%.3f ms_per_iteration=%.4f loglik=%.17g\n", (long long)n, K, iters, ms, ms / iters, L);
    return 0;
}
