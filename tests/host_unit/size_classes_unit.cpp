// garlic_amd/host/size_classes.hpp as a stand-alone program (tests/test_gmm_cpu.py compiles it with ASan + UBSan; nothing is
// loaded into python).  usage: size_classes_unit <dir>
//   <dir>/lengths.f64  ROH lengths               <dir>/params.f64  K, then a[K], mean[K], var[K] of a fitted mixture (any order)
// writes <dir>/out.f64: the initial guess for K classes (a, mean, var: 3 K doubles), the order of the classes by mean (K),
// the K - 1 boundaries; <dir>/out.txt: the Gaussian lines and the boundary line.  Also runs the refusals of the root search.
#include "../../garlic_amd/host/size_classes.hpp"

#include <cstdlib>
#include <fstream>
#include <iostream>

using namespace garlic_host;

static std::vector<double> slurp(const std::string &path)
{
    std::ifstream f(path.c_str(), std::ios::binary);
    if (!f) { std::cerr << "cannot open " << path << "\n"; exit(2); }
    f.seekg(0, std::ios::end);
    const size_t bytes = (size_t)f.tellg();
    f.seekg(0);
    std::vector<double> v(bytes / sizeof(double));
    f.read(reinterpret_cast<char *>(v.data()), (std::streamsize)(v.size() * sizeof(double)));
    return v;
}

#define CHECK(cond) do { if (!(cond)) { std::cerr << "FAILED: " #cond " (line " << __LINE__ << ")\n"; return 1; } } while (0)

int main(int argc, char **argv)
{
    if (argc != 2) { std::cerr << "usage: size_classes_unit <dir>\n"; return 2; }
    const std::string dir = argv[1];
    const std::vector<double> len = slurp(dir + "/lengths.f64"), par = slurp(dir + "/params.f64");
    CHECK(!len.empty() && !par.empty());
    const int K = (int)par[0];
    CHECK(K >= 1 && K <= GMM_MAX_K && (int)par.size() == 1 + 3 * K);
    const double *a = par.data() + 1, *mean = a + K, *var = mean + K;

    std::vector<double> out((size_t)(3 * K));
    sizeClassInit(len.data(), (int64_t)len.size(), K, out.data(), out.data() + K, out.data() + 2 * K);
    for (int k : sizeClassOrder(mean, K)) out.push_back(k);
    std::vector<double> bounds;
    std::string err;
    CHECK(sizeClassBounds(a, mean, var, K, &bounds, &err));
    CHECK((int)bounds.size() == K - 1);
    for (double b : bounds) out.push_back(b);
    {
        std::ofstream f((dir + "/out.f64").c_str(), std::ios::binary);
        f.write(reinterpret_cast<const char *>(out.data()), (std::streamsize)(out.size() * sizeof(double)));
        std::ofstream t((dir + "/out.txt").c_str());
        t << sizeClassLines(a, mean, var, K) << sizeBoundsLine(bounds);
    }

    // one value: the variance is 0 * inf
    const double one = 5.0;
    CHECK(sizeMean(&one, 1) == 5.0 && std::isnan(sizeVariance(&one, 1)));
    // a root the solver must find to the interval test on a function with a known zero
    double r = 0;
    CHECK(brentRoot([](double x) { return x * x * x - 8.0; }, 1.0, 5.0, 1e-4, 1000, &r, &err));
    CHECK(std::fabs(r - 2.0) <= 2e-4 * 2.0);
    CHECK(brentRoot([](double x) { return std::cos(x); }, 1.0, 2.0, 1e-12, 1000, &r, &err) && std::fabs(r - M_PI / 2) < 1e-11);
    // refusals: no sign change, equal means, no convergence within the iterations allowed
    CHECK(!brentRoot([](double x) { return x * x + 1.0; }, -1.0, 1.0, 1e-4, 1000, &r, &err) && err.find("straddle") != std::string::npos);
    CHECK(!brentRoot([](double x) { return x - 0.3; }, 0.0, 1.0, 0.0, 3, &r, &err) || r == 0.3);
    const double a2[2] = {0.5, 0.5}, m2[2] = {10.0, 10.0}, v2[2] = {1.0, 4.0};
    CHECK(!sizeClassBounds(a2, m2, v2, 2, &bounds, &err) && err.find("no boundary between size classes A") == 0);
    const double a3[2] = {0.999, 0.001}, m3[2] = {0.0, 1.0}, v3[2] = {100.0, 100.0};   // class A above class B at both means
    CHECK(!sizeClassBounds(a3, m3, v3, 2, &bounds, &err) && err.find("straddle") != std::string::npos);
    // K = 1: no boundary, one line
    CHECK(sizeClassBounds(a, mean, var, 1, &bounds, &err) && bounds.empty());
    std::cout << "size_classes_unit ok\n";
    return 0;
}
