// What selectSizeClasses (src/garlic-roh.cpp:935-1003) does around the EM fit of the ROH lengths (garlic_gmm_fit runs the
// fit itself on the device): the initial guess from the lengths' mean and variance, the classes ordered by mean, the
// boundary between neighbouring classes (BoundFinder, src/BoundFinder.cpp: the root of the difference of the two weighted
// densities between their means) and the two kinds of log lines.  Header-only, no GPU: the host library, the tool and
// tests/host_unit/size_classes_unit.cpp (under the sanitizers) compile the same lines.  Every translation unit that
// includes it is built with -ffp-contract=off.
#ifndef GARLIC_SIZE_CLASSES_HPP
#define GARLIC_SIZE_CLASSES_HPP

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace garlic_host {

constexpr int GMM_MAX_K = 8;               // GARLIC_GMM_MAX_K
constexpr int GMM_MAX_ITER = 1000;         // selectSizeClasses' maxIter
constexpr double GMM_PRECISION = 1e-5;     // ... and tolerance
constexpr int BOUND_MAX_ITER = 1000;       // BoundFinder's maxIt
constexpr double BOUND_EPSREL = 1e-4;      // ... and err

// gsl_stats_mean: the running mean in long double
inline double sizeMean(const double *x, int64_t n)
{
    long double mean = 0;
    for (int64_t i = 0; i < n; i++) mean += (x[i] - mean) / (i + 1);
    return (double)mean;
}

// gsl_stats_variance: the running mean of (x - mean)^2 in long double around the double mean, times n / (n - 1)
// (n = 1: 0 * inf, a NaN, as in the reference)
inline double sizeVariance(const double *x, int64_t n)
{
    const double mean = sizeMean(x, n);
    long double variance = 0;
    for (int64_t i = 0; i < n; i++) {
        const long double delta = x[i] - mean;
        variance += (delta * delta - variance) / (i + 1);
    }
    const double v = (double)variance;
    return v * ((double)n / (double)(n - 1));
}

// :953-960: equal weights, means at mu (n + 1) / (K + 1), variances var (n + 1) / K
inline void sizeClassInit(const double *x, int64_t n, int K, double *a, double *mean, double *var)
{
    const double v = sizeVariance(x, n), mu = sizeMean(x, n);
    for (int k = 0; k < K; k++) {
        a[k] = 1.0 / double(K);
        mean[k] = mu * double(k + 1) / double(K + 1);
        var[k] = v * (k + 1) / double(K);
    }
}

// gsl_sort_index of the means: order[i] is the component with the i-th smallest mean
inline std::vector<int> sizeClassOrder(const double *mean, int K)
{
    std::vector<int> order((size_t)K);
    for (int k = 0; k < K; k++) order[(size_t)k] = k;
    std::stable_sort(order.begin(), order.end(), [&](int p, int q) { return mean[p] < mean[q]; });
    return order;
}

// gsl_ran_gaussian_pdf(x, sigma)
inline double gaussianPdf(double x, double sigma)
{
    const double u = x / std::fabs(sigma);
    return (1 / (std::sqrt(2 * M_PI) * std::fabs(sigma))) * std::exp(-u * u / 2);
}

// BoundFinder::f: class 1's weighted density minus class 2's (the third Gaussian parameter is the variance)
struct BoundFunction {
    double mu1, var1, a1, mu2, var2, a2;
    double operator()(double x) const
    {
        const double s1 = std::sqrt(var1), s2 = std::sqrt(var2);
        return a1 * gaussianPdf(x - mu1, s1) - a2 * gaussianPdf(x - mu2, s2);
    }
};

// Brent-Dekker root bracketing on [lo, hi] (Brent 1973, "zeroin"): b is the best estimate, c the end across the sign
// change, a the previous b; a step is inverse quadratic interpolation (a secant step when only two distinct points are
// known), taken when it falls well inside the bracket and at most halves the step before last, otherwise bisection.
// After every step the bracket [min(b, c), max(b, c)] is tested as gsl_root_test_interval(lo, hi, 0, epsrel) does:
// |hi - lo| < epsrel * min(|lo|, |hi|) (0 when the bracket contains 0).  false with *err set: no sign change between
// the ends, a function value that is not finite, or no convergence in max_iter steps.
template <class F> bool brentRoot(F f, double lo, double hi, double epsrel, int max_iter, double *root, std::string *err)
{
    auto bad = [&](const std::string &what) { if (err) *err = what; return false; };
    double a = lo, b = hi, fa = f(a), fb = f(b);
    if (!std::isfinite(fa) || !std::isfinite(fb)) return bad("the function is not finite at an end of the bracket");
    if ((fa < 0 && fb < 0) || (fa > 0 && fb > 0)) return bad("the ends of the bracket do not straddle 0");
    double c = b, fc = fb, d = 0, e = 0;
    for (int iter = 0; iter < max_iter; iter++) {
        if ((fb < 0 && fc < 0) || (fb > 0 && fc > 0)) {   // the root lies between a and b: c takes a's place
            c = a; fc = fa;
            d = e = b - a;
        }
        if (std::fabs(fc) < std::fabs(fb)) {               // b is to be the end with the smaller value
            a = b; b = c; c = a;
            fa = fb; fb = fc; fc = fa;
        }
        const double tol = 0.5 * DBL_EPSILON * std::fabs(b), m = 0.5 * (c - b);
        if (fb == 0) { *root = b; return true; }
        if (std::fabs(m) <= tol) { *root = b; return true; }
        if (std::fabs(e) < tol || std::fabs(fa) <= std::fabs(fb)) {
            d = e = m;                                       // bisection
        } else {
            double p, q;
            const double s = fb / fa;
            if (a == c) {                                    // secant
                p = 2 * m * s;
                q = 1 - s;
            } else {                                         // inverse quadratic interpolation
                const double qq = fa / fc, r = fb / fc;
                p = s * (2 * m * qq * (qq - r) - (b - a) * (r - 1));
                q = (qq - 1) * (r - 1) * (s - 1);
            }
            if (p > 0) q = -q;
            else p = -p;
            const double bound1 = 3 * m * q - std::fabs(tol * q), bound2 = std::fabs(e * q);
            if (2 * p < (bound1 < bound2 ? bound1 : bound2)) {
                e = d;
                d = p / q;
            } else {
                d = e = m;
            }
        }
        a = b; fa = fb;
        b += std::fabs(d) > tol ? d : (m > 0 ? tol : -tol);
        fb = f(b);
        if (!std::isfinite(fb)) return bad("the function is not finite inside the bracket");
        // the bracket after this step: b and whichever of a (the old b) and c lies across the sign change
        const bool keep_c = !((fb < 0 && fc < 0) || (fb > 0 && fc > 0));
        const double other = keep_c ? c : a;
        const double x_lo = b < other ? b : other, x_hi = b < other ? other : b;
        const double min_abs = (x_lo > 0 && x_hi > 0) || (x_lo < 0 && x_hi < 0) ? std::min(std::fabs(x_lo), std::fabs(x_hi)) : 0.0;
        if (std::fabs(x_hi - x_lo) < epsrel * min_abs || fb == 0) { *root = b; return true; }
    }
    return bad("Root finder failed to converge after " + std::to_string(max_iter) + " iterations.");
}

// :987-996: the boundaries between neighbouring classes of the ordered mixture
inline bool sizeClassBounds(const double *a, const double *mean, const double *var, int K, std::vector<double> *bounds, std::string *err)
{
    const std::vector<int> order = sizeClassOrder(mean, K);
    bounds->clear();
    for (int i = 1; i < K; i++) {
        const int p = order[(size_t)i - 1], q = order[(size_t)i];
        const BoundFunction f{mean[p], var[p], a[p], mean[q], var[q], a[q]};
        const double lo = mean[p] > mean[q] ? mean[q] : mean[p], hi = mean[p] > mean[q] ? mean[p] : mean[q];
        double r = 0;
        std::string why;
        if (!(lo < hi) || !brentRoot(f, lo, hi, BOUND_EPSREL, BOUND_MAX_ITER, &r, &why)) {
            if (err) {
                char buf[256];
                snprintf(buf, sizeof buf, "no boundary between size classes %c (mean %g) and %c (mean %g): %s", (char)('A' + i - 1), mean[p],
                         (char)('A' + i), mean[q], why.empty() ? "the means are equal or not finite" : why.c_str());
                *err = buf;
            }
            return false;
        }
        bounds->push_back(r);
    }
    return true;
}

// "Gaussian class A ( mixture, mean, std ) = ( a, mean, var )" per class in order of the means (the third value is the
// variance: the reference's label is kept), each number as the reference's stream prints it (%g)
inline std::string sizeClassLines(const double *a, const double *mean, const double *var, int K)
{
    const std::vector<int> order = sizeClassOrder(mean, K);
    std::string out;
    for (int i = 0; i < K; i++) {
        const int k = order[(size_t)i];
        char buf[256];
        snprintf(buf, sizeof buf, "Gaussian class %c ( mixture, mean, std ) = ( %g, %g, %g )\n", (char)('A' + i), a[k], mean[k], var[k]);
        out += buf;
    }
    return out;
}

inline std::string sizeBoundsLine(const std::vector<double> &bounds)
{
    std::string out = "Selected ROH size boundaries = (";
    for (double b : bounds) {
        char buf[64];
        snprintf(buf, sizeof buf, " %g", b);
        out += buf;
    }
    return out + " )\n";
}

} // namespace garlic_host
#endif
