// The host arithmetic around the device KDE (garlic_feed_kde): nrd0's bandwidth from the moments and order statistics,
// the 512 targets, the normalisation (computeKDE, src/garlic-kde.cpp:14-140), and what the reference does with the
// density afterwards: the LOD cutoff (get_min_btw_modes, :142-234), the smoothness figure of --auto-winsize
// (calculateWiggle, :3-12) and the .kde file (writeKDEResult).  Header-only, no GPU: libgarlic_hip.so, the host tool and
// tests/host_unit/kde_select_unit.cpp (under the sanitizers) compile the same lines.  Every translation unit that
// includes it is built with -ffp-contract=off: each operation below rounds on its own, in the association written.
#ifndef GARLIC_KDE_SELECT_HPP
#define GARLIC_KDE_SELECT_HPP

#include <cmath>
#include <cstdint>
#include <fstream>
#include <limits>
#include <string>
#include <vector>

namespace garlic_host {

constexpr int KDE_POINTS = 512;      // computeKDE's M (GARLIC_KDE_POINTS)
constexpr double KDE_CUT = 3.0;      // ... and CUT
constexpr int KDE_MODE_WINDOW = 20;  // get_min_btw_modes' and calculateWiggle's window

// gsl_stats_quantile_from_sorted_data: the value lies between x[k] and x[k + 1] with weight delta on the latter
inline void kdeQuantileIndex(int64_t n, double f, int64_t *k, double *delta)
{
    const double idx = f * (double)(n - 1);
    *k = (int64_t)idx;
    *delta = idx - (double)*k;
}

inline double kdeQuantileMix(double xk, double xk1, double delta) { return (1 - delta) * xk + delta * xk1; }

inline double kdeQuantileSorted(const double *x, int64_t n, double f)
{
    int64_t k;
    double delta;
    kdeQuantileIndex(n, f, &k, &delta);
    return k >= n - 1 ? x[n - 1] : kdeQuantileMix(x[k], x[k + 1], delta);
}

// nrd0 (:130-139) behind the sort: sd = sqrt(ssq / (n - 1)) comes from the caller
inline double kdeBandwidth(double sd, double q25, double q75, int64_t n)
{
    const double iqr = q75 - q25;
    const double lo = sd < iqr / 1.34 ? sd : iqr / 1.34;
    return 0.9 * lo * pow((double)n, -0.2);
}

// the targets (:44-68) for the feed's ends lo = x[0], hi = x[n - 1]
inline void kdeTargets(double lo, double hi, double h, double *t)
{
    double max = hi, min = lo;
    max += KDE_CUT * h;
    min -= KDE_CUT * h;
    for (int i = 0; i < KDE_POINTS; i++) t[i] = (double(i + 1) / double(KDE_POINTS)) * (max - min) + min;
}

// :70, :86-95: the sum in index order, every point over (sum * spacing)
inline void kdeNormalise(const double *raw, const double *t, double *y)
{
    const double spacing = t[1] - t[0];
    double sum = 0;
    for (int i = 0; i < KDE_POINTS; i++) sum += raw[i];
    for (int i = 0; i < KDE_POINTS; i++) y[i] = raw[i] / (sum * spacing);
}

// get_arg_max with its starting value: the smallest positive normal double, so a window without a larger entry has no
// maximum (-1)
inline int kdeArgMax(const double *v, int len)
{
    double best = std::numeric_limits<double>::min();
    int at = -1;
    for (int i = 0; i < len; i++)
        if (best < v[i]) { best = v[i]; at = i; }
    return at;
}

inline int kdeArgMin(const double *v, int len)
{
    double best = std::numeric_limits<double>::max();
    int at = -1;
    for (int i = 0; i < len; i++)
        if (best > v[i]) { best = v[i]; at = i; }
    return at;
}

// get_min_btw_modes restated.  The density's maximum over every window of 20 points is taken; runs of equal maxima are
// counted; the two largest counts name the modes and the cutoff is x at the smallest y between them.  Kept as the
// reference has them: the branch for window 1 (it overwrites slot 1 whatever the current slot is), the `<=` in both
// "largest two" scans (a tie moves the older value down), the last index winning where y equals a mode's height, the
// counts compared as truncated integers, and the final |x / wsize| < 1 test (else 0).  Where the reference would read
// or write outside an array -- a window without a maximum at the front (y[-1]), a run slot past the end, a mode height
// that no y[i] equals (index -1), an empty stretch between the modes -- this returns false and says which in *err; the
// reference has undefined behaviour there.
inline bool kdeMinBetweenModes(const double *x, const double *y, int size, int wsize, double *cutoff, int *min_index,
                               std::string *err)
{
    auto bad = [&](const char *what) { if (err) *err = what; return false; };
    const int win = KDE_MODE_WINDOW;
    const int n = size - win;
    if (n < 1) return bad("fewer density points than one window of 20");
    std::vector<double> run_max((size_t)n, 0.0), run_count((size_t)n, 0.0);
    int slot = 0;
    for (int i = 0; i < n; i++) {
        const int at = kdeArgMax(y + i, win) + i;
        if (at < 0) return bad("the first window of the density has no positive entry");
        const double m = y[at];         // (a later window without one: at = i - 1, the point in front of it, as the reference reads)
        if (i == 1) {
            run_max[1] = m;
            run_count[1]++;
        } else if (run_max[(size_t)slot] == m) {
            run_count[(size_t)slot]++;
        } else {
            if (++slot >= n) return bad("more runs of maxima than windows");
            run_max[(size_t)slot] = m;
            run_count[(size_t)slot]++;
        }
    }
    int most = (int)run_count[0], second = 0;
    for (int i = 1; i < n; i++) {
        if (most <= run_count[(size_t)i]) { second = most; most = (int)run_count[(size_t)i]; }
        else if (second <= run_count[(size_t)i]) second = (int)run_count[(size_t)i];
    }
    double first_max = -1, second_max = -1;
    for (int i = 0; i < n; i++)
        if (most == run_count[(size_t)i] || second == run_count[(size_t)i]) {
            const double v = run_max[(size_t)i];
            if (first_max <= v) { second_max = first_max; first_max = v; }
            else if (second_max <= v) second_max = v;
        }
    int left = -1, right = -1;
    for (int i = 0; i < size; i++) {
        if (y[i] == first_max) left = i;
        if (y[i] == second_max) right = i;
    }
    if (left < 0 || right < 0) return bad("a mode's height equals no density point");
    if (right < left) { const int t = right; right = left; left = t; }
    const int rel = kdeArgMin(y + left, right - left + 1);
    if (rel < 0) return bad("no minimum between the modes");
    const int at = rel + left;
    if (min_index) *min_index = at;
    *cutoff = std::fabs(x[at] / wsize) < 1 ? x[at] : 0.0;
    return true;
}

// calculateWiggle: for every start i < size - 20, the residual sum of squares of the least-squares line through the 20
// points (x[i..], 100 * y[i..]) (gsl_fit_linear's sumsq), over 20; summed.  Works on a copy: the reference scales y in
// place, which is why the .kde that its --auto-winsize writes holds 100 * y (the caller of writeKde scales).
inline double kdeWiggle(const double *x, const double *y, int size)
{
    const int win = KDE_MODE_WINDOW;
    double tot = 0;
    for (int i = 0; i < size - win; i++) {
        double mx = 0, my = 0;
        for (int j = 0; j < win; j++) { mx += x[i + j]; my += 100 * y[i + j]; }
        mx /= win;
        my /= win;
        double sxx = 0, sxy = 0;
        for (int j = 0; j < win; j++) {
            const double dx = x[i + j] - mx, dy = 100 * y[i + j] - my;
            sxx += dx * dx;
            sxy += dx * dy;
        }
        const double slope = sxy / sxx;
        double rss = 0;
        for (int j = 0; j < win; j++) {
            const double dx = x[i + j] - mx, dy = 100 * y[i + j] - my;
            const double r = dy - slope * dx;
            rss += r * r;
        }
        tot += rss / double(win);
    }
    return tot;
}

// writeKDEResult: "x y" per line, default ostream formatting (six significant digits).  (The file of the --auto-winsize
// path holds 100 * y, see kdeWiggle: its caller scales.)
inline bool writeKde(const std::string &path, const double *x, const double *y, int size)
{
    std::ofstream f(path.c_str());
    if (!f) return false;
    for (int i = 0; i < size; i++) f << x[i] << " " << y[i] << "\n";
    f.close();
    return !f.fail();
}

} // namespace garlic_host
#endif
