// garlic_amd/host/kde_select.hpp as a stand-alone program (tests/test_kde_cpu.py compiles it with ASan + UBSan; nothing is
// loaded into python).  usage: kde_select_unit <fixture.kde> <winsize> <dir>
//   <dir>/feed.f64  an ascending feed            <dir>/sd.f64  its standard deviation (one double)
//   <dir>/raw.f64   512 unnormalised sums
// writes <dir>/out.f64: q25, q75, h, the 512 targets, the 512 normalised values, the wiggle of (targets, values), then for
// the fixture: index of the minimum, cutoff, wiggle; <dir>/out.kde and <dir>/out100.kde through writeKde; prints the
// fixture's cutoff under default ostream formatting.
#include "../../garlic_amd/host/kde_select.hpp"

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>

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
    if (argc != 4) { std::cerr << "usage: kde_select_unit <fixture.kde> <winsize> <dir>\n"; return 2; }
    const std::string dir = argv[3];
    const int wsize = atoi(argv[2]);
    std::vector<double> fx, fy;
    {
        std::ifstream f(argv[1]);
        double a, b;
        while (f >> a >> b) { fx.push_back(a); fy.push_back(b); }
    }
    CHECK((int)fx.size() == KDE_POINTS);

    const std::vector<double> feed = slurp(dir + "/feed.f64"), sd = slurp(dir + "/sd.f64"), raw = slurp(dir + "/raw.f64");
    CHECK(feed.size() >= 2 && sd.size() == 1 && (int)raw.size() == KDE_POINTS);
    const int64_t n = (int64_t)feed.size();
    std::vector<double> out;
    const double q25 = kdeQuantileSorted(feed.data(), n, 0.25), q75 = kdeQuantileSorted(feed.data(), n, 0.75);
    const double h = kdeBandwidth(sd[0], q25, q75, n);
    std::vector<double> t(KDE_POINTS), y(KDE_POINTS);
    kdeTargets(feed.front(), feed.back(), h, t.data());
    kdeNormalise(raw.data(), t.data(), y.data());
    out.push_back(q25); out.push_back(q75); out.push_back(h);
    out.insert(out.end(), t.begin(), t.end());
    out.insert(out.end(), y.begin(), y.end());
    const std::vector<double> y_before(y);
    out.push_back(kdeWiggle(t.data(), y.data(), KDE_POINTS));
    CHECK(y == y_before);                                   // works on a copy
    CHECK(writeKde(dir + "/out.kde", t.data(), y.data(), KDE_POINTS));
    std::vector<double> y100(y);
    for (double &v : y100) v = v * 100.0;
    CHECK(writeKde(dir + "/out100.kde", t.data(), y100.data(), KDE_POINTS));
    CHECK(!writeKde(dir + "/no/such/dir/out.kde", t.data(), y.data(), KDE_POINTS));

    // the quantile at the ends and for two values
    const double two[2] = {1.0, 3.0};
    CHECK(kdeQuantileSorted(two, 2, 0.25) == 1.5 && kdeQuantileSorted(two, 2, 0.75) == 2.5 && kdeQuantileSorted(two, 2, 1.0) == 3.0);

    // the fixture: the reference's own example output and the cutoff its log records
    double cutoff = 0;
    int at = -1;
    std::string err;
    CHECK(kdeMinBetweenModes(fx.data(), fy.data(), KDE_POINTS, wsize, &cutoff, &at, &err));
    out.push_back((double)at); out.push_back(cutoff); out.push_back(kdeWiggle(fx.data(), fy.data(), KDE_POINTS));
    std::cout << "cutoff " << cutoff << "\n";
    // |x / wsize| >= 1: 0
    double c1 = -1;
    CHECK(kdeMinBetweenModes(fx.data(), fy.data(), KDE_POINTS, 1, &c1, nullptr, nullptr) && c1 == 0.0);

    // where the reference leaves its arrays: an error, and nothing outside ours is touched (the sanitizers watch)
    std::vector<double> zeros(KDE_POINTS, 0.0), flat(KDE_POINTS, 0.25), ramp(KDE_POINTS);
    for (int i = 0; i < KDE_POINTS; i++) ramp[(size_t)i] = 1.0 + i;
    double c = 7;
    CHECK(!kdeMinBetweenModes(fx.data(), zeros.data(), KDE_POINTS, wsize, &c, nullptr, &err) && !err.empty() && c == 7);
    CHECK(!kdeMinBetweenModes(fx.data(), fy.data(), KDE_MODE_WINDOW, wsize, &c, nullptr, &err) && c == 7);
    CHECK(!kdeMinBetweenModes(fx.data(), flat.data(), KDE_POINTS, wsize, &c, nullptr, &err) && c == 7);   // one run: no second mode
    bool ok = kdeMinBetweenModes(fx.data(), ramp.data(), KDE_POINTS, wsize, &c, &at, &err);                 // every window a new maximum
    CHECK(!ok || (at >= 0 && at < KDE_POINTS));
    // zeros in front of the mass (a window without a maximum past the first one reads the point in front of it)
    std::vector<double> lead(fy);
    for (int i = 30; i < 60; i++) lead[(size_t)i] = 0.0;
    ok = kdeMinBetweenModes(fx.data(), lead.data(), KDE_POINTS, wsize, &c, &at, &err);
    CHECK(!ok || (at >= 0 && at < KDE_POINTS));

    std::ofstream f((dir + "/out.f64").c_str(), std::ios::binary);
    f.write(reinterpret_cast<const char *>(out.data()), (std::streamsize)(out.size() * sizeof(double)));
    f.close();
    CHECK(!f.fail());
    std::cout << "kde_select_unit ok\n";
    return 0;
}
