"""The data sets of the device GMM fit (garlic_gmm_fit) and a numpy reference of GMM::estimate / GMM::update
(src/gmm.cpp:276-331, 385-442) and of what selectSizeClasses (src/garlic-roh.cpp:935-1003) does around it, written from
the formulas independently of garlic_amd/csrc/gmm_kernels.hpp and garlic_amd/host/size_classes.hpp.  Every per-point
operation is one numpy operation in the reference's association; the N-term sums run in index order (np.cumsum adds
sequentially), once in float64 -- the reference's own arithmetic -- and once in np.longdouble.  The distance between the
two is the rounding noise of the reference itself: tests/test_gpu_gmm.py grants the device 8 times it.
tests/test_gmm_cpu.py checks this file against the reference binary's recorded output."""
import concurrent.futures
import functools
import gzip
import math
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
MAX_K = 8
MAX_ITER, PRECISION = 1000, 1e-5          # selectSizeClasses' maxIter and tolerance
FIELDS = ("a", "mean", "var", "loglik", "bic")


def block_points():
    """points per workgroup of the EM pass, from the constant the kernels are built with"""
    src = open(os.path.join(ROOT, "garlic_amd", "csrc", "gmm_kernels.hpp")).read()
    return int(re.search(r"^constexpr int GMM_BLOCK_POINTS = (\d+);", src, re.M).group(1))


def blocks(n):
    """workgroups of one pass: a function of n alone"""
    b = block_points()
    return (n + b - 1) // b


# ---- the data

CONTENTS = ["three", "two", "one", "overlap"]
BIG = 100003
KS = [1, 2, 3, 5, 8]
FIXED_ITERS = (1, 2, 25)


def sizes():
    b = block_points()
    return [1, 2, 63, 64, 65, b - 1, b, b + 1, 3 * b + 17, BIG]


@functools.lru_cache(maxsize=None)
def content(name, n):
    """n ROH-like lengths in bp, in no particular order: lognormal size classes"""
    rng = np.random.default_rng(7300 + CONTENTS.index(name) * 31 + n % 1000)
    u = rng.random(n)
    if name == "three":          # three well-separated classes, the shape of GARLIC's A / B / C
        mu = np.select([u < 0.55, u < 0.85], [math.log(3.0e4), math.log(2.0e5)], math.log(1.5e6))
        x = np.exp(rng.normal(mu, 0.25))
    elif name == "two":
        x = np.exp(rng.normal(np.where(u < 0.7, math.log(5.0e4), math.log(6.0e5)), 0.3))
    elif name == "one":
        x = np.exp(rng.normal(math.log(1.0e5), 0.2, n))
    else:
        assert name == "overlap"     # two classes whose densities overlap heavily
        x = np.exp(rng.normal(np.where(u < 0.5, math.log(8.0e4), math.log(1.2e5)), 0.35))
    x = np.ascontiguousarray(x, dtype=np.float64)
    x.setflags(write=False)
    return x


def golden_lengths(tag):
    """the size column of tests/golden/e2e/<tag>.roh.bed.gz: the lengths the reference binary fitted, in its order"""
    out = []
    with gzip.open(os.path.join(ROOT, "tests", "golden", "e2e", tag + ".roh.bed.gz"), "rt") as f:
        for line in f:
            if not line.startswith("track"):
                out.append(float(line.split("\t")[4]))
    return np.array(out, dtype=np.float64)


def golden_log(tag):
    """(list of (a, mean, var) strings per class in printed order, list of boundary strings)"""
    lines = open(os.path.join(ROOT, "tests", "golden", "e2e", tag + ".log.txt")).read().splitlines()
    gauss = [re.fullmatch(r"Gaussian class (\w) \( mixture, mean, std \) = \( (\S+), (\S+), (\S+) \)", l) for l in lines[:-1]]
    assert all(gauss) and [m.group(1) for m in gauss] == [chr(65 + i) for i in range(len(gauss))]
    bounds = re.fullmatch(r"Selected ROH size boundaries = \( (.*) \)", lines[-1]).group(1).split()
    return [m.groups()[1:] for m in gauss], bounds


def printed_alike(got, want):
    """two %g strings agree to the six printed digits, +-1 in the last"""
    g, w = float(got), float(want)
    unit = 10.0 ** (math.floor(math.log10(abs(w))) - 5)
    return abs(g - w) <= 1.0001 * unit


# ---- selectSizeClasses around the fit

def init(x, k, recurrence=False):
    """the initial guess: a_n = 1 / K, mean_n = mu (n + 1) / (K + 1), var_n = var (n + 1) / K from the mean and the (n - 1)
    variance of the lengths.  recurrence: the long-double running means of gsl_stats_mean / gsl_stats_variance literally
    (a Python loop: small n only); otherwise exactly rounded sums (math.fsum), which agree with them to a few ulp."""
    n = x.shape[0]
    if recurrence:
        mean = LD(0)
        for i in range(n):
            mean += (LD(x[i]) - mean) / LD(i + 1)
        mu = float(mean)
        v = LD(0)
        for i in range(n):
            d = LD(x[i]) - LD(mu)
            v += (d * d - v) / LD(i + 1)
        v = float(v)
    else:
        mu = math.fsum(x) / n
        v = math.fsum((t - mu) ** 2 for t in x.tolist()) / n
    with np.errstate(all="ignore"):
        var = np.float64(v) * (np.float64(n) / np.float64(n - 1))
    a0 = np.full(k, 1.0 / float(k))
    mean0 = np.array([mu * float(i + 1) / float(k + 1) for i in range(k)])
    with np.errstate(all="ignore"):
        var0 = np.array([np.float64(var) * np.float64(i + 1) / np.float64(k) for i in range(k)])
    return a0, mean0, var0


def pdf(x, sigma):
    """gsl_ran_gaussian_pdf"""
    u = x / abs(sigma)
    return (1.0 / (math.sqrt(2.0 * math.pi) * abs(sigma))) * math.exp(-u * u / 2.0)


def boundaries(a, mean, var):
    """the classes ordered by mean; between neighbours the root of a1 pdf(x - mu1, sqrt(var1)) - a2 pdf(x - mu2, sqrt(var2))
    inside [mu1, mu2], to 1e-12 relative (scipy's brentq where scipy is installed, else bisection)"""
    order = np.argsort(np.asarray(mean), kind="stable")
    out = []
    for p, q in zip(order[:-1], order[1:]):
        f = lambda t: a[p] * pdf(t - mean[p], math.sqrt(var[p])) - a[q] * pdf(t - mean[q], math.sqrt(var[q]))
        lo, hi = float(mean[p]), float(mean[q])
        assert f(lo) * f(hi) < 0, "no sign change between the means"
        try:
            from scipy.optimize import brentq
            out.append(float(brentq(f, lo, hi, xtol=1e-12 * lo, rtol=1e-12, maxiter=1000)))
        except ImportError:
            flo = f(lo)
            while hi - lo > 1e-12 * lo:
                mid = 0.5 * (lo + hi)
                if (f(mid) < 0) == (flo < 0):
                    lo = mid
                else:
                    hi = mid
            out.append(0.5 * (lo + hi))
    return [int(i) for i in order], out


def class_lines(a, mean, var):
    order = np.argsort(np.asarray(mean), kind="stable")
    return ["Gaussian class %s ( mixture, mean, std ) = ( %g, %g, %g )" % (chr(65 + i), a[k], mean[k], var[k]) for i, k in enumerate(order)]


# ---- the fit

def update(x, a, mean, var, dtype):
    """one GMM::update in `dtype`: (a, mean, var, loglik, bic) of the next iteration"""
    T = dtype
    n, k = x.shape[0], a.shape[0]
    xs = x.astype(T)
    C = T(-0.5) * np.log(T(2) * T(np.pi))          # the reference's 2 * M_PI is a double
    with np.errstate(all="ignore"):
        r = np.empty((k, n), dtype=T)
        for i in range(k):
            d = xs - mean[i]
            r[i] = np.log(a[i]) + ((C - T(0.5) * np.log(var[i])) - (d * d) / (T(2.0) * var[i]))
        l_max = np.full(n, -np.finfo(np.float64).max, dtype=T)
        for i in range(k):
            l_max = np.where(r[i] > l_max, r[i], l_max)
        s = np.zeros(n, dtype=T)
        for i in range(k):
            s = s + np.exp(r[i] - l_max)
        tmp = l_max + np.log(s)
        L = np.cumsum(tmp)[-1]
        den = np.zeros(n, dtype=T)
        for i in range(k):
            r[i] = np.exp(r[i] - tmp)
            den = den + r[i]
        na, nm, nv = np.empty(k, dtype=T), np.empty(k, dtype=T), np.empty(k, dtype=T)
        for i in range(k):
            s0 = np.cumsum(r[i] / den)[-1]
            s1 = np.cumsum(xs * r[i] / den)[-1]
            s2 = np.cumsum(xs * xs * r[i] / den)[-1]
            na[i] = s0 / T(n)
            nm[i] = s1 / s0
            nv[i] = s2 / s0 - nm[i] * nm[i]
        bic = T(-2.0) * L + T(3.0 * k - 1) * np.log(T(n))
    return na, nm, nv, L, bic


def fit(x, a0, mean0, var0, max_iter, precision, dtype, keep=()):
    """GMM::estimate in `dtype`: dict of a, mean, var, loglik, bic, iterations, converged; with keep = (i1, i2, ...) a dict
    {i: that dict after i updates} as well (the fit runs with precision < 0 then, or the stop may come first)"""
    T = dtype
    a, mean, var = (np.array(v, dtype=np.float64).astype(T) for v in (a0, mean0, var0))
    prev = T(-np.finfo(np.float64).max)
    state = lambda it, conv, L, bic: {"a": a.copy(), "mean": mean.copy(), "var": var.copy(), "loglik": L, "bic": bic,
                                      "iterations": it, "converged": conv}
    kept = {}
    L = bic = T(0)
    it, conv = 0, 0
    for it in range(1, max_iter + 1):
        a, mean, var, L, bic = update(x, a, mean, var, T)
        if abs(L - prev) <= T(precision):
            conv = 1
        if it in keep:
            kept[it] = state(it, conv, L, bic)
        if conv:
            break
        prev = L
    out = state(it, conv, L, bic)
    return (out, kept) if keep else out


def flat(s):
    """the fields of a fit as one vector"""
    return np.concatenate([np.asarray(s[f]).reshape(-1) for f in FIELDS])


def noise(f64, ld):
    """the largest relative deviation of the float64 reference from the long-double one over the fields; None when they do
    not have the same NaNs (the case then only pins the NaN pattern)"""
    p, q = flat(f64).astype(LD), flat(ld).astype(LD)
    if not (np.isnan(p) == np.isnan(q)).all():
        return None
    ok = ~np.isnan(q) & (q != 0)
    return float(np.max(np.abs(p[ok] - q[ok]) / np.abs(q[ok]))) if ok.any() else 0.0


def fixed_cases():
    """(content, n, k) of the fixed-iteration grid: every size with every K on the three-class data, the other contents at
    the multi-block size with the K they were made for"""
    b = block_points()
    out = [("three", n, k) for n in sizes() for k in KS]
    out += [("two", 3 * b + 17, 2), ("one", 3 * b + 17, 1), ("overlap", 3 * b + 17, 2), ("overlap", b + 1, 3)]
    return out


def stop_cases():
    """(content or golden tag, n, k) whose float64 and long-double references stop at the same iteration (test_gmm_cpu.py
    asserts that they do)"""
    b = block_points()
    return [("refs3", 113, 3), ("refs2", 113, 2), ("three", 3 * b + 17, 3), ("two", b + 1, 2), ("one", 65, 1), ("three", b - 1, 2)]


def data_of(name, n):
    if name.startswith("refs"):
        x = golden_lengths(name)
        assert x.shape[0] == n
        return x
    return content(name, n)


@functools.lru_cache(maxsize=None)
def fixed_reference(name, n, k):
    """{iterations: (float64 state, long-double state)} at FIXED_ITERS, never stopping early"""
    x = data_of(name, n)
    a0, m0, v0 = init(x, k)
    _, k64 = fit(x, a0, m0, v0, max(FIXED_ITERS), -1.0, np.float64, keep=FIXED_ITERS)
    _, kld = fit(x, a0, m0, v0, max(FIXED_ITERS), -1.0, LD, keep=FIXED_ITERS)
    return {i: (k64[i], kld[i]) for i in FIXED_ITERS}


@functools.lru_cache(maxsize=None)
def stop_reference(name, n, k):
    """(float64 state, long-double state) of the fit with the reference's stop rule"""
    x = data_of(name, n)
    a0, m0, v0 = init(x, k, recurrence=name.startswith("refs"))
    return fit(x, a0, m0, v0, MAX_ITER, PRECISION, np.float64), fit(x, a0, m0, v0, MAX_ITER, PRECISION, LD)


def warm(cases, fn):
    """fill fn's cache for all cases on a few threads (numpy's loops release the lock; each case's sums keep their order)"""
    with concurrent.futures.ThreadPoolExecutor(16) as pool:
        list(pool.map(lambda c: fn(*c), cases))
