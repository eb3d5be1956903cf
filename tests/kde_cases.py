"""The feeds of the device KDE (garlic_feed_kde) and a numpy reference of computeKDE's numbers, src/garlic-kde.cpp:14-140:
sd and the Gaussian sums in np.longdouble, the quantile, targets and normalisation in float64 in the reference's
association; get_min_btw_modes and calculateWiggle written here independently of garlic_amd/host/kde_select.hpp.
tests/test_kde_cpu.py checks this reference, tests/test_gpu_kde.py the device against it."""
import concurrent.futures
import functools
import math
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POINTS, CUT, MODE_WINDOW = 512, 3.0, 20
LD = np.longdouble


def kde_chunk():
    """sources per chunk of the sums kernel, from the constant the kernels are built with"""
    src = open(os.path.join(ROOT, "garlic_amd", "csrc", "kde_kernels.hpp")).read()
    return int(re.search(r"^constexpr int KDE_CHUNK = (\d+);", src, re.M).group(1))


# ---- the feeds

CONTENTS = ["bimodal", "uniform", "wide", "narrow", "shifted", "two_values"]
BIG = 100003          # several slices


def sizes():
    c = kde_chunk()
    return [2, 3, 63, 64, 65, c - 1, c, c + 1, 3 * c + 17, BIG]


@functools.lru_cache(maxsize=None)
def content(name, n):
    """n ascending finite doubles with a spread between the quartiles (|mean| <= 1e3 sd throughout)"""
    rng = np.random.default_rng(9900 + CONTENTS.index(name) * 17 + n % 1000)
    if name == "bimodal":        # the shape of a real feed: non-autozygous windows below zero, autozygous ones above
        x = np.where(rng.random(n) < 0.8, rng.normal(-12.0, 6.0, n), rng.normal(9.0, 2.5, n))
    elif name == "uniform":
        x = rng.uniform(-3.0, 5.0, n)
    elif name == "wide":         # range >= 1e4 h from n = 63 on: a unit cluster sets the quartiles (and with them h), a few
        x = rng.normal(0.0, 1.0, n)   # values far out set the range; most (chunk, target) pairs contribute exactly 0
        far = rng.random(n) < 0.1
        x[far] = rng.uniform(-2.0e4, 2.0e4, int(far.sum()))
        if n >= 63:
            x[:2] = -2.0e4, 2.0e4
    elif name == "narrow":       # the narrowest a feed gets: two tight clusters that hold the quartiles.  lo <= sd <= range / 2
        x = (np.arange(n) % 2) + rng.uniform(0.0, 1e-3, n)   # bounds range / h from below by 2.2 n^0.2 (about 2 h at n = 2 only,
        #                          22 h at 1e5): still no argument reaches -746, so no pair is skipped at any size here
    elif name == "shifted":      # mean = 1e3 sd (990, so that rounding leaves it inside the bound the h tolerance assumes)
        z = rng.normal(0.0, 1.0, n)
        x = (z - z.mean()) + 990.0 * z.std(ddof=1)
    else:
        assert name == "two_values"
        x = np.where(np.arange(n) % 2 == 0, -1.5, 2.25)
    x = np.sort(np.ascontiguousarray(x, dtype=np.float64))
    if n == 2 and x[0] == x[1]:
        x[1] = x[0] + 1.0
    x.setflags(write=False)
    return x


# ---- the reference

def quantile(x, f):
    """gsl_stats_quantile_from_sorted_data"""
    n = x.shape[0]
    idx = f * float(n - 1)
    k = int(idx)
    d = idx - float(k)
    if k >= n - 1:
        return float(x[n - 1])
    return float((1 - d) * float(x[k]) + d * float(x[k + 1]))


def sd_longdouble(x):
    xl = x.astype(LD)
    mean = xl.sum() / LD(x.shape[0])
    return np.sqrt(((xl - mean) ** 2).sum() / LD(x.shape[0] - 1))


def bandwidth(sd, q25, q75, n):
    lo = min(float(sd), (q75 - q25) / 1.34)
    return 0.9 * lo * math.pow(float(n), -0.2)


def targets(lo, hi, h):
    mx = hi + CUT * h
    mn = lo - CUT * h
    return np.array([(float(i + 1) / float(POINTS)) * (mx - mn) + mn for i in range(POINTS)], dtype=np.float64)


def raw_longdouble(x, t, h, block=4096):
    """(1/n) sum_i exp(-(x_i - t_j)^2 / h^2) in long double, the sources in blocks so that memory stays small"""
    tl, hl = t.astype(LD), LD(h)

    def part(i):
        d = x[i:i + block].astype(LD)[:, None] - tl[None, :]
        return np.exp(-(d * d) / (hl * hl)).sum(axis=0)

    acc = np.zeros(t.shape[0], dtype=LD)
    with concurrent.futures.ThreadPoolExecutor(8) as pool:      # (numpy's loops release the lock; the order of the adds is fixed)
        for p in pool.map(part, range(0, x.shape[0], block)):
            acc += p
    return acc / LD(x.shape[0])


def normalise(raw, t):
    spacing = float(t[1]) - float(t[0])
    s = 0.0
    for v in raw:
        s += float(v)
    return np.array([float(v) / (s * spacing) for v in raw], dtype=np.float64)


HUGE = 2100 * 2048 + 1029          # more chunks than slices: two chunks per slice, and a last slice of one


def raw_targets(n):
    """the targets at which the long-double sums are evaluated: all 512; at HUGE (the case is there for the loop over a
    slice's chunks, which every target runs alike, and the reference costs 0.1 us per pair) one per thread quarter and end"""
    return np.arange(POINTS) if n < HUGE else np.array([0, 1, 130, 257, 383, 510, 511])


@functools.lru_cache(maxsize=None)
def reference_of(name, n, with_raw=True):
    return reference(content(name, n), with_raw)


def reference(x, with_raw=True):
    """every field of garlic_kde for the ascending feed x (raw at raw_targets(n), y only when those are all)"""
    n = x.shape[0]
    sd = sd_longdouble(x)
    q25, q75 = quantile(x, 0.25), quantile(x, 0.75)
    h = bandwidth(float(sd), q25, q75, n)
    t = targets(float(x[0]), float(x[-1]), h)
    r = {"n": n, "sd": sd, "q25": q25, "q75": q75, "h": h, "lo": float(x[0]), "hi": float(x[-1]), "x": t}
    if with_raw:
        at = raw_targets(n)
        r["raw_at"] = at
        r["raw"] = raw_longdouble(x, t[at], h)
        if at.shape[0] == POINTS:
            r["y"] = normalise(r["raw"].astype(np.float64), t)
    return r


# ---- behind the density: get_min_btw_modes (:142-234) and calculateWiggle (:3-12), independently of kde_select.hpp

def arg_max_window(v):
    best, at = np.finfo(np.float64).tiny, -1          # numeric_limits<double>::min()
    for i, e in enumerate(v):
        if best < e:
            best, at = e, i
    return at


def min_between_modes(x, y, wsize):
    """-> (cutoff, index of the minimum, (left mode index, right mode index), (largest count, second count))"""
    size, win = len(y), MODE_WINDOW
    n = size - win
    maxes, counts = [0.0] * n, [0] * n
    slot = 0
    for i in range(n):
        at = arg_max_window(y[i:i + win]) + i
        assert at >= 0, "the reference reads y[-1] here"
        m = y[at]
        if i == 1:
            maxes[1] = m
            counts[1] += 1
        elif maxes[slot] == m:
            counts[slot] += 1
        else:
            slot += 1
            maxes[slot] = m
            counts[slot] += 1
    most, second = counts[0], 0
    for c in counts[1:]:
        if most <= c:
            most, second = c, most
        elif second <= c:
            second = c
    first_max = second_max = -1.0
    for m, c in zip(maxes, counts):
        if c == most or c == second:
            if first_max <= m:
                first_max, second_max = m, first_max
            elif second_max <= m:
                second_max = m
    left = right = -1
    for i in range(size):
        if y[i] == first_max:
            left = i
        if y[i] == second_max:
            right = i
    assert left >= 0 and right >= 0
    if right < left:
        left, right = right, left
    at = left + min(range(right - left + 1), key=lambda k: (y[left + k], k))
    cutoff = float(x[at]) if abs(float(x[at]) / wsize) < 1 else 0.0
    return cutoff, at, (left, right), (most, second)


def wiggle(x, y):
    """sum over the windows of 20 points of (residual sum of squares of the least-squares line through (x, 100 y)) / 20"""
    x, y = np.asarray(x, dtype=np.float64), 100.0 * np.asarray(y, dtype=np.float64)
    tot = 0.0
    for i in range(len(y) - MODE_WINDOW):
        xs, ys = x[i:i + MODE_WINDOW], y[i:i + MODE_WINDOW]
        _, res, _, _, _ = np.polyfit(xs - xs.mean(), ys, 1, full=True)
        tot += (float(res[0]) if len(res) else 0.0) / float(MODE_WINDOW)
    return tot


def kde_lines(x, y, scale=1.0):
    """writeKDEResult: "x y" per line under default ostream formatting (%g)"""
    return "".join("%g %g\n" % (a, b * scale if scale != 1.0 else b) for a, b in zip(x, y))


def read_kde(path):
    a = np.loadtxt(path)
    return np.ascontiguousarray(a[:, 0]), np.ascontiguousarray(a[:, 1])
