"""Splits of the feeds of tests/kde_cases.py into sorted parts (garlic_kde_parts): every part is ascending, the union is
kde_cases.content(name, n).  tests/test_kde_parts_cpu.py runs the host descent over them, tests/test_gpu_kde_parts.py the
device."""
import functools

import numpy as np

import kde_cases as cases

PARTS = [1, 2, 3, 8, 64]


def totals():
    """n = 2 and n = 3 are the smallest shapes ((1, 1) and (1, 2)); 3c + 17 is several chunks; BIG several slices"""
    return [2, 3, 65, 3 * cases.kde_chunk() + 17, cases.BIG]


def key(x):
    """garlic_feed_sort's 64-bit key (include/garlic_hip.h): unsigned order of the keys is ascending order of the doubles"""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return b ^ np.where(b >> np.uint64(63) != 0, np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64(0x8000000000000000))


def key_value(k):
    k = np.ascontiguousarray(k, dtype=np.uint64)
    b = np.where(k >> np.uint64(63) != 0, k ^ np.uint64(0x8000000000000000), ~k)
    return b.view(np.float64)


def interleaved(x, P):
    """value i goes to part i mod P: the parts' ranges overlap fully"""
    return [np.ascontiguousarray(x[p::P]) for p in range(P)]


def ranges(x, P):
    """contiguous and disjoint"""
    n = x.shape[0]
    return [np.ascontiguousarray(x[n * p // P: n * (p + 1) // P]) for p in range(P)]


def by_sizes(x, sizes):
    assert sum(sizes) == x.shape[0]
    at = np.concatenate([[0], np.cumsum(sizes)])
    return [np.ascontiguousarray(x[at[i]:at[i + 1]]) for i in range(len(sizes))]


def lopsided(x):
    n = x.shape[0]
    return [("1+rest", by_sizes(x, (1, n - 1))), ("0+all", by_sizes(x, (0, n))), ("rest+0+2", by_sizes(x, (n - 2, 0, 2)))]


def chunks(x):
    """parts of c - 1, c and c + 1 values (n = 3c + 17 gives a fourth of 17)"""
    c, n = cases.kde_chunk(), x.shape[0]
    sizes = [s for s in (c - 1, c, c + 1)]
    if n < sum(sizes):
        return None
    if n > sum(sizes):
        sizes.append(n - sum(sizes))
    return by_sizes(x, sizes)


@functools.lru_cache(maxsize=None)
def splits(name, n):
    """[(label, [part, ...])] for the feed content(name, n): every split kind at every part count that fits"""
    x = cases.content(name, n)
    out = []
    for P in PARTS:
        if P == 1:
            out.append(("one", [np.ascontiguousarray(x)]))
            continue
        out.append(("interleaved%d" % P, interleaved(x, P)))      # (P > n: the parts past n are empty)
        out.append(("ranges%d" % P, ranges(x, P)))
    out += [("lopsided " + what, parts) for what, parts in lopsided(x)]
    if chunks(x) is not None and n <= 3 * cases.kde_chunk() + 17:
        out.append(("chunks", chunks(x)))
    for _, parts in out:
        assert sum(p.shape[0] for p in parts) == n and len(parts) <= 64
        assert all((np.diff(p) >= 0).all() for p in parts)
        assert np.array_equal(np.sort(np.concatenate(parts)), x)
    if name == "two_values" and n >= 4:       # both values in both parts: ties cross parts, a quartile falls inside a tie
        for what, parts in out:
            if what.startswith("interleaved2"):
                assert all(len(np.unique(p)) == 2 for p in parts)
    return out


def zero_feed():
    """-0.0 and +0.0 in key order with ties, split so that both signs sit in both parts"""
    x = np.array([-2.0, -1.0, -0.0, -0.0, 0.0, 0.0, 3.0, 3.0, 4.0])      # x[k25] = x[k25 + 1] = -0.0: the sign is checked
    assert np.array_equal(np.argsort(key(x), kind="stable"), np.arange(x.shape[0]))
    return x, [np.ascontiguousarray(x[0::2]), np.ascontiguousarray(x[1::2])]


def descent(rank_sum, ranks):
    """the radix descent restated in numpy, independently of host/kde_parts.hpp: rank_sum(keys uint64 [1024]) -> the
    union's counts below each key.  Returns (the values at the ranks, rounds)."""
    prefix = np.zeros(4, dtype=np.uint64)
    digits = np.arange(256, dtype=np.uint64)
    rounds = 0
    for byte in range(7, -1, -1):
        shift = np.uint64(8 * byte)
        probes = (prefix[:, None] | (digits[None, :] << shift)).reshape(-1)
        below = np.asarray(rank_sum(probes), dtype=np.int64).reshape(4, 256)
        rounds += 1
        for q in range(4):
            d = int(np.nonzero(below[q] <= ranks[q])[0].max())
            prefix[q] |= np.uint64(d) << shift
    return key_value(prefix), rounds


def order_ranks(n):
    """the four 0-based ranks garlic_kde_parts selects, clamped to the last value as the single-feed kernels clamp"""
    k25, k75 = int(0.25 * float(n - 1)), int(0.75 * float(n - 1))
    return [min(k, n - 1) for k in (k25, k25 + 1, k75, k75 + 1)]
