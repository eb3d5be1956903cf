"""The key sets and panel cases of the sorted KDE feed (tests/test_gpu_feed_sort.py runs them on the GPU,
tests/test_feed_sort_cpu.py checks with numpy and the oracle alone that "ascending" is unique for every one of them)."""
import functools
import os
import re

import numpy as np

import oracle_lib as ol
import tgls_feed_cases as tcases
import tgls_slab_cases as scases
import wlod_feed_cases as wcases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MG, ERROR, M, MU = wcases.MG, wcases.ERROR, wcases.M, wcases.MU


def fs_tile():
    """keys per tile of the sorter, from the constant the kernels are built with"""
    src = open(os.path.join(ROOT, "garlic_amd", "csrc", "feed_sort_kernel.hpp")).read()
    return int(re.search(r"^constexpr int FS_TILE = (\d+);", src, re.M).group(1))


# ---- the key order of include/garlic_hip.h restated

def key(x):
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return b ^ np.where(b >> np.uint64(63) != 0, np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64(0x8000000000000000))


def unkey(k):
    k = np.ascontiguousarray(k, dtype=np.uint64)
    return (k ^ np.where(k >> np.uint64(63) != 0, np.uint64(0x8000000000000000), np.uint64(0xFFFFFFFFFFFFFFFF))).view(np.float64)


def sorted_by_key(x):
    """the values in ascending key order (keys that are equal are equal bit patterns: the result is unique)"""
    return unkey(np.sort(key(x)))


# ---- sorter alone

def sizes():
    t = fs_tile()
    return [0, 1, 2, 63, 64, 65, t - 1, t, t + 1, 3 * t + 17, 200003]


CONTENTS = ["normal", "equal", "two", "ascending", "descending", "mixed"]


def content(name, n, seed=0):
    rng = np.random.default_rng(9500 + seed + n % 1000)
    if name == "normal":
        return rng.standard_normal(n)
    if name == "equal":
        return np.full(n, -3.25)
    if name == "two":
        return rng.choice([1.5, -2.0], size=n)
    if name == "ascending":
        return np.arange(n, dtype=np.float64) - n / 3.0
    if name == "descending":
        return n / 3.0 - np.arange(n, dtype=np.float64)
    assert name == "mixed"       # +-inf, +-0.0, denormals, both signs
    special = np.array([np.inf, -np.inf, 0.0, -0.0, 5e-324, -5e-324, 2.2e-308, -2.2e-308, 1e-310, -1e-310, 1.0, -1.0, 1e300, -1e300])
    x = rng.standard_normal(n) * 10.0 ** rng.integers(-300, 300, size=n)
    where = rng.random(n) < 0.5
    x[where] = rng.choice(special, size=int(where.sum()))
    return x


def one_byte_keys(byte, n, seed=0):
    """n doubles whose keys differ in byte `byte` (0 = least significant) and nowhere else, at least two values of it"""
    rng = np.random.default_rng(9600 + byte + seed)
    base = np.uint64(0x3C4D5E6F708192A3) & ~(np.uint64(0xFF) << np.uint64(8 * byte))
    digits = rng.integers(0, 256, size=n).astype(np.uint64)
    digits[0], digits[-1] = 7, 200
    return unkey(base | (digits << np.uint64(8 * byte)))


# ---- through the feed calls: one small panel per individual count serves every call

W = 20
MULTI_SIZES = [12, 20, 33]
TGLS_MULTI_SIZES = [8, 12, 20, 24, 33]          # two groups: the four smallest share a ring, 33 has its own
NINDS = [1, 65, 200]
SUBSET = [130, 3, 190, 129, 0]                  # of 200: unordered, block 1 left out
CALLS = ["chain", "scores", "wlod", "wlod_gl", "tgls", "tgls_slabs", "multi", "multi_tgls"]


def chrom_sizes():
    """1, W-1, W, W+1, W+33 SNPs and one with gaps and a centromere"""
    return [1, W - 1, W, W + 1, W + 33, 700]


@functools.lru_cache(maxsize=None)
def panel(nind):
    """(chroms, gpos, lds, codes, values, likelihoods) of the panel with nind individuals"""
    rng = np.random.default_rng(9700 + nind)
    szs = chrom_sizes()
    chroms = [ol.random_panel(rng, n, nind, max_gap=MG, gaps=3 if k == 5 else 0, centro=k >= 5) for k, n in enumerate(szs)]
    gpos = [np.cumsum(np.diff(c[2], prepend=0) * 1e-6 * rng.uniform(0.8, 1.2, size=c[2].shape[0])) for c in chroms]
    lds = [rng.uniform(1.0, 5.0, size=(n, W)) for n in szs]
    values = np.array([1e-6, 1e-3, 0.01, 0.2])      # bounded: the ring form is due (tgls_feed_cases.bounded_likelihoods)
    codes = [rng.integers(0, len(values), size=c[0].shape).astype(np.uint8) for c in chroms]
    return chroms, gpos, lds, codes, values, [values[k] for k in codes]


def call_sizes(call):
    """[(winsize, step)] of a call"""
    if call == "multi":
        return [(w, w) for w in MULTI_SIZES]
    if call == "multi_tgls":
        return [(w, w) for w in TGLS_MULTI_SIZES]
    return [(W, 1 if call == "scores" else W)]


@functools.lru_cache(maxsize=None)
def oracle_scores(nind, kind, winsize):
    """kind: 'lod' (--error), 'tgls', 'wlod', 'wlod_gl'"""
    chroms, gpos, lds, _, _, gl = panel(nind)
    if kind == "lod":
        return [ol.oracle_calc_lod(g, f, p, cs, ce, winsize, ERROR, MG, threads=8) for g, f, p, cs, ce in chroms]
    if kind == "tgls":
        return tcases.tgls_scores(chroms, gl, winsize)
    return wcases.wlod_scores(chroms, gpos, lds, winsize, gl=gl if kind == "wlod_gl" else None)


KIND = {"chain": "lod", "scores": "lod", "multi": "lod", "wlod": "wlod", "wlod_gl": "wlod_gl", "tgls": "tgls", "tgls_slabs": "tgls",
        "multi_tgls": "tgls"}


@functools.lru_cache(maxsize=None)
def oracle_feeds(call, nind, subset=False):
    """per size of the call: the oracle's feed per chromosome, in the reference's order"""
    idx = SUBSET if subset else None
    return [wcases.flat(oracle_scores(nind, KIND[call], w), step, idx) for w, step in call_sizes(call)]


def panel_cases():
    """(call, nind, subset)"""
    return [(c, n, False) for c in CALLS for n in NINDS] + [(c, 200, True) for c in CALLS]


def slab_budget(nind):
    """one-block slabs (tgls_slab_cases)"""
    return scases.budget_for(sum(chrom_sizes()), 1, nind)


def shard_merge_cases():
    """lists of ascending shard feeds: equal values across shards, empty shards, one shard, none"""
    rng = np.random.default_rng(9800)
    a = np.sort(rng.standard_normal(1000))
    b = np.sort(np.concatenate([a[::7], rng.standard_normal(333)]))          # values shared with a
    c = np.sort(rng.choice([-1.0, 0.5, 2.0], size=257))
    e = np.empty(0)
    return [[a, b, c], [e, a, e, b], [a], [e, e], [], [c, c.copy(), c.copy()], [np.full(5, 1.0), np.full(3, 1.0), np.array([0.5, 1.0, 7.0])]]
