"""The cases of the multi-size TGLS feed (garlic_lod_feed_multi_tgls): tests/test_gpu_tgls_feed_multi.py runs them on
the GPU, tests/test_tgls_feed_multi_cpu.py builds every one and checks with the oracle alone that each size's feed has
something to compare.  Also the grouping rule of include/garlic_hip.h, stated in Python."""
import functools
import os
import re

import numpy as np

import oracle_lib as ol
import tgls_feed_cases as cases
import tgls_slab_cases as scases

MG, ERROR = cases.MG, cases.ERROR
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUBSETS = cases.SUBSETS


def max_sizes():
    """TGM_MAX_SIZES, from the kernel's header"""
    src = open(os.path.join(cases.CSRC, "tgls_feed_multi_kernel.hpp")).read()
    return int(re.search(r"^constexpr int TGM_MAX_SIZES = (\d+);", src, re.M).group(1))


def groups_of(winsizes, ring_ok=None, solo=False, limit=None, max_w=None):
    """The grouping rule: the sizes that take the ring and are <= max_w, ascending (ties: call order), cut into groups of at
    most `limit` (of one under the switch), numbered from 0; then every other size a group of its own, ascending again."""
    limit = (limit or max_sizes()) if not solo else 1
    max_w = max_w or cases.single_max_w()
    ring_ok = [True] * len(winsizes) if ring_ok is None else ring_ok
    order = sorted(range(len(winsizes)), key=lambda i: (winsizes[i], i))
    group, n, held = [-1] * len(winsizes), 0, 0
    for i in order:
        if ring_ok[i] and winsizes[i] <= max_w:
            if held == 0 or held == limit:
                n, held = n + 1, 0
            group[i] = n - 1
            held += 1
    for i in order:
        if group[i] < 0:
            group[i] = n
            n += 1
    return group


def shared_of(group):
    return [group.count(g) >= 2 for g in group]


def take_ring(W, step, exact=False):
    return step >= cases.MIN_STEP and not exact


# ---- 1. shapes

def size_lists():
    m = max_sizes()
    many = [8, 20, 47, 64, 100, 144, 30, 77, 120, 12][: m + 2]
    return {"narrow": [5, 10, 33], "wide": [10, 100, 144], "tile": [31, 32, 33, 64], "twice": [60, 60], "many": many}


def step_kinds(name):
    return ["own"] if name == "twice" else ["4", "W", "W+7", "beyond"]


def steps_of(name, kind, ws, sizes):
    if name == "twice":
        return [60, 7]
    return {"4": [4] * len(ws), "W": list(ws), "W+7": [w + 7 for w in ws], "beyond": [max(sizes) + 5] * len(ws)}[kind]


def chrom_sizes(ws):
    """1, Wmin-1, Wmin, one strictly between Wmin and Wmax (only some sizes hold a window), Wmax, Wmax+1, Wmax+33 SNPs,
    a few thousand with gaps and a centromere, and one that is no multiple of 32"""
    lo, hi = min(ws), max(ws)
    mid = [(lo + hi) // 2] if hi - lo >= 2 else []
    return [1, lo - 1, lo] + mid + [hi, hi + 1, hi + 33, 3000, 2477]


def make_panel(ws, nind, seed, kind, sizes=None):
    rng = np.random.default_rng(seed)
    sizes = sizes or chrom_sizes(ws)
    chroms = [ol.random_panel(rng, n, nind, max_gap=MG, gaps=3 if n >= 2000 else 0, centro=n >= 2000) for n in sizes]
    return chroms, cases.bounded_likelihoods(np.random.default_rng(seed + 1), chroms, kind)


@functools.lru_cache(maxsize=None)
def shape_case(name):
    """(window sizes, nind, chroms, likelihoods, {W: oracle scores})"""
    names = sorted(size_lists())
    ws = size_lists()[name]
    nind = cases.NINDS[names.index(name)]
    chroms, gl = make_panel(ws, nind, 9300 + 10 * names.index(name), "codes" if names.index(name) % 2 else "continuous")
    return ws, nind, chroms, gl, scores_of(chroms, gl, ws)


def scores_of(chroms, gl, ws):
    return {W: cases.tgls_scores(chroms, gl, W) for W in sorted(set(ws))}


def expected(scores, ws, steps, idx=None):
    """per size the per-chromosome feeds of the oracle"""
    return [cases.flat(scores[W], step, idx) for W, step in zip(ws, steps)]


# ---- 2. ring boundary

def boundary_lists():
    s = cases.single_max_w()
    return [[s, s + 1], [50, 100, 200, 300]]


@functools.lru_cache(maxsize=None)
def boundary_case(k):
    ws = boundary_lists()[k]
    chroms, gl = make_panel(ws, 65, 9400 + k, "codes")
    return ws, 65, chroms, gl, scores_of(chroms, gl, ws)


# ---- 3. likelihoods

GL_SIZES = [10, 60, 100]


@functools.lru_cache(maxsize=None)
def likelihood_case(kind):
    """dictionary codes or continuous values with the clamp values 1e-16 and 1.0 among them (100 x -16 stays above -9990)"""
    from wlod_feed_cases import likelihoods
    nind = 70
    chroms, _ = make_panel(GL_SIZES, nind, 9500, "codes")
    gl = likelihoods(np.random.default_rng(9501 + (kind == "codes")), chroms, kind)
    for e in gl:
        e[::7, ::3] = 1e-16
        e[3::11, 1::5] = 1.0
    return GL_SIZES, nind, chroms, gl, scores_of(chroms, gl, GL_SIZES)


@functools.lru_cache(maxsize=None)
def codes_case():
    nind = 70
    chroms, _ = make_panel(GL_SIZES, nind, 9600, "codes")
    values = np.array([1e-16, 1e-3, 0.01, 0.2, 1.0])
    rng = np.random.default_rng(9601)
    codes = [rng.integers(0, len(values), size=c[0].shape).astype(np.uint8) for c in chroms]
    gl = [values[k] for k in codes]
    return GL_SIZES, nind, chroms, codes, values, gl, scores_of(chroms, gl, GL_SIZES)


# ---- 4. subsets, 8. switch and repeats

SUBSET_SIZES = [10, 50, 100]


@functools.lru_cache(maxsize=None)
def subset_case():
    chroms, gl = make_panel(SUBSET_SIZES, cases.SUBSET_NIND, 9700, "continuous")
    return SUBSET_SIZES, cases.SUBSET_NIND, chroms, gl, scores_of(chroms, gl, SUBSET_SIZES)


# ---- 5. slabs

SLAB_SIZES = [10, 50, 100, 200]


@functools.lru_cache(maxsize=None)
def slab_case(nind):
    """dictionary codes (only they take slabs); (sizes, chroms, codes, {W: scores})"""
    rng = np.random.default_rng(9800 + nind)
    chroms, _ = make_panel(SLAB_SIZES, nind, 9801 + nind, "codes")
    codes = [rng.integers(0, len(scases.VALUES), size=c[0].shape).astype(np.uint8) for c in chroms]
    gl = [scases.VALUES[k] for k in codes]
    return SLAB_SIZES, chroms, codes, scores_of(chroms, gl, SLAB_SIZES)


def slab_budgets():
    """(nind, slab blocks asked for, slab blocks the library's rule gives): the 200-individual panel has 4 blocks, where
    the smallest budget that holds two-block slabs (2 + 2 blocks) holds one slab of all 4 as well and the library takes
    the larger (tests/test_gpu_tgls_slabs.py); two-block slabs proper run on the 456-individual panel (8 blocks)"""
    return [(scases.NIND, 1, 1), (scases.NIND, 2, 4), (scases.NIND_WIDE, 2, 2)]


# ---- 6. fallbacks per size

@functools.lru_cache(maxsize=None)
def fallback_case():
    """on cases.exact_case's panel (likelihoods of 1e-16, W = 1000: a sum of exactly -9999.0 is possible): a step-3 size,
    the exact size, two ordinary ones.  (sizes, steps, takes the ring, nind, chroms, likelihoods, scores)"""
    W, narrow, nind, chroms, gl = cases.exact_case()
    ws, steps = [10, W, 50, narrow], [3, W, 50, narrow]
    ring = [False, False, True, True]
    return ws, steps, ring, nind, chroms, gl, scores_of(chroms, gl, ws)


# ---- 7. non-finite terms

NONFINITE_SIZES = [5, 60, 100]


@functools.lru_cache(maxsize=None)
def nonfinite_case():
    """as cases.nonfinite_case: a NaN frequency, likelihoods of 0 and infinity, in chromosomes every size has runs in"""
    nind, W = 70, 60
    sizes = chrom_sizes(NONFINITE_SIZES) + [2 * W + 100, 2 * W + 140]
    chroms, gl = make_panel(NONFINITE_SIZES, nind, 9900, "continuous", sizes=sizes)
    chroms[-1][1][W + 7] = np.nan
    gl[-2][W // 2, ::2] = 0.0
    gl[-2][W + 20, 1::4] = np.inf
    return NONFINITE_SIZES, nind, chroms, gl, scores_of(chroms, gl, NONFINITE_SIZES)


# ---- 9. neighbours

NEIGHBOUR_SIZES = [20, 40, 100]


@functools.lru_cache(maxsize=None)
def neighbour_case():
    nind, chroms, gpos, lds, gl, _ = cases.neighbour_case(20)
    return NEIGHBOUR_SIZES, nind, chroms, gpos, lds, gl, scores_of(chroms, gl, NEIGHBOUR_SIZES)


# ---- every call of the GPU file: (name, per-size per-chromosome expected feeds, sizes that may be empty on some chromosome)

def all_calls():
    for name in sorted(size_lists()):
        ws, nind, chroms, gl, scores = shape_case(name)
        sizes = [c[0].shape[0] for c in chroms]
        for kind in step_kinds(name):
            yield ("shape", name, kind), expected(scores, ws, steps_of(name, kind, ws, sizes))
    for k in range(len(boundary_lists())):
        ws, nind, chroms, gl, scores = boundary_case(k)
        yield ("boundary", k), expected(scores, ws, ws)
    for kind in ("codes", "continuous"):
        ws, nind, chroms, gl, scores = likelihood_case(kind)
        yield ("gl", kind), expected(scores, ws, ws)
    ws, nind, chroms, codes, values, gl, scores = codes_case()
    yield ("set_gl_codes",), expected(scores, ws, ws)
    ws, nind, chroms, gl, scores = subset_case()
    for idx in SUBSETS:
        yield ("subset", tuple(idx)), expected(scores, ws, ws, np.array(idx))
    yield ("everyone",), expected(scores, ws, ws)
    for nind in sorted({b[0] for b in slab_budgets()}):
        ws, chroms, codes, scores = slab_case(nind)
        yield ("slabs", nind), expected(scores, ws, ws)
    ws, steps, ring, nind, chroms, gl, scores = fallback_case()
    yield ("fallbacks",), expected(scores, ws, steps)
    ws, nind, chroms, gl, scores = nonfinite_case()
    yield ("non-finite",), expected(scores, ws, ws)
    ws, nind, chroms, gpos, lds, gl, scores = neighbour_case()
    yield ("neighbours",), expected(scores, ws, ws)
