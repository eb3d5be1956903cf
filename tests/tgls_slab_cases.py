"""The panels, budgets and calls of the TGLS term slabs (tests/test_gpu_tgls_slabs.py runs them on the GPU,
tests/test_tgls_slabs_cpu.py checks with the oracle alone that every one of them has something to compare)."""
import functools

import numpy as np

import oracle_lib as ol
import tgls_feed_cases as fcases

MG, ERROR = fcases.MG, fcases.ERROR
WIDTHS = [10, 100, 200]              # both sides of TG_SINGLE_MAX_W = 144 (the one-stream / two-stream ring)
NIND = 200                           # 3 full 64-individual blocks + 8
NIND_WIDE = 456                      # 7 full blocks + 8: slabs of 2 blocks (four of them) and of 3 (3 + 3 + 2)
VALUES = np.array([1e-16, 1e-3, 0.01, 0.2, 1.0])      # dictionary likelihoods, the clamp values among them
FEEDINGS = ["set_gl", "set_gl_codes"]
FRAC = 0.25
ROWS_PAD = 32 + 4160                 # the rows of a block of the term matrix beside its SNPs (include/garlic_hip.h)
SUB_RANGE = (64, 100)                # ind_begin, ind_count: blocks 1 and 2, across the boundary of one- and two-block slabs
# individual lists: blocks {0, 2, 3} (one of four left out), {0, 2} and {1, 3} (two left out, the rest not neighbours),
# {2, 3} (two left out, the rest neighbours)
SUBSETS = [[130, 3, 199, 0], [130, 3, 190, 129, 0], [199, 64], [140, 199, 130]]


def sizes_of(W):
    """1, W-1, W, W+1, W+33 SNPs and two chromosomes of a few thousand with gaps and a centromere (one no multiple of 32)"""
    return [1, W - 1, W, W + 1, W + 33, 3000, 2477]


@functools.lru_cache(maxsize=None)
def case(W, nind=NIND, seed=0):
    """(chroms, codes, likelihoods, oracle scores) of one panel; seed != 0: the changed panel of the sequence test"""
    rng = np.random.default_rng(9100 + 10 * W + nind + seed)
    sizes = sizes_of(W)
    chroms = [ol.random_panel(rng, n, nind, max_gap=MG, gaps=3 if k >= 5 else 0, centro=k >= 5) for k, n in enumerate(sizes)]
    codes = [rng.integers(0, len(VALUES), size=c[0].shape).astype(np.uint8) for c in chroms]
    gl = [VALUES[k] for k in codes]
    return chroms, codes, gl, fcases.tgls_scores(chroms, gl, W)


def cutoff_of(scores):
    """a cutoff that leaves windows, covered SNPs and segments to compare"""
    scored = np.concatenate([x[np.isfinite(x) & (x != ol.MISSING)] for x in scores])
    return float(np.quantile(scored, 0.7))


def blocks_of(nind, idx=None, sub=None):
    """the 64-individual blocks a call scores"""
    if idx is not None:
        return sorted({int(i) >> 6 for i in idx})
    b, n = sub or (0, nind)
    return list(range(b >> 6, (b + n + 63) >> 6))


def n_slabs_of(blocks, slab_blocks):
    """include/garlic_hip.h: a slab begins at the next block the call scores and spans slab_blocks consecutive blocks"""
    n, i = 0, 0
    while i < len(blocks):
        end = blocks[i] + slab_blocks
        n += 1
        while i < len(blocks) and blocks[i] < end:
            i += 1
    return n


def block_bytes(nloci):
    return (ROWS_PAD + nloci) * 64 * 8


def nind_pad_of(nind):
    """the library's padded individual count: the columns of the whole term matrix (a pad block when less than one is free)"""
    return (nind + 126) // 64 * 64


def blocks_needed(slab_blocks, nind):
    """include/garlic_hip.h: one buffer holds a full slab, the other what the second slab holds"""
    nblk = (nind + 63) // 64
    return slab_blocks + min(slab_blocks, nblk - slab_blocks)


def budget_for(nloci, slab_blocks, nind):
    """the smallest budget that holds the buffers of slabs of slab_blocks blocks"""
    return blocks_needed(slab_blocks, nind) * block_bytes(nloci)


def slab_blocks_for(budget, nloci, nind):
    """include/garlic_hip.h: the largest slab whose buffers fit in the budget"""
    return max([s for s in range(1, (nind + 63) // 64 + 1) if blocks_needed(s, nind) * block_bytes(nloci) <= budget], default=0)


def oracle_segments(chroms, scores, W, cutoff):
    out = []
    for c, (g, f, p, cs, ce) in enumerate(chroms):
        cov = ol.oracle_roh_coverage(np.ascontiguousarray(scores[c]), W, cutoff)
        out += [(i, c, a, b) for i, a, b in ol.oracle_roh_segments(cov, p, cs, ce, W, MG, FRAC)]
    return sorted(out)
