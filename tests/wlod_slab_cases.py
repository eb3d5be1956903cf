"""The panels, weights, budgets and calls of the weighted scores over TGLS term slabs (tests/test_gpu_wlod_slabs.py runs them
on the GPU, tests/test_wlod_slabs_cpu.py checks with the oracle alone that every one of them has something to compare).

The panels are those of tests/tgls_slab_cases.py (same generator, same dictionary, same chromosome sizes) with genetic
positions added.  The LD weights are an input here: random values in [1, W / 4] handed to garlic_panel_set_ld -- no LD
kernel and no LD oracle runs (the reference's LD is O(nloci W^2 nsub))."""
import functools

import numpy as np

import oracle_lib as ol
import tgls_slab_cases as tcases

MG, ERROR, FRAC = tcases.MG, tcases.ERROR, tcases.FRAC
M, MU = 7, 1e-9
M2, MU2 = 3, 2e-9                    # the second scale of the sequence test
# the stream form (W < 16), the 80-VGPR strip (<= 113), the wide strip (<= 241), the ring tile form (> 241)
WIDTHS = [10, 100, 200, 260]
NIND = tcases.NIND                   # 200: four blocks; a budget of 2 blocks gives one-block slabs (every strip pair loses its
                                     # partner), a budget of 4 blocks one slab
NIND_WIDE = tcases.NIND_WIDE         # 456: eight blocks; slabs of 2 and of 3 (3 + 3 + 2), W = 100 only
WIDE_W = 100
VALUES = tcases.VALUES
SUB_RANGE = tcases.SUB_RANGE         # (64, 100): blocks 1 and 2
UNALIGNED_RANGE = (70, 90)           # begins inside block 1: no slab launch can start there, the terms are looked up
SUBSETS = tcases.SUBSETS
WIDE_SUBSETS = [[130, 3, 455, 0, 300], [455, 64, 200]]          # blocks {0, 2, 4, 7} and {1, 3, 7}

sizes_of = tcases.sizes_of
blocks_of, n_slabs_of, slab_blocks_for, budget_for = tcases.blocks_of, tcases.n_slabs_of, tcases.slab_blocks_for, tcases.budget_for
nind_pad_of, block_bytes, cutoff_of, oracle_segments = tcases.nind_pad_of, tcases.block_bytes, tcases.cutoff_of, tcases.oracle_segments
ROWS_PAD = tcases.ROWS_PAD


@functools.lru_cache(maxsize=None)
def case(W, nind=NIND):
    """(chroms, codes, likelihoods, genetic positions, LD weights) of one panel"""
    chroms, codes, gl, _ = tcases.case(W, nind)
    rng = np.random.default_rng([9100 + 10 * W + nind, 1])        # the case's own seed, a stream of its own
    gpos = [np.cumsum(np.diff(c[2], prepend=0) * 1e-6 * rng.uniform(0.8, 1.2, size=c[2].shape[0])) for c in chroms]
    lds = [rng.uniform(1.0, max(2.0, W / 4.0), size=(c[0].shape[0], W)) for c in chroms]
    return chroms, codes, gl, gpos, lds


@functools.lru_cache(maxsize=None)
def scores_of(W, nind=NIND, m=M, mu=MU):
    """the oracle's weighted scores with likelihoods, per chromosome [nind][nloci_c]; computed once, shared, never written"""
    chroms, _, gl, gpos, lds = case(W, nind)
    out = [ol.oracle_calc_wlod(g, f, p, gpos[c], lds[c], cs, ce, W, ERROR, MG, mu, m, gl=gl[c], threads=8)
           for c, (g, f, p, cs, ce) in enumerate(chroms)]
    for s in out:
        s.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def unweighted_scores_of(W, nind=NIND):
    """the unweighted use_gl scores of the same panel (the sequence test alternates the two kinds)"""
    return tcases.case(W, nind)[3]


def flat(scores, step, idx=None):
    """per-chromosome feeds of the oracle"""
    return [ol.oracle_flatten(s, step) if idx is None else ol.oracle_flatten_subset(s, step, idx) for s in scores]


def thinned_doubles(sizes, nind, step, pitch_align=32):
    """total of the thinned score layout: per chromosome ceil(nloci / step) columns padded to pitch_align, rows to 64"""
    rows = (nind + 63) // 64 * 64
    return sum(((n + step - 1) // step + pitch_align - 1) // pitch_align * pitch_align * rows for n in sizes)


def budgets_of(nloci, nind):
    """(blocks per slab, budget in bytes) of the budgets a panel runs under"""
    if nind == NIND:
        return [(1, budget_for(nloci, 1, nind)), (4, budget_for(nloci, 4, nind))]
    return [(2, budget_for(nloci, 2, nind) + 12345), (3, budget_for(nloci, 3, nind) + 12345)]     # (no multiple of anything)
