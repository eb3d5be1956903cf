"""The panels of the 16-bit likelihood dictionary (GARLIC_TGLS_DICTIONARY16): tests/test_gpu_dict16.py runs them on the
GPU, tests/test_dict16_cpu.py checks with the oracle alone that each has finite scores to compare.

One panel shape: 3 chromosomes of 700 / 99 / 41 SNPs (the first with a gap above max_gap and a centromere that holds
SNPs), 130 individuals (two full 64-individual blocks and a ragged one), 1 % missing genotypes.  Likelihood tables of
257 (one past the one-byte dictionary), 1,000 and 65,536 (the full 16-bit table) distinct values in (0, 1], the clamp
values 1e-16 and 1.0 of readTGLSData among them."""
import functools

import numpy as np

import oracle_lib as ol
import tgls_feed_cases as fcases
import tgls_slab_cases as scases

MG, ERROR, FRAC = fcases.MG, fcases.ERROR, scases.FRAC
SIZES = [700, 99, 41]
NIND = 130
NVALUES = [257, 1000, 65536]
WIDTHS = [2, 10, 40, 100]
FEED_SIZES = [10, 40, 100]
EXACT_W = 640          # 640 x log10(1e-16) = -10240 <= -9990: a window sum of exactly -9999.0 cannot be excluded up front
M, MU = 7, 1e-9
ROWS_PAD = scases.ROWS_PAD


def table(nvalues):
    """nvalues distinct doubles in (0, 1]: 1.0 down to 1e-5 in equal steps of the exponent (what a printed GL column
    converts to) and 1e-16, in a shuffled order (codes are not sorted by value)"""
    v = np.concatenate([10.0 ** (-5.0 * np.arange(nvalues - 1) / (nvalues - 2)), [1e-16]])
    assert v[0] == 1.0 and np.unique(v).shape[0] == nvalues and v.min() == 1e-16 and v.max() == 1.0
    return np.random.default_rng(16000 + nvalues).permutation(v)


@functools.lru_cache(maxsize=None)
def panel(seed=0):
    rng = np.random.default_rng(16100 + seed)
    chroms = [ol.random_panel(rng, n, NIND, miss=0.01, max_gap=MG, gaps=1 if k == 0 else 0, centro=k == 0)
              for k, n in enumerate(SIZES)]
    gpos = [np.cumsum(np.diff(c[2], prepend=0) * 1e-6 * rng.uniform(0.8, 1.2, size=c[2].shape[0])) for c in chroms]
    return chroms, gpos


@functools.lru_cache(maxsize=None)
def codes_of(nvalues, seed=0):
    """(values, codes per chromosome [nloci][nind] uint16, the doubles they stand for).  The rare clamp value 1e-16 is kept
    rare (as in a real column): the windows of WIDTHS then stay far above -9990."""
    rng = np.random.default_rng(16200 + nvalues + seed)
    values = table(nvalues)
    codes = [rng.integers(0, nvalues, size=c[0].shape).astype(np.uint16) for c in panel()[0]]
    lo, hi = int(np.argmin(values)), int(np.argmax(values))
    for c in codes:
        c[::7, ::5] = lo
        c[3::11, 1::4] = hi
    return values, codes, [values[c] for c in codes]


@functools.lru_cache(maxsize=None)
def lod_scores(nvalues, W, freq_seed=0):
    chroms = with_freq(freq_seed)
    gl = codes_of(nvalues)[2]
    return [ol.oracle_calc_lod(g, f, p, cs, ce, W, ERROR, MG, gl=gl[c], threads=8) for c, (g, f, p, cs, ce) in enumerate(chroms)]


def wlod_scores(nvalues, W, lds, freq_seed=0, M_=M, mu=MU):
    """lds: the LD weights per chromosome [nloci_c][W] (those garlic_panel_compute_ld installed)"""
    chroms, gpos = with_freq(freq_seed), panel()[1]
    gl = codes_of(nvalues)[2]
    return [ol.oracle_calc_wlod(g, f, p, gpos[c], lds[c], cs, ce, W, ERROR, MG, mu, M_, gl=gl[c], threads=8)
            for c, (g, f, p, cs, ce) in enumerate(chroms)]


@functools.lru_cache(maxsize=None)
def with_freq(freq_seed):
    """the panel with other allele frequencies (a new --freq-file): freq_seed 0 is the panel itself"""
    chroms = panel()[0]
    if freq_seed == 0:
        return chroms
    rng = np.random.default_rng(16300 + freq_seed)
    return [(g, rng.uniform(0.05, 0.95, size=f.shape), p, cs, ce) for g, f, p, cs, ce in chroms]


def split_ld(ld):
    """[nloci][W] of the whole panel -> per chromosome"""
    out, at = [], 0
    for n in SIZES:
        out.append(np.ascontiguousarray(ld[at: at + n]))
        at += n
    return out


def budgets():
    """(slab_blocks, budget): one-block slabs (3 slabs on the 3 blocks), and one slab of all 3 blocks (the whole matrix has a
    pad block more and does not fit).  Two slabs cannot be forced on three blocks: the slabs of a call alternate between two
    buffers, so slabs of 2 blocks cost 2 + 1 blocks, as much as the single slab of 3, which the library then takes
    (include/garlic_hip.h).  Two slabs run on a range of two blocks under the one-block budget, and on exact_case()."""
    nloci = sum(SIZES)
    return [(k, scases.budget_for(nloci, k, NIND)) for k in (1, 3)]


@functools.lru_cache(maxsize=None)
def exact_case():
    """(chroms, values, codes, doubles, oracle scores at EXACT_W): one chromosome of 700 SNPs without gap or centromere, so
    that windows of EXACT_W SNPs exist; 70 individuals; the 257-value table, which holds 1e-16"""
    rng = np.random.default_rng(16500)
    chroms = [ol.random_panel(rng, 700, 70, miss=0.01, max_gap=MG, gaps=0, centro=False)]
    values = table(257)
    codes = [rng.integers(0, 257, size=chroms[0][0].shape).astype(np.uint16)]
    gl = [values[codes[0]]]
    g, f, p, cs, ce = chroms[0]
    return chroms, values, codes, gl, [ol.oracle_calc_lod(g, f, p, cs, ce, EXACT_W, ERROR, MG, gl=gl[0], threads=8)]
