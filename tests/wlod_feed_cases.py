"""The (panel, window, step) cases of the weighted sampled-window feed (tests/test_gpu_wlod_feed.py runs them on the GPU,
tests/test_wlod_feed_cpu.py checks with the oracle alone that none of them is an empty feed)."""
import numpy as np

import oracle_lib as ol

MG = 200000
ERROR, M, MU = 0.001, 7, 1e-9

# the widths at which the dispatcher changes wLOD kernel form (tests/test_gpu_window_regimes.py): the full path the
# sampled one is compared with is another kernel each time
WIDTHS = [2, 10, 15, 16, 17, 60, 100, 113, 114, 241, 242, 300, 1000]
EXTRA_STEP_WIDTHS = [10, 60, 114, 300]            # also step = W + 7, 2 W, and one beyond the longest chromosome
NINDS = [1, 63, 64, 65, 200]
GL_WIDTHS = [10, 60, 114, 242]


def nind_of(W):
    return NINDS[WIDTHS.index(W) % len(NINDS)]


def chrom_sizes(W):
    """1, W-1, W, W+1, W+33, a big one (gaps, a centromere holding SNPs), one that is no multiple of 32"""
    odd = W + 777 if (W + 777) % 32 else W + 778
    return [1, max(1, W - 1), W, W + 1, W + 33, max(3000, 3 * W + 500), odd]


def make_case(W, nind, seed, sizes=None):
    """chromosomes, genetic positions and LD weights of one case"""
    rng = np.random.default_rng(seed)
    sizes = sizes or chrom_sizes(W)
    chroms = [ol.random_panel(rng, n, nind, max_gap=MG, gaps=3 if k == 5 else 0, centro=k >= 5) for k, n in enumerate(sizes)]
    gpos = [np.cumsum(np.diff(c[2], prepend=0) * 1e-6 * rng.uniform(0.8, 1.2, size=c[2].shape[0])) for c in chroms]
    lds = [rng.uniform(1.0, max(2.0, W / 4.0), size=(n, W)) for n in sizes]
    return chroms, gpos, lds


def steps_of(W, sizes):
    return [W] + ([W + 7, 2 * W, max(sizes) + 5] if W in EXTRA_STEP_WIDTHS else [])


def likelihoods(rng, chroms, kind):
    """kind: 'codes' (a handful of values: the dictionary form) or 'continuous' (more values than the dictionary holds)"""
    if kind == "codes":
        return [rng.choice([1e-16, 1e-3, 0.01, 0.2, 1.0], size=c[0].shape) for c in chroms]
    return [rng.uniform(1e-3, 0.3, size=c[0].shape) for c in chroms]


def wlod_scores(chroms, gpos, lds, W, error=ERROR, gl=None):
    return [ol.oracle_calc_wlod(g, f, p, gpos[c], lds[c], cs, ce, W, error, MG, MU, M, gl=None if gl is None else gl[c], threads=8)
            for c, (g, f, p, cs, ce) in enumerate(chroms)]


def flat(scores, step, idx=None):
    """per-chromosome feeds of the oracle"""
    return [ol.oracle_flatten(s, step) if idx is None else ol.oracle_flatten_subset(s, step, idx) for s in scores]


def thinned_doubles(sizes, nind, step, pitch_align=32):
    """total of the thinned score layout: per chromosome ceil(nloci / step) columns padded to pitch_align, rows to 64"""
    rows = (nind + 63) // 64 * 64
    return sum(((n + step - 1) // step + pitch_align - 1) // pitch_align * pitch_align * rows for n in sizes)
