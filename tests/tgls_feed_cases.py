"""The (panel, window, step) cases of the thinned TGLS feed (tests/test_gpu_tgls_feed.py runs them on the GPU,
tests/test_tgls_feed_cpu.py checks with the oracle alone that none of them is an empty feed)."""
import os
import re

import numpy as np

import oracle_lib as ol
from wlod_feed_cases import MG, ERROR, chrom_sizes, flat, thinned_doubles   # noqa: F401  (re-exported)

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "garlic_amd", "csrc")
MIN_STEP = 4                     # feed_single: smaller steps keep the full scores


def single_max_w():
    """the last window width of the one-stream form, from the constants the kernels are built with (tgls_feed_kernel
    shares lod_chain_ring_kernel's ring: TG_SINGLE_MAX_W = TG_RING - 32 - 4 * TG_GROUP * 2)"""
    ring_src = open(os.path.join(CSRC, "tgls_ring_kernel.hpp")).read()
    ring = int(re.search(r"^#define GARLIC_TG_RING (\d+)\s*$", ring_src, re.M).group(1))
    group = int(re.search(r"^constexpr int TG_GROUP = (\d+);", ring_src, re.M).group(1))
    assert re.search(r"TG_SINGLE_MAX_W = TG_RING - 32 - 4 \* TG_GROUP \* 2;", ring_src)
    return ring - 32 - 4 * group * 2


def widths():
    s = single_max_w()
    return sorted({2, 10, 31, 32, 33, 100, s, s + 1, 300, 1000})


def extra_step_widths():
    """also step = W + 7, 2 W, 4 and one beyond the longest chromosome: narrow, tile edge, both sides of the stream switch, wide"""
    s = single_max_w()
    return [10, 33, 100, s, s + 1, 300, 1000]


NINDS = [1, 63, 64, 65, 200]
GL_WIDTHS = [10, 100, 300]
SUBSET_NIND = 200                # four 64-individual blocks
# unordered lists: blocks {0, 2} / {1} / {1, 3} / {2} / {0, 2, 3} -- two, three, two, three and ONE of the four left out
SUBSETS = [[130, 3, 190, 129, 0], [77], [199, 64], [150, 131], [130, 3, 199, 0]]


def nind_of(W):
    """1 .. 200 individuals spread over the widths so that the widths with every step see 63, 200, 64, 1, 65 of them"""
    return NINDS[(3 * widths().index(W) + 1) % len(NINDS)]


def steps_of(W, sizes):
    """step = W (the reference's thinning; W = 2: the smallest step that is thinned at all) and the extras"""
    return [max(W, MIN_STEP)] + ([W + 7, 2 * W, MIN_STEP, max(sizes) + 5] if W in extra_step_widths() else [])


def make_case(W, nind, seed, sizes=None):
    """chromosomes of 1, W-1, W, W+1, W+33 SNPs, a long one with gaps above max_gap and a centromere holding SNPs, and
    one that is no multiple of 32"""
    rng = np.random.default_rng(seed)
    sizes = sizes or chrom_sizes(W)
    return [ol.random_panel(rng, n, nind, max_gap=MG, gaps=3 if k == 5 else 0, centro=k >= 5) for k, n in enumerate(sizes)]


def bounded_likelihoods(rng, chroms, kind):
    """error values >= 1e-6 (GQ <= 60): every finite term stays above about -7.5, so that 1000 of them stay above
    -9990 and the sampled form is due at every width here (lod_exact_needed).  'codes': a handful of values (the
    dictionary form); 'continuous': more values than the dictionary holds"""
    if kind == "codes":
        return [rng.choice([1e-6, 1e-3, 0.01, 0.2], size=c[0].shape) for c in chroms]
    return [rng.uniform(1e-6, 0.3, size=c[0].shape) for c in chroms]


def kind_of(W):
    return "codes" if widths().index(W) % 2 == 0 else "continuous"


def shape_case(W):
    nind = nind_of(W)
    chroms = make_case(W, nind, 7100 + W)
    gl = bounded_likelihoods(np.random.default_rng(7200 + W), chroms, kind_of(W))
    return nind, chroms, gl


def tgls_scores(chroms, gl, W, error=ERROR):
    """the oracle's full TGLS scores, per chromosome [nind][nloci]"""
    return [ol.oracle_calc_lod(g, f, p, cs, ce, W, error, MG, gl=gl[c], threads=8) for c, (g, f, p, cs, ce) in enumerate(chroms)]


# ---- the other cases of tests/test_gpu_tgls_feed.py: (chroms, likelihoods, ...) built here so that tests/test_tgls_feed_cpu.py
#      can check with the oracle alone that each of their calls has something to compare

def likelihood_case(W, kind):
    """dictionary codes or continuous values with the clamp values 1e-16 and 1.0 among them; steps W, W + 7, 4"""
    from wlod_feed_cases import likelihoods
    nind = 130 if W % 4 else 65
    chroms = make_case(W, nind, 7300 + W)
    gl = likelihoods(np.random.default_rng(7400 + W), chroms, kind)
    for e in gl:
        e[::7, ::3] = 1e-16
        e[3::11, 1::5] = 1.0
    return nind, chroms, gl, [W, W + 7, MIN_STEP]


def codes_case():
    """a panel fed by codes + values: (W, nind, chroms, codes, values, likelihoods, steps)"""
    W, nind = 60, 70
    chroms = make_case(W, nind, 7500)
    values = np.array([1e-16, 1e-3, 0.01, 0.2, 1.0])
    rng = np.random.default_rng(7501)
    codes = [rng.integers(0, len(values), size=c[0].shape).astype(np.uint8) for c in chroms]
    return W, nind, chroms, codes, values, [values[k] for k in codes], [W, 2 * W + 1]


def subset_case(W):
    chroms = make_case(W, SUBSET_NIND, 7600 + W)
    gl = bounded_likelihoods(np.random.default_rng(7700 + W), chroms, "codes" if W == 10 else "continuous")
    return SUBSET_NIND, chroms, gl


def nonfinite_case(W):
    """a NaN frequency, likelihoods of 0 and infinity; steps W and 4"""
    nind = 70 if W % 2 else 130
    sizes = chrom_sizes(W) + [2 * W + 100, 2 * W + 140]
    chroms = make_case(W, nind, 7800 + W, sizes=sizes)
    gl = bounded_likelihoods(np.random.default_rng(7900 + W), chroms, "continuous")
    chroms[-1][1][W + 7] = np.nan
    gl[-2][W // 2, ::2] = 0.0
    gl[-2][W + 20, 1::4] = np.inf
    return nind, chroms, gl, [W, MIN_STEP]


def fallback_case():
    """(W, nind, chroms, likelihoods, steps): the thinned step W and the steps 1 and 3 that keep the full scores"""
    W, nind = 60, 65
    chroms = make_case(W, nind, 8000)
    return W, nind, chroms, bounded_likelihoods(np.random.default_rng(8001), chroms, "codes"), [W, 1, 3]


def exact_case():
    """W = 1000 with likelihoods of 1e-16: W times the most negative term passes -9999; then W = 100 on the same panel"""
    from wlod_feed_cases import likelihoods
    W, nind = 1000, 64
    chroms = make_case(W, nind, 8100, sizes=[W + 33, 3 * W + 500])
    return W, 100, nind, chroms, likelihoods(np.random.default_rng(8101), chroms, "codes")


def neighbour_case(W):
    """(nind, chroms, gpos, lds, likelihoods, steps of the thinned calls)"""
    import wlod_feed_cases as wcases
    nind = 130
    chroms, gpos, lds = wcases.make_case(W, nind, 8200 + W)
    gl = bounded_likelihoods(np.random.default_rng(8300 + W), chroms, "codes" if W == 20 else "continuous")
    return nind, chroms, gpos, lds, gl, [W, W + 7, 2 * W]


def random_case(seed):
    """(W, step, nind, chroms, likelihoods, subset) drawn from a seeded generator"""
    rng = np.random.default_rng(20261000 + seed)
    W = int(rng.choice([4, 7, 23, 64, 150, 260]))
    nind = int(rng.integers(1, 260))
    step = max(MIN_STEP, W + int(rng.choice([0, 0, 1, 13, W, -W // 2])))
    sizes = [int(rng.integers(W + 40, 2500)) for _ in range(int(rng.integers(1, 5)))] + [int(rng.integers(1, W + 3))]
    rp = np.random.default_rng(int(rng.integers(1 << 30)))
    chroms = [ol.random_panel(rp, n, nind, max_gap=MG, gaps=int(rng.integers(0, 3))) for n in sizes]
    gl = bounded_likelihoods(rp, chroms, "codes" if seed % 2 else "continuous")
    idx = rp.permutation(nind)[: max(1, nind // 3)]
    return W, step, nind, chroms, gl, idx


def repeat_case():
    W, nind = 100, 200
    chroms = make_case(W, nind, 8400)
    return W, nind, chroms, bounded_likelihoods(np.random.default_rng(8401), chroms, "continuous")
