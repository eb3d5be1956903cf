"""No GPU: the thinned TGLS feed's interface and code object.

Header, binding and built library agree on GARLIC_FEED_TGLS_CHAIN under ABI 8; the gfx950 code object of the built library
holds tgls_feed_kernel; the header names the switch GARLIC_TGLS_FEED_FULL; and every case of tests/test_gpu_tgls_feed.py
is a non-empty feed by the oracle alone (an empty one would compare nothing there)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle_lib as ol
import tgls_feed_cases as cases
import wlod_feed_cases as wcases
from garlic_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = b"_ZN6garlic16tgls_feed_kernelENS_12TglsFeedArgsE"


def header():
    return open(os.path.join(ROOT, "include", "garlic_hip.h")).read()


def test_constant_declared_and_bound_under_abi_8():
    h = header()
    for name, value in (("GARLIC_FEED_FROM_SCORES", 0), ("GARLIC_FEED_CHAIN", 1), ("GARLIC_FEED_SAMPLED_WLOD", 2),
                        ("GARLIC_FEED_TGLS_CHAIN", 3)):
        assert re.search(r"#define %s %d\b" % (name, value), h), name
    assert abi.FEED_TGLS_CHAIN == 3
    assert "#define GARLIC_HIP_ABI_VERSION 8" in h and abi.ABI_VERSION == 8
    assert abi.lib().garlic_hip_abi_version() == 8
    history = h[: h.index("#define GARLIC_HIP_ABI_VERSION")]
    assert re.search(r"\* 8:.*GARLIC_FEED_TGLS_CHAIN", history, re.S)
    assert hasattr(C.CDLL(abi.LIB_PATH), "garlic_lod_feed_info")


def test_kernel_symbol_in_the_built_library():
    """the shipped library embeds a gfx950 code object that names the kernel; the ring kernel it is built from is still there"""
    blob = open(abi.LIB_PATH, "rb").read()
    assert KERNEL in blob
    assert b"_ZN6garlic21lod_chain_ring_kernelENS_8TglsArgsE" in blob


def test_the_library_knows_the_form_and_the_switch():
    blob = open(abi.LIB_PATH, "rb").read()
    assert b"GARLIC_TGLS_FEED_FULL" in blob


def test_header_names_the_switch_and_the_fallbacks():
    h = header()
    comment = h[h.index("The explore / auto-winsize flows"): h.index("int garlic_lod_feed(")]
    assert "GARLIC_TGLS_FEED_FULL" in comment and "GARLIC_TGLS_NO_RING" in comment
    assert "unweighted per-genotype likelihoods" not in comment        # no longer among "the other variants"
    assert "garlic_panel_chain_kind" in comment


def test_widths_hold_both_sides_of_the_stream_switch():
    s = cases.single_max_w()
    w = cases.widths()
    assert s in w and s + 1 in w and {2, 10, 31, 32, 33, 100, 300, 1000} <= set(w)
    assert all(step >= cases.MIN_STEP for W in w for step in cases.steps_of(W, cases.chrom_sizes(W)))


@pytest.mark.parametrize("W", cases.widths())
def test_every_shape_case_is_a_nonempty_feed(W):
    nind, chroms, gl = cases.shape_case(W)
    sizes = [c[0].shape[0] for c in chroms]
    scores = cases.tgls_scores(chroms, gl, W)
    for step in cases.steps_of(W, sizes):
        per_chr = [len(x) for x in cases.flat(scores, step)]
        assert sum(per_chr) > 0, (W, step)
        assert per_chr[0] == 0                      # the one-SNP chromosome never holds a window
        if step <= W:
            assert per_chr[5] > 0 and per_chr[4] > 0, (W, step, per_chr)


def nonempty(scores, step, idx=None):
    return sum(len(x) for x in cases.flat(scores, step, idx)) > 0


@pytest.mark.parametrize("kind", ["codes", "continuous"])
@pytest.mark.parametrize("W", cases.GL_WIDTHS)
def test_every_likelihood_case_is_a_nonempty_feed(W, kind):
    nind, chroms, gl, steps = cases.likelihood_case(W, kind)
    scores = cases.tgls_scores(chroms, gl, W)
    assert all(nonempty(scores, step) for step in steps), (W, kind)


@pytest.mark.parametrize("W", [10, 100])
def test_every_subset_case_is_a_nonempty_feed(W):
    nind, chroms, gl = cases.subset_case(W)
    scores = cases.tgls_scores(chroms, gl, W)
    for idx in cases.SUBSETS:
        assert nonempty(scores, W, np.array(idx)), (W, idx)


def test_the_subsets_leave_out_one_and_three_of_four_blocks():
    assert (cases.SUBSET_NIND + 63) // 64 == 4
    left_out = {4 - len({i >> 6 for i in idx}) for idx in cases.SUBSETS}
    assert {1, 3} <= left_out and any(len(idx) == 1 for idx in cases.SUBSETS)
    assert all(idx != sorted(idx) for idx in cases.SUBSETS if len(idx) > 2)     # unordered


@pytest.mark.parametrize("W", [5, 60, 300])
def test_the_nonfinite_cases_hold_nan_and_a_feed(W):
    nind, chroms, gl, steps = cases.nonfinite_case(W)
    scores = cases.tgls_scores(chroms, gl, W)
    assert np.isnan(np.concatenate([s.ravel() for s in scores])).any()
    assert all(nonempty(scores, step) for step in steps)


def test_the_codes_fallback_exact_and_repeat_cases_are_nonempty_feeds():
    W, nind, chroms, codes, values, gl, steps = cases.codes_case()
    scores = cases.tgls_scores(chroms, gl, W)
    assert all(nonempty(scores, step) for step in steps)
    W, nind, chroms, gl, steps = cases.fallback_case()
    scores = cases.tgls_scores(chroms, gl, W)
    assert all(nonempty(scores, step) for step in steps)
    W, narrow, nind, chroms, gl = cases.exact_case()
    assert nonempty(cases.tgls_scores(chroms, gl, W), W) and nonempty(cases.tgls_scores(chroms, gl, narrow), narrow)
    W, nind, chroms, gl = cases.repeat_case()
    assert nonempty(cases.tgls_scores(chroms, gl, W), W)


@pytest.mark.parametrize("W", [20, 200])
def test_every_neighbour_case_is_a_nonempty_feed(W):
    nind, chroms, gpos, lds, gl, steps = cases.neighbour_case(W)
    scores = cases.tgls_scores(chroms, gl, W)
    assert all(nonempty(scores, step) for step in steps)
    assert nonempty(wcases.wlod_scores(chroms, gpos, lds, W, gl=gl), W)                     # the weighted neighbour
    assert nonempty([ol.oracle_calc_lod(g, f, p, cs, ce, W, cases.ERROR, cases.MG) for (g, f, p, cs, ce) in chroms], W)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_every_random_case_is_a_nonempty_feed(seed):
    W, step, nind, chroms, gl, idx = cases.random_case(seed)
    scores = cases.tgls_scores(chroms, gl, W)
    assert nonempty(scores, step) and nonempty(scores, step, idx)


def test_thinned_layout_total():
    assert cases.thinned_doubles([1, 99, 100, 3201], 65, 100) == (32 + 32 + 32 + 64) * 128
    assert cases.thinned_doubles([1000], 64, 4) == 256 * 64
