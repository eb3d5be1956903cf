"""No GPU: with the oracle alone, that every case of tests/test_gpu_wlod_slabs.py has something to compare -- scored
windows in every chromosome that can hold one, a non-empty feed for every individual list, covered SNPs and at least one
ROH segment -- and that the slab rule of tests/tgls_slab_cases.py gives the slab counts the GPU test asserts.  Also the
interface: the header says which weighted shapes look their terms up, and the built library holds the slab builder with
its decay-table argument."""
import os
import re

import numpy as np
import pytest

import oracle_lib as ol
import wlod_slab_cases as cases
from garlic_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PANELS = [(W, cases.NIND) for W in cases.WIDTHS] + [(cases.WIDE_W, cases.NIND_WIDE)]


def test_widths_take_the_four_kernel_forms():
    """the dispatcher's thresholds, from its source: a group of 16 windows, 7 and 15 compute waves per strip workgroup"""
    src = open(os.path.join(ROOT, "garlic_amd", "csrc", "wlod_strip_kernel.hpp")).read()
    var = open(os.path.join(ROOT, "garlic_amd", "csrc", "variant_kernels.hpp")).read()
    r = int(re.search(r"constexpr int WLOD_R = (\d+);", var).group(1))
    narrow = int(re.search(r"constexpr int WS_WAVES = (\d+);", src).group(1))
    wide = int(re.search(r"constexpr int WS_WAVES_WIDE = (\d+);", src).group(1))
    strip_max = lambda waves: 16 * waves + 16 - 15                  # W + 15 - 16 waves <= 16
    assert (r, strip_max(narrow), strip_max(wide)) == (16, 113, 241)
    assert cases.WIDTHS == [10, 100, 200, 260]
    assert cases.WIDTHS[0] < r <= cases.WIDTHS[1] <= strip_max(narrow) < cases.WIDTHS[2] <= strip_max(wide) < cases.WIDTHS[3]


def test_slab_counts_the_gpu_test_asserts():
    nloci = sum(cases.sizes_of(100))
    got = []
    for nind in (cases.NIND, cases.NIND_WIDE):
        for k, budget in cases.budgets_of(nloci, nind):
            s = cases.slab_blocks_for(budget, nloci, nind)
            assert s == k and budget < cases.block_bytes(nloci) * (cases.nind_pad_of(nind) // 64)
            got.append(cases.n_slabs_of(cases.blocks_of(nind), s))
    assert got == [4, 1, 4, 3]
    # the subset feeds: one-block slabs run a slab per listed block, one slab of four holds every list
    assert [cases.n_slabs_of(cases.blocks_of(cases.NIND, idx=x), 1) for x in cases.SUBSETS] == [3, 2, 2, 2]
    assert [cases.n_slabs_of(cases.blocks_of(cases.NIND, idx=x), 4) for x in cases.SUBSETS] == [1, 1, 1, 1]
    assert [cases.n_slabs_of(cases.blocks_of(cases.NIND_WIDE, idx=x), 2) for x in cases.WIDE_SUBSETS] == [4, 3]
    assert [cases.n_slabs_of(cases.blocks_of(cases.NIND_WIDE, idx=x), 3) for x in cases.WIDE_SUBSETS] == [3, 2]
    # the sub-ranges: blocks 1 and 2; the unaligned one begins inside block 1
    assert cases.blocks_of(cases.NIND, sub=cases.SUB_RANGE) == [1, 2] and cases.SUB_RANGE[0] % 64 == 0
    assert cases.UNALIGNED_RANGE[0] % 64 != 0 and sum(cases.UNALIGNED_RANGE) <= cases.NIND


@pytest.mark.parametrize("W,nind", PANELS)
def test_every_case_has_something_to_compare(W, nind):
    chroms, codes, gl, gpos, lds = cases.case(W, nind)
    scores = cases.scores_of(W, nind)
    assert [c[0].shape[0] for c in chroms] == cases.sizes_of(W) and chroms[0][0].shape[1] == nind
    assert all(ld.shape == (c[0].shape[0], W) and ld.min() >= 1.0 and ld.max() <= max(2.0, W / 4.0) for ld, c in zip(lds, chroms))
    assert all(np.all(np.diff(g) > 0) for g in gpos if len(g) > 1)
    for c, s in enumerate(scores):
        scored = np.isfinite(s) & (s != ol.MISSING)
        assert s.shape == (nind, chroms[c][0].shape[0])
        if s.shape[1] >= W:
            assert scored.any(axis=1).all(), (W, c)          # every individual has a scored window there
        else:
            assert not scored.any(), (W, c)
    subsets = cases.SUBSETS if nind == cases.NIND else cases.WIDE_SUBSETS
    for step, idx in [(W, None), (3, None)] + [(W, np.array(x)) for x in subsets]:
        assert sum(len(x) for x in cases.flat(scores, step, idx)) > 0, (W, step, idx)
    for b, n in (cases.SUB_RANGE, cases.UNALIGNED_RANGE):
        assert any(np.any(np.isfinite(s[b: b + n]) & (s[b: b + n] != ol.MISSING)) for s in scores)
    cutoff = cases.cutoff_of(scores)
    covered = sum(int(np.count_nonzero(ol.oracle_roh_coverage(np.ascontiguousarray(s), W, cutoff))) for s in scores)
    assert covered > 0
    assert len(cases.oracle_segments(chroms, scores, W, cutoff)) > 0


def test_second_scale_gives_other_scores():
    """the sequence test's (M, mu) = (3, 2e-9) must not be satisfied by terms scaled for (7, 1e-9)"""
    a, b = cases.scores_of(100), cases.scores_of(100, cases.NIND, cases.M2, cases.MU2)
    differing = sum(int(np.count_nonzero(x.view(np.uint64) != y.view(np.uint64))) for x, y in zip(a, b))
    scored = sum(int(np.count_nonzero(x != ol.MISSING)) for x in a)
    assert scored > 0 and differing > scored // 2


def test_header_states_the_weighted_rule_and_the_look_up_shapes():
    h = open(os.path.join(ROOT, "include", "garlic_hip.h")).read()
    assert "#define GARLIC_HIP_ABI_VERSION 8" in h and abi.ABI_VERSION == 8
    comment = h[h.index("Unweighted scores from dictionary-coded likelihoods run in two passes"): h.index("int garlic_panel_set_tgls_term_budget(")]
    assert "built whole as before and outside this bound" not in comment
    for phrase in ("garlic_wlod_windows", "GARLIC_FEED_SAMPLED_WLOD", "looks its terms up", "multiple of 64", "GARLIC_WLOD_GENERIC"):
        assert phrase in comment, phrase
    info = h[h.index("int garlic_panel_set_tgls_term_budget("): h.index("int garlic_panel_tgls_terms_info(")]
    assert "weighted or not" in info


def test_the_slab_builder_takes_a_decay_table():
    """gl_terms_slab_kernel(VariantArgs, long, long, int, int, const double *decay, double *terms)"""
    blob = open(abi.LIB_PATH, "rb").read()
    assert b"gl_terms_slab_kernelENS_11VariantArgsElliiPKdPd" in blob
