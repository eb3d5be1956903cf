"""No GPU: the interface of the TGLS term slabs, and with the oracle alone that every case of
tests/test_gpu_tgls_slabs.py has something to compare: a non-empty feed for every step and individual list, at least one
window at or above the cutoff and at least one ROH segment."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle_lib as ol
import tgls_feed_cases as fcases
import tgls_slab_cases as cases
from garlic_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("garlic_panel_set_tgls_term_budget", "garlic_panel_tgls_terms_info")


def test_header_binding_and_library_list_both_functions_under_abi_8():
    h = open(os.path.join(ROOT, "include", "garlic_hip.h")).read()
    assert "#define GARLIC_HIP_ABI_VERSION 8" in h and abi.ABI_VERSION == 8
    assert abi.lib().garlic_hip_abi_version() == 8
    history = h[: h.index("#define GARLIC_HIP_ABI_VERSION")]
    for name in NAMES:
        assert re.search(r"^int %s\(garlic_panel \*panel," % name, h, re.M), name
        assert name in abi.SYMBOLS and hasattr(C.CDLL(abi.LIB_PATH), name), name
        assert re.search(r"\* 8:.*%s" % name, history, re.S), name
    assert hasattr(abi.Panel, "set_tgls_term_budget") and hasattr(abi.Panel, "tgls_terms_info")
    comment = h[h.index("Unweighted scores from dictionary-coded likelihoods run in two passes"): h.index("int garlic_panel_set_tgls_term_budget(")]
    assert "GARLIC_ERR_INVALID" in comment and "not covered" in comment and "keeps budget 0" in comment


def test_the_slab_kernel_is_in_the_built_library():
    blob = open(abi.LIB_PATH, "rb").read()
    assert b"gl_terms_slab_kernel" in blob


def test_rows_of_a_block_match_the_kernels_constants():
    src = open(os.path.join(ROOT, "garlic_amd", "csrc", "lod_kernels.hpp")).read()
    goff = int(re.search(r"constexpr int GOFF = (\d+);", src).group(1))
    back = int(re.search(r"GPAD_BACK = GPAD_CHAIN > (\d+) \? GPAD_CHAIN : \1;", src).group(1))
    assert goff + back == cases.ROWS_PAD


def test_slab_count_rule():
    assert cases.n_slabs_of([0, 1, 2, 3], 3) == 2 and cases.n_slabs_of([1, 2], 2) == 1 and cases.n_slabs_of([1, 2], 1) == 2
    assert cases.n_slabs_of([0, 3], 2) == 2 and cases.n_slabs_of([2, 3], 2) == 1 and cases.n_slabs_of(list(range(8)), 3) == 3
    left_out = {4 - len(cases.blocks_of(cases.NIND, idx=x)) for x in cases.SUBSETS}
    assert left_out == {1, 2}
    assert cases.WIDTHS == [10, 100, 200] and fcases.single_max_w() == 144
    # 200 individuals: slabs of 1 block, and one slab of all 4 (the whole matrix has a pad block more); 456: slabs of 2 and 3
    blk = cases.block_bytes(1000)
    assert [cases.slab_blocks_for(k * blk, 1000, cases.NIND) for k in (1, 2, 3, 4)] == [0, 1, 1, 4] and cases.nind_pad_of(cases.NIND) == 5 * 64
    assert [cases.slab_blocks_for(k * blk, 1000, cases.NIND_WIDE) for k in (2, 4, 6, 7, 8)] == [1, 2, 3, 3, 8]
    assert cases.slab_blocks_for(blk, 1000, 24) == 1 and cases.nind_pad_of(24) == 128


@pytest.mark.parametrize("nind,subsets,sub_range", [(cases.NIND, cases.SUBSETS, cases.SUB_RANGE),
                                                    (cases.NIND_WIDE, [[130, 3, 455, 0, 300], [455, 64, 200]], (64, 300))])
@pytest.mark.parametrize("W", cases.WIDTHS)
def test_every_case_has_something_to_compare(W, nind, subsets, sub_range):
    chroms, codes, gl, scores = cases.case(W, nind)
    assert [c[0].shape[0] for c in chroms] == cases.sizes_of(W) and chroms[0][0].shape[1] == nind
    assert {1e-16, 1.0} <= set(np.unique(np.concatenate([g.ravel() for g in gl])))
    for step, idx in [(W, None), (4, None), (3, None)] + [(W, np.array(x)) for x in subsets]:
        assert sum(len(x) for x in fcases.flat(scores, step, idx)) > 0, (W, step, idx)
    b, n = sub_range
    assert any(np.any(np.isfinite(s[b: b + n]) & (s[b: b + n] != ol.MISSING)) for s in scores)
    cutoff = cases.cutoff_of(scores)
    assert sum(int(np.count_nonzero(s[np.isfinite(s)] >= cutoff)) for s in scores) > 0
    assert len(cases.oracle_segments(chroms, scores, W, cutoff)) > 0
    # no window of these panels can sum to -9999.0: the tuned chain alone takes every call
    allw = np.concatenate([s.ravel() for s in scores])
    assert float(allw[np.isfinite(allw) & (allw != ol.MISSING)].min()) > -9000
