"""No GPU: the multi-size TGLS feed's declarations, exports and grouping rule, and every case of
tests/test_gpu_tgls_feed_multi.py built and checked with the oracle alone for something to compare."""
import ctypes
import os
import re

import tgls_feed_cases as cases
import tgls_feed_multi_cases as mcases
from garlic_amd import abi

ROOT = mcases.ROOT
HEADER = open(os.path.join(ROOT, "include", "garlic_hip.h")).read()
NAMES = ["garlic_lod_feed_multi_tgls", "garlic_lod_feed_multi_info"]


def test_header_declares_the_calls_and_the_form():
    for name in NAMES:
        assert re.search(r"^int %s\(garlic_panel \*panel," % name, HEADER, re.M), name
    assert re.search(r"^#define GARLIC_FEED_TGLS_CHAIN_SHARED 4\s*$", HEADER, re.M)
    assert abi.FEED_TGLS_CHAIN_SHARED == 4
    assert re.search(r"^#define GARLIC_HIP_ABI_VERSION 8\s*$", HEADER, re.M)


def test_history_comment_lists_them_under_abi_8():
    history = HEADER[HEADER.index("/* 2: the LD functions"): HEADER.index("#define GARLIC_HIP_ABI_VERSION")]
    under_8 = history[history.index(" * 8:"):]
    for name in NAMES + ["GARLIC_FEED_TGLS_CHAIN_SHARED"]:
        assert name in under_8, name


def test_bindings_and_library_export_them():
    lib = ctypes.CDLL(abi.LIB_PATH)
    for name in NAMES:
        assert name in abi.SYMBOLS
        assert hasattr(lib, name), name
    assert hasattr(abi.Panel, "lod_feed_multi_tgls") and hasattr(abi.Panel, "feed_multi_info")


def test_header_states_the_limits_the_kernel_is_built_with():
    """the rule's two numbers in include/garlic_hip.h are the kernel's constants"""
    assert "at most %d (TGM_MAX_SIZES)" % mcases.max_sizes() in HEADER
    assert "<= %d (the one-stream ring's widest window)" % cases.single_max_w() in HEADER
    assert "GARLIC_TGLS_FEED_MULTI_SOLO=1" in HEADER


def test_grouping_rule():
    """the documented rule on the size lists of the GPU tests (written out for TGM_MAX_SIZES = 4, W <= 144)"""
    g = lambda ws, **kw: mcases.groups_of(ws, limit=4, max_w=144, **kw)
    assert g([5, 10, 33]) == [0, 0, 0]
    assert g([31, 32, 33, 64]) == [0, 0, 0, 0]
    assert g([60, 60]) == [0, 0]
    assert g([8, 20, 47, 64, 100, 144]) == [0, 0, 0, 0, 1, 1]
    assert g([144, 20, 100, 8, 64, 47]) == [1, 0, 1, 0, 0, 0]          # call order does not matter, sizes do
    assert g([144, 145]) == [0, 1]
    assert g([50, 100, 200, 300]) == [0, 0, 1, 2]
    assert g([300, 50, 200, 100]) == [2, 0, 1, 0]
    # a step-3 size and an exact one do not take the ring: numbered after the ring groups, ascending
    assert g([10, 1000, 50, 100], ring_ok=[False, False, True, True]) == [1, 2, 0, 0]
    assert g([10, 50, 100], solo=True) == [0, 1, 2]
    assert mcases.shared_of([0, 0, 1, 2]) == [True, True, False, False]
    # ... and with the constants of this build
    m, s = mcases.max_sizes(), cases.single_max_w()
    many = mcases.size_lists()["many"]
    assert len(many) == m + 2 and max(many) <= s
    assert sorted(set(mcases.groups_of(many))) == [0, 1]
    assert mcases.groups_of([s, s + 1]) == [0, 1]


def test_every_gpu_case_has_something_to_compare():
    """each size's expected feed is non-empty; where a chromosome holds no window of a size, another one does"""
    n_calls = 0
    for what, want in mcases.all_calls():
        for k, per_chr in enumerate(want):
            assert sum(len(x) for x in per_chr) > 0, (what, k)
        n_calls += 1
    assert n_calls >= 25


def test_shape_cases_have_a_chromosome_only_some_sizes_fit():
    for name, ws in mcases.size_lists().items():
        sizes = mcases.chrom_sizes(ws)
        if min(ws) < max(ws):
            assert any(min(ws) < n < max(ws) for n in sizes), name
        for n in (1, min(ws) - 1, min(ws), max(ws), max(ws) + 1, max(ws) + 33):
            assert n in sizes, (name, n)
