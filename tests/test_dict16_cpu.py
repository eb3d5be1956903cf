"""No GPU: the interface of the 16-bit likelihood dictionary (garlic_panel_set_gl_codes16, GARLIC_TGLS_DICTIONARY16), and
with the oracle alone that every panel of tests/test_gpu_dict16.py has finite scores to compare and that a window sum of
exactly -9999.0 can be excluded up front for every width but the one built for it."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import dict16_cases as cases
import oracle_lib as ol
import tgls_slab_cases as scases
from garlic_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "garlic_panel_set_gl_codes16"


def test_header_binding_and_library_list_the_call_and_the_mode_under_abi_8():
    h = open(os.path.join(ROOT, "include", "garlic_hip.h")).read()
    assert "#define GARLIC_HIP_ABI_VERSION 8" in h and abi.ABI_VERSION == 8
    assert abi.lib().garlic_hip_abi_version() == 8
    assert re.search(r"^int %s\(garlic_panel \*panel, const uint16_t \*codes," % NAME, h, re.M)
    assert re.search(r"^#define GARLIC_TGLS_DICTIONARY16 3$", h, re.M) and abi.TGLS_DICTIONARY16 == 3
    assert (abi.TGLS_DICTIONARY, abi.TGLS_CONTINUOUS) == (1, 2)
    history = h[: h.index("#define GARLIC_HIP_ABI_VERSION")]
    assert re.search(r"\* 8:.*%s, GARLIC_TGLS_DICTIONARY16" % NAME, history, re.S)
    assert NAME in abi.SYMBOLS and hasattr(C.CDLL(abi.LIB_PATH), NAME)
    assert hasattr(abi.Panel, "set_gl_codes16")
    doc = h[h.index("GenoLikeData::data (src/garlic-data.h:91)"): h.index("int garlic_panel_set_gl(")]
    for word in ("GARLIC_TGLS_DICTIONARY ", "GARLIC_TGLS_DICTIONARY16", "GARLIC_TGLS_CONTINUOUS", "Transitions", "65,536"):
        assert word in doc, word
    budget = h[h.index("Unweighted scores from dictionary-coded likelihoods run in two passes"): h.index("int garlic_panel_set_tgls_term_budget(")]
    assert "GARLIC_TGLS_DICTIONARY16" in budget and "GARLIC_ERR_NOMEM" in budget


def test_the_term_kernel_is_in_the_built_library():
    blob = open(abi.LIB_PATH, "rb").read()
    for kernel in (b"gl_terms_wide_kernel", b"gl_widen_kernel", b"gl_decode16_kernel", b"gl_recode16_kernel"):
        assert kernel in blob, kernel


@pytest.mark.parametrize("nvalues", cases.NVALUES)
def test_tables_and_codes(nvalues):
    values, codes, gl = cases.codes_of(nvalues)
    assert values.shape == (nvalues,) and np.unique(values).shape[0] == nvalues
    assert values.min() == 1e-16 and values.max() == 1.0 and (values > 0).all()
    allc = np.concatenate([c.ravel() for c in codes])
    assert allc.dtype == np.uint16 and int(allc.max()) < nvalues
    assert np.unique(allc).shape[0] > 256                     # never a one-byte dictionary
    assert (np.concatenate([g.ravel() for g in gl]) == 1e-16).any() and (np.concatenate([g.ravel() for g in gl]) == 1.0).any()
    if nvalues == 65536:
        assert int(allc.max()) > 60000                        # codes of the table's far end are in use


def test_panel_shape():
    chroms, gpos = cases.panel()
    assert [c[0].shape for c in chroms] == [(700, 130), (99, 130), (41, 130)]
    g, f, p, cs, ce = chroms[0]
    assert (np.diff(p.astype(np.int64)) > cases.MG).sum() == 1
    assert cs < ce and ((p >= cs) & (p <= ce)).any()
    miss = np.mean(np.concatenate([(c[0] == -9).ravel() for c in chroms]))
    assert 0.005 < miss < 0.015
    assert scases.nind_pad_of(cases.NIND) == 256 and (cases.NIND + 63) // 64 == 3
    assert [scases.slab_blocks_for(b, sum(cases.SIZES), cases.NIND) for _, b in cases.budgets()] == [1, 3]
    assert all(np.all(np.diff(x) > 0) for x in gpos)


@pytest.mark.parametrize("nvalues", cases.NVALUES)
def test_scores_are_finite_and_no_window_can_sum_to_the_sentinel(nvalues):
    """every scored window of every width is finite, something is scored on every width's first chromosome, and the bound
    the library takes up front (W x (log10 of the smallest value - 1e-6)) keeps the widths of the score tests out of the
    by-value regime and puts EXACT_W into it"""
    values = cases.codes_of(nvalues)[0]
    bound = math.log10(values.min()) - 1e-6
    for W in cases.WIDTHS:
        assert W * bound > -9990.0
        scores = cases.lod_scores(nvalues, W)
        scored = np.concatenate([s[s != ol.MISSING] for s in scores])
        assert scored.size > 0 and np.isfinite(scored).all()
        assert not (np.concatenate([s.ravel() for s in scores]) == ol.MISSING).all()
        # nothing below the bound: the smallest window sum is at least W x bound
        assert scored.min() >= W * bound
    assert cases.EXACT_W * bound <= -9990.0


def test_the_sentinel_case_has_scored_windows():
    chroms, values, codes, gl, scores = cases.exact_case()
    assert values.min() == 1e-16 and cases.EXACT_W * (math.log10(values.min()) - 1e-6) <= -9990.0
    scored = scores[0][scores[0] != ol.MISSING]
    assert scored.size == 70 * (700 - cases.EXACT_W + 1) and np.isfinite(scored).all()


def test_reader_takes_one_byte_16_bit_or_double_form(tmp_path):
    """tests/host_unit/tgls_forms_unit.cpp (compiled here, ASan + UBSan; a stand-alone program): readTGLSData(compact = true) on
    GL-typed texts it writes itself -- 256 distinct values: the one-byte codes and table of the linear-scan reader; 257: 16-bit
    codes that decode to the doubles of compact = false; 65,536: still 16-bit; 65,537: doubles -- and the monomorphic-site
    filter keeping rows and values aligned in every form"""
    exe = str(tmp_path / "tgls_forms_unit")
    libdir = os.path.join(ROOT, "garlic_amd")
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                         "-o", exe, os.path.join(ROOT, "tests", "host_unit", "tgls_forms_unit.cpp"),
                         os.path.join(libdir, "host", "garlic_host.cpp"), "-L" + libdir, "-lgarlic_hip", "-lz",
                         "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and "tgls_forms_unit ok" in r.stdout, (r.stdout + r.stderr)[-3000:]


def test_the_tool_no_longer_stops_at_256_values():
    src = open(os.path.join(ROOT, "garlic_amd", "host", "garlic_host.cpp")).read()
    assert "more than 256 distinct genotype likelihood values" not in src
    assert "garlic_panel_set_gl_codes16(" in src
