"""No GPU: the sampled-window weighted feed's interface and code object.

Header, binding and built library agree on garlic_lod_feed_info; the gfx950 code object holds wlod_feed_kernel (both
forms) and the compiler's own resource report shows no scratch and no spilled register; and every case of
tests/test_gpu_wlod_feed.py is a non-empty feed by the oracle alone (an empty one would prove nothing there)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
import wlod_feed_cases as cases
from garlic_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "garlic_amd", "csrc")


def test_feed_info_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "garlic_hip.h")).read()
    assert re.search(r"int garlic_lod_feed_info\(garlic_panel \*panel, int32_t \*form, int64_t \*score_doubles\);", header)
    for name, value in (("GARLIC_FEED_FROM_SCORES", 0), ("GARLIC_FEED_CHAIN", 1), ("GARLIC_FEED_SAMPLED_WLOD", 2)):
        assert re.search(r"#define %s %d\b" % (name, value), header), name
    assert (abi.FEED_FROM_SCORES, abi.FEED_CHAIN, abi.FEED_SAMPLED_WLOD) == (0, 1, 2)
    assert "garlic_lod_feed_info" in abi.SYMBOLS
    assert hasattr(C.CDLL(abi.LIB_PATH), "garlic_lod_feed_info")
    assert hasattr(abi.Panel, "feed_info")
    form = C.c_int32()
    assert abi.lib().garlic_lod_feed_info(None, C.byref(form), None) == abi.ERR_INVALID


def test_abi_version_unchanged_and_listed():
    header = open(os.path.join(ROOT, "include", "garlic_hip.h")).read()
    assert "#define GARLIC_HIP_ABI_VERSION 8" in header
    history = header[: header.index("#define GARLIC_HIP_ABI_VERSION")]
    assert re.search(r"\* 8:.*garlic_lod_feed_info", history, re.S)


@pytest.fixture(scope="module")
def device_report(tmp_path_factory):
    """the library's device code compiled once more for gfx950 with the compiler's resource report (what
    tools/asm_stats.sh reads), flags as in garlic_amd/csrc/Makefile"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = tmp_path_factory.mktemp("wlod_feed_asm")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(CSRC, "garlic_hip.hip"), "-o", str(out / "device.o")],
                       capture_output=True, text=True, cwd=str(out))
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stderr


@pytest.mark.parametrize("gl", [False, True])
def test_kernel_in_code_object_without_spills(device_report, gl):
    name = "_ZN6garlic16wlod_feed_kernelILb%dEEEvNS_12WlodFeedArgsE" % int(gl)
    blocks = device_report.split("Function Name: ")
    mine = [b for b in blocks if b.startswith(name)]
    assert len(mine) == 1, "wlod_feed_kernel<%s> is not in the gfx950 code object" % gl

    def field(label):
        m = re.search(re.escape(label) + r": (\d+)", mine[0])
        assert m, label
        return int(m.group(1))
    assert field("ScratchSize [bytes/lane]") == 0
    assert field("SGPRs Spill") == 0 and field("VGPRs Spill") == 0
    assert field("LDS Size [bytes/block]") <= 64 * 1024        # static LDS only
    assert field("Occupancy [waves/SIMD]") >= 2


def test_kernel_symbol_in_the_built_library():
    """the shipped library embeds a gfx950 code object that names both forms"""
    blob = open(abi.LIB_PATH, "rb").read()
    for gl in (0, 1):
        assert (b"_ZN6garlic16wlod_feed_kernelILb%dEEEvNS_12WlodFeedArgsE" % gl) in blob


def test_kernel_is_plain_cpp_without_inline_assembly():
    src = open(os.path.join(CSRC, "wlod_feed_kernel.hpp")).read()
    assert "asm" not in src.replace("assembly", "")


@pytest.mark.parametrize("W", cases.WIDTHS)
def test_every_shape_case_is_a_nonempty_feed(W):
    nind = cases.nind_of(W)
    sizes = cases.chrom_sizes(W)
    chroms, gpos, lds = cases.make_case(W, nind, 5100 + W)
    scores = cases.wlod_scores(chroms, gpos, lds, W)
    for step in cases.steps_of(W, sizes):
        per_chr = [len(x) for x in cases.flat(scores, step)]
        assert sum(per_chr) > 0, (W, step)
        assert per_chr[0] == 0                      # the one-SNP chromosome never holds a window
        if step == W:
            assert per_chr[5] > 0 and per_chr[4] > 0, (W, step, per_chr)


def test_thinned_layout_total():
    assert cases.thinned_doubles([1, 99, 100, 3201], 65, 100) == (32 + 32 + 32 + 64) * 128
    assert cases.thinned_doubles([1000], 64, 7) == 160 * 64
