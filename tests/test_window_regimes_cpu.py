"""The widths at which the dispatcher switches kernel forms, read from the headers, against the widths
tests/test_gpu_window_regimes.py runs: a retune that moves a switch fails here, naming the switch, until the GPU
file tests both sides of it again."""
import os
import re

import test_gpu_window_regimes as regimes

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "garlic_amd", "csrc")


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _const(header, pattern):
    m = re.findall(pattern, _read(header), flags=re.M)
    assert len(m) == 1, (header, pattern, m)
    return int(m[0])


def constants():
    return {
        "GARLIC_TG_RING": _const("tgls_ring_kernel.hpp", r"^#define GARLIC_TG_RING (\d+)\s*$"),
        "TG_GROUP": _const("tgls_ring_kernel.hpp", r"^constexpr int TG_GROUP = (\d+);"),
        "COVF_MAX_W": _const("coverage_kernel.hpp", r"^constexpr int COVF_MAX_W = (\d+);"),
        "WS_WAVES": _const("wlod_strip_kernel.hpp", r"^constexpr int WS_WAVES = (\d+);"),
        "WS_WAVES_WIDE": _const("wlod_strip_kernel.hpp", r"^constexpr int WS_WAVES_WIDE = (\d+);"),
        "WLOD_R": _const("variant_kernels.hpp", r"^constexpr int WLOD_R = (\d+);"),
        "GPAD_BACK": _const("lod_kernels.hpp", r"^constexpr int GPAD_BACK = GPAD_CHAIN > (\d+) \? GPAD_CHAIN : \1;"),
    }


def test_the_switch_formulas_are_the_ones_restated_here():
    """the expressions below are the dispatcher's: if one is rewritten, this test and the boundaries are revisited"""
    assert re.search(r"TG_SINGLE_MAX_W = TG_RING - 32 - 4 \* TG_GROUP \* 2;", _read("tgls_ring_kernel.hpp"))
    assert "const bool single = W <= TG_SINGLE_MAX_W;" in _read("tgls_ring_kernel.hpp")
    hip = _read("garlic_hip.hip")
    assert "(W + 15 - 16 * WS_WAVES <= 16 || getenv(\"GARLIC_WLOD_STRIP_NARROW_ONLY\")) ? WS_WAVES : WS_WAVES_WIDE" in hip
    assert "W + 15 - 16 * strip_waves <= 16" in hip
    assert "!weighted && !use_gl && W <= COVF_MAX_W" in hip
    assert "W + 64 <= GPAD_BACK" in hip
    assert "const bool wlod_small = W < WLOD_R;" in hip


def boundaries(k):
    """(name, last width of the lower form, widths lists that must hold it and the next one)"""
    tg_single_max = k["GARLIC_TG_RING"] - 32 - 4 * k["TG_GROUP"] * 2
    strip_max = lambda waves: max(W for W in range(1, 16 * waves + 64) if W + 15 - 16 * waves <= 16)
    return [
        ("TGLS chain: one stream up to TG_SINGLE_MAX_W, two streams above", tg_single_max,
         [("TGLS_WIDTHS", regimes.TGLS_WIDTHS), ("TGLS_BITS_WIDTHS", regimes.TGLS_BITS_WIDTHS)]),
        ("unweighted coverage bits up to COVF_MAX_W, scores + counts above", k["COVF_MAX_W"],
         [("UNWEIGHTED_BITS_WIDTHS", regimes.UNWEIGHTED_BITS_WIDTHS)]),
        ("GL wLOD strip kernel: WS_WAVES compute waves up to here, WS_WAVES_WIDE above", strip_max(k["WS_WAVES"]),
         [("WEIGHTED_WIDTHS", regimes.WEIGHTED_WIDTHS)]),
        ("GL wLOD strip kernel (WS_WAVES_WIDE) up to here, the GL ring tile kernel above", strip_max(k["WS_WAVES_WIDE"]),
         [("WEIGHTED_WIDTHS", regimes.WEIGHTED_WIDTHS)]),
    ]


def test_every_switch_is_tested_on_both_sides():
    missing = []
    for name, b, lists in boundaries(constants()):
        for lname, widths in lists:
            for w in (b, b + 1):
                if w not in widths:
                    missing.append(f"{name} (W = {b} | {b + 1}): {lname} lacks W = {w}")
    assert not missing, "\n".join(missing)


def test_the_tested_widths_reach_the_forms_they_are_meant_for():
    k = constants()
    tg_single_max = k["GARLIC_TG_RING"] - 32 - 4 * k["TG_GROUP"] * 2
    # the two-stream TGLS form is tested well past the switch, where its halves wrap many times
    assert max(regimes.TGLS_WIDTHS) > 4 * tg_single_max and max(regimes.TGLS_BITS_WIDTHS) > 2 * tg_single_max
    # the tuned wLOD kernels take WLOD_R <= W <= GPAD_BACK - 64: every weighted width is theirs, and one lies past both
    # strip forms (the GL ring tile kernel)
    assert all(k["WLOD_R"] <= W <= k["GPAD_BACK"] - 64 for W in regimes.WEIGHTED_WIDTHS)
    assert max(regimes.WEIGHTED_WIDTHS) > 16 * k["WS_WAVES_WIDE"] + 1 + 64
    # the chains' rolling sums with non-finite terms: a width under one tile, one of a few tiles, one of many
    assert min(regimes.NONFINITE_WIDTHS) < 32 < max(regimes.NONFINITE_WIDTHS) and max(regimes.NONFINITE_WIDTHS) > 256


def test_the_switches_are_where_the_gpu_file_says():
    """the values its docstring names (a retune updates both)"""
    k = constants()
    assert [b for _, b, _ in boundaries(k)] == [144, 1024, 113, 241]
    assert k["GPAD_BACK"] - 64 == 4096
