"""No GPU: the numpy reference of the device KDE (tests/kde_cases.py) against brute force, the host arithmetic of
garlic_amd/host/kde_select.hpp (a stand-alone program under ASan + UBSan) against that reference, the cutoff selection
against the reference's own example output, and the declarations."""
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

import kde_cases as cases
import oracle_lib as ol

ROOT = cases.ROOT
FIXTURE = os.path.join(ROOT, "tests", "golden", "kde", "example.60SNPs.kde")
EXPECTED = json.load(open(os.path.join(ROOT, "tests", "golden", "kde", "example.expected.json")))


def test_contents_are_what_their_names_say():
    for name in cases.CONTENTS:
        for n in cases.sizes():
            x = cases.content(name, n)
            assert x.shape == (n,) and np.isfinite(x).all() and (np.diff(x) >= 0).all()
            r = cases.reference_of(name, n, False)
            assert r["h"] > 0 and math.isfinite(r["h"]), (name, n)
            assert abs(float(x.mean())) <= 1.0e3 * float(r["sd"]), (name, n)       # the h tolerance of the GPU test needs it
            span = (x[-1] - x[0]) / r["h"]
            if name == "wide" and n >= 63:
                assert span >= 1e4, (n, span)
            if name == "narrow":
                assert (span + cases.CUT) ** 2 < 746, (n, span)   # the farthest pair: a target 3 h outside one end, a source at the other
            if name == "shifted":
                assert abs(float(x.mean())) >= 0.9e3 * float(r["sd"])


def test_reference_against_fsum_brute_force():
    """n <= 200: every sum again with math.fsum (exactly rounded sums of float64 terms)"""
    for name in cases.CONTENTS:
        for n in (2, 3, 65, 200):
            x = cases.content(name, n) if n != 200 else np.sort(cases.content(name, 2049)[::10][:200])
            r = cases.reference(x)
            mean = math.fsum(x) / n
            sd = math.sqrt(math.fsum((v - mean) ** 2 for v in x) / (n - 1))
            assert abs(sd - float(r["sd"])) <= 1e-13 * sd, (name, n)
            h, t = r["h"], r["x"]
            for j in range(0, cases.POINTS, 37):
                want = math.fsum(math.exp(-((v - t[j]) ** 2) / (h * h)) for v in x) / n
                # float64 arguments of up to 746 carry a few roundings each: 1e-12 relative, as on the GPU
                assert abs(float(r["raw"][j]) - want) <= 1e-12 * want + 1e-300, (name, n, j)
            s = sum(float(v) for v in r["raw"].astype(np.float64))
            assert np.allclose(r["y"].sum() * (t[1] - t[0]), 1.0, rtol=1e-12) and s > 0


def test_quantile_is_numpys_linear_method():
    """gsl_stats_quantile_from_sorted_data is numpy's default: the same point between the same neighbours a = x[k],
    b = x[k + 1].  numpy forms a + (b - a) t (or b - (b - a)(1 - t)) where this forms (1 - t) a + t b: each carries at
    most three roundings of quantities no larger than max(|a|, |b|), hence 4 ulp of the larger neighbour"""
    for name in cases.CONTENTS:
        for n in cases.sizes()[:-1] + [1001]:
            x = cases.content(name, n) if n != 1001 else cases.content(name, cases.BIG)[::99][:1001]
            for f in (0.25, 0.75, 0.0, 1.0, 0.5):
                got, want = cases.quantile(x, f), float(np.quantile(x, f, method="linear"))
                k = min(int(f * float(x.shape[0] - 1)), x.shape[0] - 2)
                unit = np.spacing(max(abs(x[k]), abs(x[k + 1])))
                assert abs(got - want) <= 4 * unit, (name, n, f, got, want)


def test_cutoff_of_the_reference_example():
    """tests/golden/kde/example.60SNPs.kde is the reference's example output; its log says "Selected LOD score cutoff: 1.26224\""""
    x, y = cases.read_kde(FIXTURE)
    assert x.shape == (512,)
    cutoff, at, modes, counts = cases.min_between_modes(x, y, EXPECTED["winsize"])
    assert at == EXPECTED["min_index"] == 421 and modes == (258, 447) and counts == (20, 20)
    assert cutoff == x[421] and "%g" % cutoff == EXPECTED["cutoff_printed"]
    assert EXPECTED["log_line"].endswith(EXPECTED["cutoff_printed"])
    assert cases.min_between_modes(x, y, 1)[0] == 0.0                               # |x / wsize| >= 1


@pytest.fixture(scope="module")
def unit_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("kde_unit") / "kde_select_unit")
    src = os.path.join(ROOT, "tests", "host_unit", "kde_select_unit.cpp")
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", exe, src], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    return exe


@pytest.mark.parametrize("name,n", [("bimodal", 6161), ("shifted", 65), ("two_values", 2), ("wide", 2049), ("narrow", 3)])
def test_host_header_unit_program(unit_exe, tmp_path, name, n):
    """kde_select.hpp on vectors written here: quantiles, bandwidth, targets and normalisation bit for bit with the numpy
    reference; the wiggle against np.polyfit's residuals at relative 1e-9 (condition of the fit on 20 equally spaced
    abscissae <= 1e4, times 2^-53, with margin); the fixture's index and printed cutoff; the .kde writer"""
    x = cases.content(name, n)
    r = cases.reference(x)
    raw = r["raw"].astype(np.float64)
    x.tofile(tmp_path / "feed.f64")
    np.array([float(r["sd"])]).tofile(tmp_path / "sd.f64")
    raw.tofile(tmp_path / "raw.f64")
    run = subprocess.run([unit_exe, FIXTURE, str(EXPECTED["winsize"]), str(tmp_path)], capture_output=True, text=True)
    assert run.returncode == 0 and "kde_select_unit ok" in run.stdout, (run.stdout + run.stderr)[-3000:]
    assert "cutoff %s\n" % EXPECTED["cutoff_printed"] in run.stdout
    out = np.fromfile(tmp_path / "out.f64")
    assert out.shape == (3 + 2 * 512 + 1 + 3,)
    q25, q75, h, t, y, wig = out[0], out[1], out[2], out[3:515], out[515:1027], out[1027]
    at, cutoff, fwig = out[1028:]
    assert ol.bits_equal(np.array([q25, q75, h]), np.array([r["q25"], r["q75"], r["h"]]))
    assert ol.bits_equal(t, r["x"]) and ol.bits_equal(y, cases.normalise(raw, r["x"]))
    want = cases.wiggle(t, y)
    assert want > 0 and abs(wig - want) <= 1e-9 * want, (wig, want)
    fx, fy = cases.read_kde(FIXTURE)
    assert int(at) == 421 and cutoff == fx[421]
    fwant = cases.wiggle(fx, fy)
    assert fwant > 0 and abs(fwig - fwant) <= 1e-9 * fwant, (fwig, fwant)
    assert open(tmp_path / "out.kde").read() == cases.kde_lines(t, y)
    assert open(tmp_path / "out100.kde").read() == cases.kde_lines(t, y, 100.0)


def test_header_and_bindings_declare_the_kde_calls():
    hdr = open(os.path.join(ROOT, "include", "garlic_hip.h")).read()
    assert re.search(r"^#define GARLIC_HIP_ABI_VERSION 8$", hdr, re.M)
    assert re.search(r"^#define GARLIC_KDE_POINTS 512$", hdr, re.M)
    for name in ("garlic_feed_kde", "garlic_lod_kde", "garlic_feed_kde_info"):
        assert re.search(r"^int %s\(" % name, hdr, re.M), name
    assert "typedef struct garlic_kde {" in hdr
    abi_src = open(os.path.join(ROOT, "garlic_amd", "abi.py")).read()
    listed = re.search(r"^SYMBOLS = \[(.*?)^\]", abi_src, re.M | re.S).group(1)
    for name in ("garlic_feed_kde", "garlic_lod_kde", "garlic_feed_kde_info"):
        assert '"%s"' % name in listed, name
    from garlic_amd import abi
    assert abi.ABI_VERSION == 8
    import ctypes as C
    assert C.sizeof(abi.Kde) == 8 * 7 + 3 * 512 * 8
