"""No GPU: the declarations of the GMM calls; the numpy reference of the EM fit (tests/gmm_cases.py) against what the
reference binary printed for the 113 golden lengths (tests/golden/e2e/refs3.*, refs2.*: its stop iteration, its Gaussians,
its boundaries); the host arithmetic of garlic_amd/host/size_classes.hpp (a stand-alone program under ASan + UBSan) against
that golden and the reference of this suite; and the condition the GPU test's stop cases rest on: the float64 and the
long-double reference stop at the same iteration."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import gmm_cases as cases

ROOT = cases.ROOT
E2E = os.path.join(ROOT, "tests", "golden", "e2e")
GOLDEN_STOP = {"refs3": 289, "refs2": 265}        # the last "iteration: N" the binary prints (COMMAND_gmm.txt)


golden_log, printed_alike = cases.golden_log, cases.printed_alike


def test_header_and_bindings_declare_the_gmm_calls():
    hdr = open(os.path.join(ROOT, "include", "garlic_hip.h")).read()
    assert re.search(r"^#define GARLIC_HIP_ABI_VERSION 8$", hdr, re.M)
    assert re.search(r"^#define GARLIC_GMM_MAX_K 8$", hdr, re.M)
    for name in ("garlic_gmm_fit", "garlic_gmm_fit_info"):
        assert re.search(r"^int %s\(" % name, hdr, re.M), name
    assert "typedef struct garlic_gmm {" in hdr
    abi_src = open(os.path.join(ROOT, "garlic_amd", "abi.py")).read()
    listed = re.search(r"^SYMBOLS = \[(.*?)^\]", abi_src, re.M | re.S).group(1)
    for name in ("garlic_gmm_fit", "garlic_gmm_fit_info"):
        assert '"%s"' % name in listed, name
    import ctypes as C
    from garlic_amd import abi
    assert abi.ABI_VERSION == 8 and abi.GMM_MAX_K == cases.MAX_K == 8
    assert C.sizeof(abi.Gmm) == 16 + 3 * 8 * 8 + 16
    lib = C.CDLL(abi.LIB_PATH)
    for name in ("garlic_gmm_fit", "garlic_gmm_fit_info"):
        assert hasattr(lib, name), name
    assert abi.lib().garlic_hip_abi_version() == 8
    assert hasattr(abi.Context, "gmm_fit") and hasattr(abi.Context, "gmm_fit_info")
    assert cases.block_points() % 256 == 0


@pytest.mark.parametrize("tag,k", [("refs3", 3), ("refs2", 2)])
def test_reference_reproduces_the_binary(tag, k):
    """the float64 reference on the golden's lengths: the binary's stop iteration, its Gaussians to the printed digits, and
    boundaries within 2e-4 relative of the printed ones (both solvers end inside a bracket of relative width 1e-4 around the
    same root)"""
    x = cases.golden_lengths(tag)
    assert x.shape == (113,)
    f64, ld = cases.stop_reference(tag, 113, k)
    assert f64["iterations"] == GOLDEN_STOP[tag] and f64["converged"] == 1
    gauss, bounds = golden_log(tag)
    mine = cases.class_lines(f64["a"], f64["mean"], f64["var"])
    for line, want in zip(mine, gauss):
        got = re.search(r"= \( (\S+), (\S+), (\S+) \)", line).groups()
        assert all(printed_alike(g, w) for g, w in zip(got, want)), (line, want)
    order, b = cases.boundaries(f64["a"], f64["mean"], f64["var"])
    assert len(b) == len(bounds) == k - 1
    for g, w in zip(b, bounds):
        assert abs(g - float(w)) <= 2e-4 * float(w), (g, w)
    # the golden's classes: every length below the first boundary it stays under
    letters = [l.split("\t")[3] for l in _bed_lines(tag)]
    assert letters == [chr(65 + sum(v >= t for t in b)) for v in x]


def _bed_lines(tag):
    import gzip
    with gzip.open(os.path.join(E2E, tag + ".roh.bed.gz"), "rt") as f:
        return [l for l in f if not l.startswith("track")]


def test_stop_cases_stop_alike_in_both_precisions():
    """asserted, not assumed: tests/test_gpu_gmm.py compares the device's stop iteration with this one"""
    cases.warm(cases.stop_cases(), cases.stop_reference)
    for case in cases.stop_cases():
        f64, ld = cases.stop_reference(*case)
        assert f64["iterations"] == ld["iterations"] and f64["converged"] == ld["converged"] == 1, case
        assert 1 < f64["iterations"] < cases.MAX_ITER, case
        noise = cases.noise(f64, ld)
        assert noise is not None and noise < 1e-9, (case, noise)
        # not marginal: the step that stopped the fit is under the precision by a margin, the one before over it
        x = cases.data_of(case[0], case[1])
        a0, m0, v0 = cases.init(x, case[2], recurrence=case[0].startswith("refs"))
        _, kept = cases.fit(x, a0, m0, v0, f64["iterations"], -1.0, np.longdouble, keep=tuple(range(1, f64["iterations"] + 1)))
        L = [kept[i]["loglik"] for i in sorted(kept)]
        last, before = abs(L[-1] - L[-2]), abs(L[-2] - L[-3]) if len(L) > 2 else np.inf
        scale = abs(L[-1]) * max(noise, 2.0 ** -52) * 64
        assert last + scale <= cases.PRECISION and before - scale > cases.PRECISION, (case, float(last), float(before), float(scale))


def test_init_forms_agree():
    """the exactly rounded sums and gsl's long-double recurrences give the same initial guess to a few ulp"""
    for name, n, k in (("three", 65, 3), ("two", 2049, 2), ("one", 63, 5)):
        x = cases.content(name, n)
        p, q = cases.init(x, k), cases.init(x, k, recurrence=True)
        for u, v in zip(p, q):
            assert np.allclose(u, v, rtol=1e-14, atol=0), (name, n, k)
    a0, m0, v0 = cases.init(cases.content("three", 1), 3)
    assert np.isnan(v0).all() and np.isfinite(m0).all()


@pytest.fixture(scope="module")
def unit_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("size_unit") / "size_classes_unit")
    src = os.path.join(ROOT, "tests", "host_unit", "size_classes_unit.cpp")
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", exe, src], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    return exe


@pytest.mark.parametrize("tag,k", [("refs3", 3), ("refs2", 2)])
def test_host_header_unit_program(unit_exe, tmp_path, tag, k):
    """size_classes.hpp on the golden: the printed Gaussians (six digits), handed over in reverse order, come back ordered,
    with the binary's boundaries within 2e-4 relative and its log lines character for character; the initial guess bit for
    bit with the long-double recurrences written in gmm_cases"""
    x = cases.golden_lengths(tag)
    gauss, bounds = golden_log(tag)
    a, mean, var = (np.array([float(g[i]) for g in gauss])[::-1] for i in range(3))
    x.tofile(tmp_path / "lengths.f64")
    np.concatenate([[float(k)], a, mean, var]).tofile(tmp_path / "params.f64")
    run = subprocess.run([unit_exe, str(tmp_path)], capture_output=True, text=True)
    assert run.returncode == 0 and "size_classes_unit ok" in run.stdout, (run.stdout + run.stderr)[-3000:]
    out = np.fromfile(tmp_path / "out.f64")
    assert out.shape == (3 * k + k + k - 1,)
    want = np.concatenate(cases.init(x, k, recurrence=True))
    assert out[:3 * k].tobytes() == want.tobytes()
    assert out[3 * k:4 * k].tolist() == list(range(k))[::-1]
    for g, w in zip(out[4 * k:], bounds):
        assert abs(g - float(w)) <= 2e-4 * float(w), (g, w)
    _, mine = cases.boundaries(a, mean, var)
    for g, w in zip(out[4 * k:], mine):
        assert abs(g - w) <= 1e-4 * w, (g, w)              # the solver's own bracket around the root of the same function
    text = open(tmp_path / "out.txt").read().splitlines()
    golden = open(os.path.join(E2E, tag + ".log.txt")).read().splitlines()
    assert text[:-1] == golden[:-1]
    got_b = re.fullmatch(r"Selected ROH size boundaries = \( (.*) \)", text[-1]).group(1).split()
    assert len(got_b) == k - 1 and all(abs(float(g) - float(w)) <= 2e-4 * float(w) for g, w in zip(got_b, bounds))
