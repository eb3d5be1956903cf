"""CPU: the KDE of a feed split into sorted parts (garlic_kde_parts) -- what is declared, and the host arithmetic of
garlic_amd/host/kde_parts.hpp in a stand-alone program under the sanitizers: the radix descent with std::lower_bound as
the rank query gives the sorted union's four order statistics bit for bit in exactly 8 rounds, for every split of
tests/kde_parts_cases.py; the combination rules follow the stated association."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import kde_cases as cases
import kde_parts_cases as pcases
import oracle_lib as ol
from garlic_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["garlic_kde_part_create", "garlic_lod_kde_part", "garlic_kde_part_destroy", "garlic_kde_part_count",
         "garlic_kde_part_moment", "garlic_kde_part_rank", "garlic_kde_part_sums", "garlic_kde_parts", "garlic_kde_parts_info"]


def test_header_bindings_and_library_declare_the_part_calls():
    hdr = open(os.path.join(ROOT, "include", "garlic_hip.h")).read()
    assert re.search(r"^#define GARLIC_HIP_ABI_VERSION 8$", hdr, re.M)
    assert re.search(r"^#define GARLIC_KDE_MAX_PARTS 64$", hdr, re.M)
    assert re.search(r"^typedef struct garlic_kde_part garlic_kde_part;$", hdr, re.M)
    history = re.search(r"^ \* 8:.*?\*/", hdr, re.M | re.S).group(0)
    lib = C.CDLL(abi.LIB_PATH)
    for name in NAMES:
        assert re.search(r"^int %s\(" % name, hdr, re.M), name
        assert re.search(r"\b%s\b" % name, history), (name, "is not in the history of ABI 8")
        assert name in abi.SYMBOLS and hasattr(lib, name), name
    assert "GARLIC_KDE_MAX_PARTS" in history and "garlic_kde_part," in history
    assert abi.lib().garlic_hip_abi_version() == abi.ABI_VERSION == 8
    assert abi.KDE_MAX_PARTS == 64
    assert C.sizeof(abi.Kde) == 8 * (7 + 3 * 512), "garlic_kde is unchanged"
    for cls, attrs in ((abi.KdePart, ("count", "moment", "rank", "sums", "close", "__enter__", "__exit__")),
                       (abi.Context, ("kde_part",)), (abi.Panel, ("lod_kde_part",))):
        for a in attrs:
            assert callable(getattr(cls, a)), (cls, a)
    assert callable(abi.kde_parts) and callable(abi.kde_parts_info)


def test_the_key_is_garlic_feed_sorts_order():
    x = np.array([-np.inf, -3.5, -5e-324, -0.0, 0.0, 5e-324, 1.0, 2.25, np.inf])
    k = pcases.key(x)
    assert (np.diff(k.astype(object)) > 0).all()
    assert ol.bits_equal(pcases.key_value(k), x)


@pytest.fixture(scope="module")
def unit_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("kde_parts_unit") / "kde_parts_unit")
    src = os.path.join(ROOT, "tests", "host_unit", "kde_parts_unit.cpp")
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", exe, src], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    return exe


def write_case(d, parts, sums):
    os.makedirs(d)
    with open(os.path.join(d, "parts.bin"), "wb") as f:
        f.write(np.int64(len(parts)).tobytes())
        for p in parts:
            f.write(np.int64(p.shape[0]).tobytes())
            f.write(np.ascontiguousarray(p, dtype=np.float64).tobytes())
    sums.tofile(os.path.join(d, "sums.f64"))


def check_case(d, parts, union, sums, what):
    """union: the values in key order"""
    out = np.fromfile(os.path.join(d, "out.f64"))
    n = union.shape[0]
    assert out.shape == (4 + 1 + 8,), what
    assert ol.bits_equal(out[:4], union[pcases.order_ranks(n)]), (what, out[:4])
    total = 0.0
    for p in range(len(parts)):
        total = total + float(sums[p, 0])
    assert np.float64(out[4]).tobytes() == np.float64(total).tobytes(), (what, "kdeCombine")
    raw = []
    for j in range(8):
        t = 0.0
        for p in range(len(parts)):
            t = t + float(sums[p, j])
        raw.append(t / float(n))
    assert ol.bits_equal(out[5:], np.array(raw)), (what, "kdeCombineSums")
    # the descent restated in numpy (what the GPU test composes from the step calls) arrives at the same values
    keys = [pcases.key(p) for p in parts]
    got, rounds = pcases.descent(lambda probes: sum(np.searchsorted(k, probes, side="left") for k in keys), pcases.order_ranks(n))
    assert rounds == 8 and ol.bits_equal(got, out[:4]), what


@pytest.mark.parametrize("name", cases.CONTENTS + ["zeros"])
def test_descent_and_combination_rules_on_every_split(unit_exe, tmp_path, name):
    rng = np.random.default_rng(77)
    todo = []
    if name == "zeros":
        x, parts = pcases.zero_feed()
        todo.append(("zeros", parts, x))
        todo.append(("zeros one part", [x], x))
    else:
        for n in pcases.totals():
            for label, parts in pcases.splits(name, n):
                todo.append(("%s %d %s" % (name, n, label), parts, cases.content(name, n)))
    dirs, sums = [], []
    for i, (what, parts, union) in enumerate(todo):
        # sums of mixed magnitude and sign, so that another association would round differently
        s = rng.normal(0.0, 1.0, (len(parts), 8)) * 10.0 ** rng.integers(-8, 8, (len(parts), 8))
        dirs.append(str(tmp_path / ("case%03d" % i)))
        sums.append(s)
        write_case(dirs[-1], parts, s)
    run = subprocess.run([unit_exe] + dirs, capture_output=True, text=True)
    assert run.returncode == 0 and "kde_parts_unit ok" in run.stdout, (run.stdout + run.stderr)[-3000:]
    assert run.stdout == "rounds 8\n" * len(todo) + "kde_parts_unit ok\n"
    for d, s, (what, parts, union) in zip(dirs, sums, todo):
        check_case(d, parts, union, s, what)
