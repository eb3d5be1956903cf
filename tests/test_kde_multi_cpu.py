"""CPU: the KDE of several feeds in one call (garlic_feed_kde_multi, garlic_lod_kde_multi) -- what is declared, and the plan
of garlic_amd/host/kde_multi_plan.hpp (which workgroup of a batched launch works on which feed's chunk or slice, and where
the feeds' partials lie) in a stand-alone program under the sanitizers: every (feed, chunk) and (feed, slice) is covered
exactly once, no two feeds overlap, and every feed's partition is the single-feed call's."""
import ctypes as C
import os
import re
import subprocess

import pytest

import kde_cases as cases
from garlic_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["garlic_feed_kde_multi", "garlic_lod_kde_multi", "garlic_feed_kde_multi_info"]
MAX_SLICES = 2048


def test_header_bindings_and_library_declare_the_multi_calls():
    hdr = open(os.path.join(ROOT, "include", "garlic_hip.h")).read()
    assert re.search(r"^#define GARLIC_HIP_ABI_VERSION 8$", hdr, re.M)
    assert re.search(r"^#define GARLIC_KDE_MAX_FEEDS 32$", hdr, re.M)
    history = re.search(r"^ \* 8:.*?\*/", hdr, re.M | re.S).group(0)
    lib = C.CDLL(abi.LIB_PATH)
    for name in NAMES:
        assert re.search(r"^int %s\(" % name, hdr, re.M), name
        assert re.search(r"\b%s\b" % name, history), (name, "is not in the history of ABI 8")
        assert name in abi.SYMBOLS and hasattr(lib, name), name
    assert "GARLIC_KDE_MAX_FEEDS" in history
    assert "no KDE twin" not in hdr
    assert abi.lib().garlic_hip_abi_version() == abi.ABI_VERSION == 8
    assert abi.KDE_MAX_FEEDS == 32
    assert C.sizeof(abi.Kde) == 8 * (7 + 3 * 512), "garlic_kde is unchanged"
    for cls, attrs in ((abi.Context, ("feed_kde_multi", "feed_kde_multi_info")), (abi.Panel, ("lod_kde_multi",))):
        for a in attrs:
            assert callable(getattr(cls, a)), (cls, a)
    plan = open(os.path.join(ROOT, "garlic_amd", "host", "kde_multi_plan.hpp")).read()
    kernels = open(os.path.join(ROOT, "garlic_amd", "csrc", "kde_kernels.hpp")).read()
    assert int(re.search(r"KDE_MULTI_CHUNK = (\d+);", plan).group(1)) == cases.kde_chunk()
    assert int(re.search(r"KDE_MULTI_MAX_SLICES = (\d+);", plan).group(1)) == MAX_SLICES == \
        int(re.search(r"KDE_MAX_SLICES = (\d+);", kernels).group(1))
    assert int(re.search(r"KDE_MULTI_MAX_FEEDS = (\d+);", plan).group(1)) == 32


def test_the_multi_kernels_run_the_single_feed_bodies():
    """the batched kernels hold no arithmetic of their own: each calls the __device__ body its single-feed twin calls"""
    multi = open(os.path.join(ROOT, "garlic_amd", "csrc", "kde_multi_kernels.hpp")).read()
    single = open(os.path.join(ROOT, "garlic_amd", "csrc", "kde_kernels.hpp")).read()
    code = re.sub(r"//.*", "", multi)
    for body in ("kde_moment_chunk", "kde_tree_feed", "kde_sum_slice", "kde_slice_total"):
        assert len(re.findall(r"\b%s\(" % body, code)) == 1, body
        assert len(re.findall(r"\b%s\(" % body, re.sub(r"//.*", "", single))) >= 2, (body, "defined and called in kde_kernels.hpp")
    assert "exp(" not in code and "atomicAdd" not in code and "__shared__" not in code


@pytest.fixture(scope="module")
def unit_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("kde_multi_unit") / "kde_multi_plan_unit")
    src = os.path.join(ROOT, "tests", "host_unit", "kde_multi_plan_unit.cpp")
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                         "-fno-omit-frame-pointer", "-o", exe, src], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    return exe


def expected(ns):
    """the single-feed call's partition of every feed, and the running offsets"""
    c = cases.kde_chunk()
    rows, chunk_off, slice_off = [], 0, 0
    for n in ns:
        n = n if n >= 2 else 0
        chunks = -(-n // c)
        cps = -(-chunks // MAX_SLICES)
        slices = -(-chunks // cps) if cps else 0
        rows.append((n, chunks, cps, slices, chunk_off, slice_off))
        chunk_off += chunks
        slice_off += slices
    return rows, chunk_off, slice_off


def lists():
    c = cases.kde_chunk()
    sizes = [2, 3, 64, 65, c - 1, c, c + 1, 3 * c + 17, cases.BIG]
    over = (MAX_SLICES + 1) * c + 5                    # more chunks than KDE_MAX_SLICES: two per slice
    assert -(-over // c) > MAX_SLICES
    return [sizes, sizes[::-1], [cases.HUGE, 65], [7], [c], list(range(2, 34)), [cases.BIG] * 32,
            [c + 1, 0, 3 * c + 17], [0, 1, 65, 0, c, 1], [0], [1, 0], [over], [over, 2, over + c, 0, cases.HUGE],
            [2 * MAX_SLICES * c, 2 * MAX_SLICES * c + 1]]


def test_plan_covers_every_chunk_and_slice_once(unit_exe):
    todo = lists()
    text = "".join(" ".join(str(n) for n in ns) + "\n" for ns in todo)
    run = subprocess.run([unit_exe], input=text, capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.endswith("kde_multi_plan_unit ok\n"), (run.stdout[-2000:] + run.stderr[-3000:])
    lines = run.stdout.splitlines()
    at = 0
    for ns in todo:
        rows, chunks, slices = expected(ns)
        assert lines[at] == "feeds %d chunks %d slices %d" % (len(ns), chunks, slices), (ns, lines[at])
        for f, row in enumerate(rows):
            assert lines[at + 1 + f] == " ".join(str(v) for v in row), (ns, f, lines[at + 1 + f])
        at += 1 + len(ns)
    assert at == len(lines) - 1


def test_plan_refuses_what_no_launch_holds(unit_exe):
    c = cases.kde_chunk()
    too_many = " ".join(["1"] * 33)
    too_long = "%d %d" % ((2 ** 31 - 1) * c, 2)           # 2^31 - 1 chunks and one more
    run = subprocess.run([unit_exe], input="\n%s\n%s\n" % (too_many, too_long), capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-3000:]
    assert run.stdout == "refused\n" * 3 + "kde_multi_plan_unit ok\n"
