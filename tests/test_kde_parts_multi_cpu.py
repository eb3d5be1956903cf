"""CPU: the KDEs of several split feeds at once (garlic_kde_parts_multi) -- what is declared, and the descent for F feeds
(kdeSelectRanksMulti of garlic_amd/host/kde_parts.hpp) in a stand-alone program under the sanitizers: per feed exactly the
values of the single-feed kdeSelectRanks and of the sorted union, 8 rank queries in all whatever F is, feeds that are
switched off change nothing.  The plan of a part set counts a part of one value as a chunk."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import kde_cases as cases
import kde_parts_multi_cases as mcases
from garlic_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["garlic_kde_part_set_create", "garlic_lod_kde_part_set", "garlic_kde_part_set_destroy", "garlic_kde_part_set_counts",
         "garlic_kde_part_set_moment", "garlic_kde_part_set_rank", "garlic_kde_part_set_sums", "garlic_kde_parts_multi",
         "garlic_kde_parts_multi_info"]


def test_header_bindings_and_library_declare_the_part_set_calls():
    hdr = open(os.path.join(ROOT, "include", "garlic_hip.h")).read()
    assert re.search(r"^typedef struct garlic_kde_part_set garlic_kde_part_set;$", hdr, re.M)
    version = int(re.search(r"^#define GARLIC_HIP_ABI_VERSION (\d+)$", hdr, re.M).group(1))
    history = re.search(r"^ \* %d:.*?\*/" % version, hdr, re.M | re.S).group(0)
    lib = C.CDLL(abi.LIB_PATH)
    for name in NAMES:
        assert re.search(r"^int %s\(" % name, hdr, re.M), name
        assert re.search(r"\b%s\b" % name, history), (name, "is not in the history of the ABI version")
        assert name in abi.SYMBOLS and hasattr(lib, name), name
    assert "garlic_kde_part_set," in history
    assert abi.lib().garlic_hip_abi_version() == abi.ABI_VERSION == version
    assert C.sizeof(abi.Kde) == 8 * (7 + 3 * 512), "garlic_kde is unchanged"
    for cls, attrs in ((abi.KdePartSet, ("counts", "moment", "rank", "sums", "close", "__enter__", "__exit__")),
                       (abi.Context, ("kde_part_set",)), (abi.Panel, ("lod_kde_part_set",))):
        for a in attrs:
            assert callable(getattr(cls, a)), (cls, a)
    assert callable(abi.kde_parts_multi) and callable(abi.kde_parts_multi_info)


def test_sharded_callers_are_there():
    from garlic_amd import shard
    import inspect
    assert callable(shard.lod_kde_multi)
    assert inspect.signature(shard.lod_kde).parameters["on_shards"].default is False


@pytest.fixture(scope="module")
def unit_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("kde_parts_multi_unit") / "kde_parts_multi_unit")
    src = os.path.join(ROOT, "tests", "host_unit", "kde_parts_multi_unit.cpp")
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", exe, src], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    return exe


def write_batch(path, feeds):
    """feeds: [(label, parts)]; a feed whose union holds fewer than 2 values is written as switched off"""
    with open(path, "wb") as f:
        f.write(np.int64(len(feeds)).tobytes())
        for _, parts in feeds:
            total = sum(p.shape[0] for p in parts)
            f.write(np.int64(1 if total >= 2 else 0).tobytes())
            f.write(np.int64(len(parts)).tobytes())
            for p in parts:
                f.write(np.int64(p.shape[0]).tobytes())
                f.write(np.ascontiguousarray(p, dtype=np.float64).tobytes())


def test_descent_for_f_feeds_is_the_single_feed_descent(unit_exe, tmp_path):
    batches = [mcases.batch(1, 1), mcases.batch(1, 3, shift=2), mcases.batch(2, 2), mcases.batch(2, 8, shift=1),
               mcases.batch(32, 2), mcases.batch(32, 3, shift=3), mcases.small_mixed(), mcases.tied(),
               mcases.small_mixed() + mcases.tied() + mcases.batch(4, 2, shift=4)]
    assert {len(b) for b in batches} >= {1, 2, 32}
    assert [sum(p.shape[0] for p in parts) for _, parts in mcases.small_mixed()] == [0, 1, 2, 3, 65]
    paths = []
    for i, feeds in enumerate(batches):
        paths.append(str(tmp_path / ("batch%02d.bin" % i)))
        write_batch(paths[-1], feeds)
    run = subprocess.run([unit_exe] + paths, capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert run.stdout == "".join("feeds %d rounds 8\n" % len(b) for b in batches) + "kde_parts_multi_unit ok\n"


def test_a_part_of_one_value_is_a_chunk_of_a_set_but_not_of_a_whole_feed(tmp_path):
    """host/kde_multi_plan.hpp: kdePartSetPlan against kdeMultiPlan on the same lengths"""
    src = tmp_path / "plan.cpp"
    src.write_text('#include "%s"\n#include <cstdio>\nint main() {\n'
                   '  const int64_t n[5] = {0, 1, 2, %d, %d};\n  garlic_host::KdeMultiPlan a, b;\n'
                   '  if (!garlic_host::kdeMultiPlan(n, 5, &a) || !garlic_host::kdePartSetPlan(n, 5, &b)) return 1;\n'
                   '  for (int f = 0; f < 5; f++) printf("%%lld %%lld %%lld %%lld\\n", (long long)a.feed[f].n_chunks, (long long)b.feed[f].n_chunks,\n'
                   '                                     (long long)a.chunk_first.at[f], (long long)b.chunk_first.at[f]);\n'
                   '  printf("%%lld %%lld %%lld %%lld\\n", (long long)a.total_chunks, (long long)b.total_chunks, (long long)a.total_slices, (long long)b.total_slices);\n'
                   '  return 0;\n}\n' % (os.path.join(ROOT, "garlic_amd", "host", "kde_multi_plan.hpp"), cases.kde_chunk(), cases.kde_chunk() + 1))
    exe = str(tmp_path / "plan")
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, str(src)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    rows = [[int(v) for v in line.split()] for line in run.stdout.splitlines()]
    assert [r[0] for r in rows[:5]] == [0, 0, 1, 1, 2] and [r[1] for r in rows[:5]] == [0, 1, 1, 1, 2]
    assert [r[2] for r in rows[:5]] == [0, 0, 0, 1, 2] and [r[3] for r in rows[:5]] == [0, 0, 1, 2, 3]
    assert rows[5] == [4, 5, 4, 5]
