"""CPU: what the sorted KDE feed rests on, with numpy and the oracle alone (tests/test_gpu_feed_sort.py runs the same key
sets and panel cases on the GPU).

  * the key transform of include/garlic_hip.h: sorting by the transformed uint64 is np.sort of the values, bit for bit,
    wherever "ascending" is unique (no NaN, no mix of -0.0 and +0.0), and puts -0.0 in front of +0.0 where both occur
  * every panel case's ORACLE feed holds no NaN, no -0.0 and is not empty: the condition under which the ascending
    arrangement is unique -- on the reference alone, not on the code under test
  * the shard-merge helper of garlic_amd/shard.py against np.sort of the concatenation
  * the host's k-way merge (garlic_amd/host/feed_merge.hpp) in a stand-alone program under ASan + UBSan"""
import os
import subprocess

import numpy as np
import pytest

import feed_sort_cases as cases
import oracle_lib as ol
from garlic_amd import shard

ROOT = cases.ROOT


def test_tile_constant_is_read_from_the_kernel_source():
    t = cases.fs_tile()
    assert 1024 <= t <= 16384 and t % 256 == 0


@pytest.mark.parametrize("name", [c for c in cases.CONTENTS if c != "mixed"])
@pytest.mark.parametrize("n", [0, 1, 2, 65, 4097, 50001])
def test_key_order_is_numeric_order(name, n):
    x = cases.content(name, n)
    assert not np.isnan(x).any() and not (np.signbit(x) & (x == 0)).any()
    assert ol.bits_equal(cases.sorted_by_key(x), np.sort(x))
    assert ol.bits_equal(cases.unkey(cases.key(x)), x)
    assert ol.bits_equal(shard.feed_sort_key(x).view(np.float64), cases.key(x).view(np.float64))


def test_key_order_with_infinities_denormals_and_zeros():
    x = cases.content("mixed", 20001)
    got = cases.sorted_by_key(x)
    assert np.array_equal(got, np.sort(x))                    # numerically the same arrangement (-0.0 == +0.0) ...
    zeros = got[got == 0]
    nneg = int(np.signbit(zeros).sum())
    assert 0 < nneg < len(zeros)
    assert np.signbit(zeros[:nneg]).all() and not np.signbit(zeros[nneg:]).any()      # ... with -0.0 in front of +0.0
    assert got[0] == -np.inf and got[-1] == np.inf
    # without the zeros of either sign the arrangement is unique: bit for bit np.sort
    y = x[x != 0]
    assert ol.bits_equal(cases.sorted_by_key(y), np.sort(y))


@pytest.mark.parametrize("byte", range(8))
def test_one_byte_keys_differ_in_that_byte_only(byte):
    k = cases.key(cases.one_byte_keys(byte, 1000))
    diff = np.bitwise_or.reduce(k ^ k[0])
    assert diff != 0 and diff & ~(np.uint64(0xFF) << np.uint64(8 * byte)) == 0


@pytest.mark.parametrize("call,nind,subset", cases.panel_cases())
def test_oracle_feeds_are_uniquely_sortable(call, nind, subset):
    for per_chr in cases.oracle_feeds(call, nind, subset):
        feed = np.concatenate(per_chr)
        assert feed.shape[0] > 0, "empty case"
        assert not np.isnan(feed).any()
        assert not (np.signbit(feed) & (feed == 0)).any(), "-0.0 in a feed"
        assert ol.bits_equal(cases.sorted_by_key(feed), np.sort(feed))


def test_shard_merge_helper():
    for feeds in cases.shard_merge_cases():
        want = np.sort(np.concatenate(feeds)) if feeds else np.empty(0)
        got = shard.merge_sorted_feeds(feeds)
        assert got.dtype == np.float64 and got.shape == want.shape
        assert ol.bits_equal(got, want)
    # -0.0 / +0.0 across shards: the key order decides
    a, b = np.array([-1.0, 0.0, 2.0]), np.array([-0.0, 0.0, 3.0])
    got = shard.merge_sorted_feeds([a, b])
    assert ol.bits_equal(got, cases.sorted_by_key(np.concatenate([a, b])))


def test_host_merge_unit_program(tmp_path):
    """tests/host_unit/feed_merge_unit.cpp, compiled here with ASan + UBSan: a stand-alone program, nothing loaded into python"""
    exe = str(tmp_path / "feed_merge_unit")
    src = os.path.join(ROOT, "tests", "host_unit", "feed_merge_unit.cpp")
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                         "-fno-omit-frame-pointer", "-o", exe, src], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "feed_merge_unit ok" in r.stdout, (r.stdout + r.stderr)[-3000:]


def test_header_and_bindings_declare_the_feature():
    from garlic_amd import abi
    header = open(os.path.join(ROOT, "include", "garlic_hip.h")).read()
    for name in ("garlic_panel_set_feed_order", "garlic_feed_sort", "garlic_feed_sort_info"):
        assert name in header and name in abi.SYMBOLS
    assert (abi.FEED_ORDER_REFERENCE, abi.FEED_ORDER_SORTED) == (0, 1)
    assert "garlic-kde.cpp:132" in header
