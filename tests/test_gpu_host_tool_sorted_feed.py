"""GPU: garlic-lod --sorted-feed end to end on the tiny data set of tests/golden/e2e: <out>.<W>SNPs.lod.sorted.f64 holds
np.sort of what the plain run writes into <out>.<W>SNPs.lod.f64 (LodOptions::feed_sorted -> garlic_panel_set_feed_order on
every shard, the shards' arrays merged on the host), bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as ol

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E2E = os.path.join(ROOT, "tests", "golden", "e2e")
TOOL = os.path.join(ROOT, "garlic_amd", "host", "garlic-lod")
TGLS = ["--tgls", os.path.join(E2E, "tiny.tgls.gz"), "--gl-type", "GQ"]


def run_tool(d, *extra, stdin=None):
    """--kde-subsample 0: everyone feeds the KDE (the default draw is time-seeded)"""
    os.makedirs(d, exist_ok=True)
    out = os.path.join(str(d), "mine")
    cmd = [TOOL, "--tped", os.path.join(E2E, "tiny.tped.gz"), "--tfam", os.path.join(E2E, "tiny.tfam"),
           "--centromere", os.path.join(E2E, "tiny.centromeres.txt"), "--out", out, "--kde-subsample", "0"]
    if "--tgls" not in extra:
        cmd += ["--error", "0.001"]
    r = subprocess.run(cmd + list(extra), capture_output=True, text=True, input=stdin)
    assert r.returncode == 0, r.stderr[-2000:]
    return out, r.stdout


def feed(out, W, sorted_feed):
    path = "%s.%dSNPs.lod.%sf64" % (out, W, "sorted." if sorted_feed else "")
    other = "%s.%dSNPs.lod.%sf64" % (out, W, "" if sorted_feed else "sorted.")
    assert os.path.exists(path) and not os.path.exists(other), (path, os.listdir(os.path.dirname(out)))
    return np.fromfile(path, dtype=np.float64)


def check(plain, got, what):
    assert plain.shape[0] > 0 and not np.isnan(plain).any() and not (np.signbit(plain) & (plain == 0)).any(), what
    assert ol.bits_equal(got, np.sort(plain)), what


def test_single_size(tmp_path):
    plain, _ = run_tool(tmp_path / "a", "--winsize", "30")
    want = feed(plain, 30, False)
    one, _ = run_tool(tmp_path / "b", "--winsize", "30", "--sorted-feed")
    check(want, feed(one, 30, True), "one shard")
    two, _ = run_tool(tmp_path / "c", "--winsize", "30", "--sorted-feed", "--devices", "0,0")      # two shards: the merge
    assert ol.bits_equal(feed(two, 30, True), feed(one, 30, True))
    raw, _ = run_tool(tmp_path / "d", "--winsize", "30", "--sorted-feed", "--raw-lod")              # host scores, std::sort
    assert ol.bits_equal(feed(raw, 30, True), feed(one, 30, True))


def test_winsize_multi_with_likelihoods(tmp_path):
    sizes = [20, 45, 33]
    plain, _ = run_tool(tmp_path / "a", "--winsize-multi", *map(str, sizes), *TGLS)
    one, _ = run_tool(tmp_path / "b", "--winsize-multi", *map(str, sizes), *TGLS, "--sorted-feed")
    two, _ = run_tool(tmp_path / "c", "--winsize-multi", *map(str, sizes), *TGLS, "--sorted-feed", "--devices", "0,0")
    for W in sizes:
        check(feed(plain, W, False), feed(one, W, True), ("tgls multi", W))
        assert ol.bits_equal(feed(two, W, True), feed(one, W, True)), W


def test_winsize_stream_names_the_sorted_file(tmp_path):
    plain, _ = run_tool(tmp_path / "a", "--winsize", "40")
    out, stdout = run_tool(tmp_path / "b", "--winsize", "30", "--winsize-stream", "--sorted-feed", stdin="40\n0\n")
    lines = [l.split() for l in stdout.splitlines() if l.startswith("FEED ")]
    assert len(lines) == 1 and lines[0][1] == "40" and lines[0][2] == out + ".40SNPs.lod.sorted.f64", stdout
    got = feed(out, 40, True)
    assert int(lines[0][3]) == got.shape[0]
    check(feed(plain, 40, False), got, "stream")


def test_usage_lists_the_flag():
    r = subprocess.run([TOOL], capture_output=True, text=True)
    assert r.returncode != 0 and "--sorted-feed" in r.stderr
