"""GPU: garlic-lod --kde --kde-sharded end to end (the data of tests/test_gpu_host_tool_kde.py): the KDE of a sharded
panel reduced over the shards' devices by garlic_kde_parts instead of merged on the host.

One device is one part, which garlic_kde_parts returns with garlic_feed_kde's bits: the same files and the same cutoff.
Two shards split the sums of the moments and of the Gaussian terms differently, so h and the density may differ in their
last bits (tests/test_gpu_kde_parts.py bounds that against the long-double reference); the .kde file prints six
significant digits, so its columns agree within one unit of the sixth digit, relative 1e-5 -- the only resolution the
file has -- and so does the printed cutoff."""
import os
import re
import subprocess

import numpy as np
import pytest

import kde_cases as cases
from test_gpu_host_tool_kde import BOUNDS, NIND, TOOL, data, printed_cutoff, run_tool  # noqa: F401  (data: the fixture)

pytestmark = pytest.mark.gpu
W = 60


def shards_line(stderr):
    """the P of every "KDE on <P> shards" line"""
    return re.findall(r"^KDE on (\d+) shards$", stderr, re.M)


def kde_file(out):
    return "%s.%dSNPs.kde" % (out, W)


def test_sharded_kde_on_one_and_two_devices(data, tmp_path):
    one, err1 = run_tool(data, tmp_path / "one", "--winsize", str(W), "--kde", "--devices", "0", *BOUNDS)
    assert shards_line(err1) == []
    # one device: one part, garlic_feed_kde's bits
    part, errp = run_tool(data, tmp_path / "part", "--winsize", str(W), "--kde", "--kde-sharded", "--devices", "0", *BOUNDS)
    assert shards_line(errp) == ["1"]
    assert open(kde_file(part), "rb").read() == open(kde_file(one), "rb").read()
    assert open(part + ".roh.bed", "rb").read() == open(one + ".roh.bed", "rb").read()
    assert printed_cutoff(errp) == printed_cutoff(err1)
    # two shards on the one GPU
    two, err2 = run_tool(data, tmp_path / "two", "--winsize", str(W), "--kde", "--kde-sharded", "--devices", "0,0", *BOUNDS)
    assert shards_line(err2) == ["2"]
    x1, y1 = cases.read_kde(kde_file(one))
    x2, y2 = cases.read_kde(kde_file(two))
    assert x1.shape == x2.shape == (512,)
    print("worst relative difference: x %.3g, y %.3g" % (np.max(np.abs(x2 - x1) / np.abs(x1)), np.max(np.abs(y2 - y1) / np.abs(y1))))
    assert (np.abs(x2 - x1) <= 1e-5 * np.abs(x1)).all() and (np.abs(y2 - y1) <= 1e-5 * np.abs(y1)).all()
    c1, c2 = float(printed_cutoff(err1)), float(printed_cutoff(err2))
    assert abs(c2 - c1) <= 1e-5 * abs(c1), (c1, c2)
    assert open(two + ".roh.bed", "rb").read().count(b"\n") > NIND
    # without the flag two shards take the path of before: the feeds merged on the host, the single device's bytes
    plain, err3 = run_tool(data, tmp_path / "plain", "--winsize", str(W), "--kde", "--devices", "0,0", *BOUNDS)
    assert shards_line(err3) == []
    assert open(kde_file(plain), "rb").read() == open(kde_file(one), "rb").read()
    assert open(plain + ".roh.bed", "rb").read() == open(one + ".roh.bed", "rb").read()
    assert printed_cutoff(err3) == printed_cutoff(err1)
    # the flag toggles like the others: given twice it is off
    off, err4 = run_tool(data, tmp_path / "off", "--winsize", str(W), "--kde", "--kde-sharded", "--kde-sharded", "--devices", "0,0", *BOUNDS)
    assert shards_line(err4) == [] and open(kde_file(off), "rb").read() == open(kde_file(one), "rb").read()


def test_kde_sharded_needs_kde(data, tmp_path):
    _, err = run_tool(data, tmp_path / "a", "--winsize", str(W), "--kde-sharded", ok=False)
    assert "--kde-sharded" in err and "--kde " in err
    r = subprocess.run([TOOL], capture_output=True, text=True)
    assert r.returncode != 0 and "--kde-sharded" in r.stderr
    assert not os.path.exists(os.path.join(str(tmp_path / "a"), "mine.%dSNPs.kde" % W))
