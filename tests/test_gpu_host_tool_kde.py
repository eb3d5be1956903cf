"""GPU: garlic-lod --kde end to end on a small synthetic TPED with planted homozygous runs (a bimodal density): the .kde
file, the printed cutoff, the ROH calls at that cutoff, the --auto-winsize loop, two shards on one GPU, and the unchanged
behaviour without the flag.  What the file must hold comes from Context.feed_kde on the feed a run WITHOUT --kde writes,
and from the Python get_min_btw_modes / wiggle of tests/kde_cases.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import kde_cases as cases

pytestmark = pytest.mark.gpu
ROOT = cases.ROOT
TOOL = os.path.join(ROOT, "garlic_amd", "host", "garlic-lod")
NSNP, NIND, SEED = 3000, 40, "7"
BOUNDS = ["--size-bounds", "500000", "2000000"]


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """one chromosome, 3000 SNPs 1 kb apart, 40 individuals; every individual carries a few runs of 150-400 SNPs in which
    both copies are the same haplotype"""
    d = tmp_path_factory.mktemp("kde_tool")
    rng = np.random.default_rng(9970)
    freq = rng.uniform(0.15, 0.85, NSNP)
    hap = (rng.random((NSNP, NIND, 2)) < freq[:, None, None]).astype(np.uint8)
    for i in range(NIND):
        for _ in range(3):
            a = int(rng.integers(0, NSNP - 400))
            b = a + int(rng.integers(150, 400))
            hap[a:b, i, 1] = hap[a:b, i, 0]
    letters = np.array(["A", "G"])
    with open(d / "syn.tped", "w") as f:
        for l in range(NSNP):
            f.write("1 rs%d 0 %d %s\n" % (l, 10000 + 1000 * l, " ".join(letters[hap[l].reshape(-1)])))
    with open(d / "syn.tfam", "w") as f:
        for i in range(NIND):
            f.write("POP ind%d 0 0 0 -9\n" % i)
    with open(d / "syn.centromeres.txt", "w") as f:
        f.write("1 90000000 90040000\n")
    return d


def run_tool(data, d, *extra, ok=True):
    os.makedirs(d, exist_ok=True)
    out = os.path.join(str(d), "mine")
    cmd = [TOOL, "--tped", str(data / "syn.tped"), "--tfam", str(data / "syn.tfam"), "--centromere", str(data / "syn.centromeres.txt"),
           "--out", out, "--error", "0.001", "--kde-seed", SEED]
    r = subprocess.run(cmd + list(extra), capture_output=True, text=True)
    assert (r.returncode == 0) == ok, r.stderr[-2000:]
    return out, r.stderr


def printed_cutoff(stderr):
    m = re.findall(r"^Selected LOD score cutoff: (\S+)$", stderr, re.M)
    assert len(m) == 1, stderr[-2000:]
    return m[0]


def expected_kde(gpu_ctx, data, tmp_path, W):
    """the density of the sorted feed that a run without --kde writes"""
    plain, _ = run_tool(data, tmp_path / ("feed%d" % W), "--winsize", str(W), "--sorted-feed")
    feed = np.fromfile("%s.%dSNPs.lod.sorted.f64" % (plain, W), dtype=np.float64)
    assert feed.shape[0] > 100
    return gpu_ctx.feed_kde(feed)


def test_kde_file_cutoff_and_roh_calls(gpu_ctx, data, tmp_path):
    W = 60
    k = expected_kde(gpu_ctx, data, tmp_path, W)
    out, err = run_tool(data, tmp_path / "a", "--winsize", str(W), "--kde", *BOUNDS)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["mine.%dSNPs.kde" % W, "mine.freq.gz", "mine.roh.bed"], names        # the feed itself is not written
    text = open("%s.%dSNPs.kde" % (out, W)).read()
    assert text == cases.kde_lines(k["x"], k["y"])
    cutoff, at, modes, _ = cases.min_between_modes(k["x"], k["y"], W)
    assert modes[0] < at < modes[1] and k["x"][modes[0]] < 0 < k["x"][modes[1]], "the planted runs make the density bimodal"
    assert printed_cutoff(err) == "%g" % cutoff
    # the same calls as a run that is handed the cutoff (all its digits)
    by_hand, _ = run_tool(data, tmp_path / "b", "--winsize", str(W), "--lod-cutoff", repr(float(cutoff)), *BOUNDS)
    bed = open(out + ".roh.bed", "rb").read()
    assert bed == open(by_hand + ".roh.bed", "rb").read() and bed.count(b"\n") > NIND
    # two shards on the one GPU: merged sorted feeds, the same file and the same calls
    two, err2 = run_tool(data, tmp_path / "c", "--winsize", str(W), "--kde", "--devices", "0,0", *BOUNDS)
    assert open("%s.%dSNPs.kde" % (two, W)).read() == text and printed_cutoff(err2) == printed_cutoff(err)
    assert open(two + ".roh.bed", "rb").read() == bed


def test_auto_winsize_runs_the_loop(gpu_ctx, data, tmp_path):
    """selectWinsize: from --winsize in steps of --auto-winsize-step until the wiggle is <= 0.50; that size's file only,
    holding 100 y (calculateWiggle scales in place before the reference writes)"""
    start, step = 20, 40
    out, err = run_tool(data, tmp_path / "a", "--winsize", str(start), "--auto-winsize", "--auto-winsize-step", str(step), "--kde")
    rows = [(int(a), float(b)) for a, b in re.findall(r"^(\d+)\t(\S+)$", err, re.M)]
    assert len(rows) > 1, "the data no longer make the loop take a step"
    assert [w for w, _ in rows] == [start + step * i for i in range(len(rows))]
    W = rows[-1][0]
    for i, (w, mse) in enumerate(rows):
        k = expected_kde(gpu_ctx, data, tmp_path, w)
        want = cases.wiggle(k["x"], k["y"])
        assert abs(mse - want) <= 1e-5 * want, (w, mse, want)                      # six printed digits
        assert (want <= 0.50) == (i == len(rows) - 1), (w, want)
    assert sorted(n for n in os.listdir(tmp_path / "a") if n.endswith(".kde")) == ["mine.%dSNPs.kde" % W]
    assert open("%s.%dSNPs.kde" % (out, W)).read() == cases.kde_lines(k["x"], k["y"], 100.0)
    assert printed_cutoff(err) == "%g" % cases.min_between_modes(k["x"], k["y"] * 100.0, W)[0]
    # selectWinsizeFromList: the last size is taken when none passes
    sizes = [rows[0][0], rows[0][0] + 2]              # the first fails the threshold (above); two sizes apart, so does the second
    out, err = run_tool(data, tmp_path / "b", "--winsize-multi", *map(str, sizes), "--auto-winsize", "--kde")
    assert sorted(n for n in os.listdir(tmp_path / "b") if n.endswith(".kde")) == ["mine.%dSNPs.kde" % sizes[-1]]
    listed = [(int(a), float(b)) for a, b in re.findall(r"^(\d+)\t(\S+)$", err, re.M)]
    assert [w for w, _ in listed] == sizes and all(m > 0.50 for _, m in listed), "none passes: the last is taken"
    # --winsize-multi without --auto-winsize: every size's density, no feed files
    out, err = run_tool(data, tmp_path / "c", "--winsize-multi", "60", "90", "--kde")
    assert sorted(os.listdir(tmp_path / "c")) == ["mine.60SNPs.kde", "mine.90SNPs.kde", "mine.freq.gz"]
    assert len(re.findall(r"^Selected LOD score cutoff: ", err, re.M)) == 2


def test_refusals_and_the_run_without_the_flag(data, tmp_path):
    _, err = run_tool(data, tmp_path / "a", "--winsize", "60", "--kde", "--raw-lod", ok=False)
    assert "--kde and --raw-lod" in err
    for flag in ("--sorted-feed", "--winsize-stream"):
        _, err = run_tool(data, tmp_path / "a", "--winsize", "60", "--kde", flag, ok=False)
        assert "--kde and %s" % flag in err
    r = subprocess.run([TOOL], capture_output=True, text=True)
    assert r.returncode != 0 and "--kde" in r.stderr
    # without --kde: the files and messages of before
    out, err = run_tool(data, tmp_path / "b", "--winsize", "60", "--auto-winsize")
    assert sorted(os.listdir(tmp_path / "b")) == ["mine.60SNPs.lod.f64", "mine.freq.gz"]
    assert "NOTE: --auto-winsize picks among the feeds above in GARLIC's KDE stage (Phase II, not part of this tool)" in err
    assert "Selected LOD score cutoff" not in err and "KDE results" not in err
