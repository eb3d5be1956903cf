"""GPU: garlic-lod --nclust end to end.  On tests/golden/e2e/tiny.* the reference's prebuilt binary wrote refs3.roh.bed /
refs2.roh.bed and the Gaussian and boundary lines of refs3.log.txt / refs2.log.txt (tools/make_golden_gmm.py,
COMMAND_gmm.txt): the tool's .roh.bed is byte-identical (no length lies within 2.4e-3 of a boundary, the solvers agree to
2e-4), its Gaussians agree to the printed digits, two shards give the same.  On a synthetic TPED with planted runs of three
sizes, --kde --nclust 3 goes from genotypes to classified calls and equals the run handed the cutoff and the bounds."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import kde_cases
from gmm_cases import golden_log, printed_alike

pytestmark = pytest.mark.gpu
ROOT = kde_cases.ROOT
E2E = os.path.join(ROOT, "tests", "golden", "e2e")
TOOL = os.path.join(ROOT, "garlic_amd", "host", "garlic-lod")
TINY = ["--tped", os.path.join(E2E, "tiny.tped.gz"), "--tfam", os.path.join(E2E, "tiny.tfam"),
        "--centromere", os.path.join(E2E, "tiny.centromeres.txt"), "--error", "0.001", "--kde-subsample", "0"]


def run(d, inputs, *extra, ok=True):
    os.makedirs(d, exist_ok=True)
    out = os.path.join(str(d), "mine")
    r = subprocess.run([TOOL] + list(inputs) + ["--out", out] + list(extra), capture_output=True, text=True)
    assert (r.returncode == 0) == ok, r.stderr[-2000:]
    return out, r.stderr


def printed(stderr):
    """(Gaussian (a, mean, var) strings per class, boundary strings) of a run's stderr"""
    gauss = re.findall(r"^Gaussian class (\w) \( mixture, mean, std \) = \( (\S+), (\S+), (\S+) \)$", stderr, re.M)
    bounds = re.findall(r"^Selected ROH size boundaries = \( (.*) \)$", stderr, re.M)
    assert len(bounds) == 1 and [g[0] for g in gauss] == [chr(65 + i) for i in range(len(gauss))], stderr[-2000:]
    return [g[1:] for g in gauss], bounds[0].split()


@pytest.mark.parametrize("tag,k", [("refs3", 3), ("refs2", 2)])
def test_golden_size_classes(tmp_path, tag, k):
    out, err = run(tmp_path / "a", TINY, "--winsize", "30", "--lod-cutoff", "-12", "--nclust", str(k))
    want_gauss, want_bounds = golden_log(tag)
    gauss, bounds = printed(err)
    assert len(gauss) == k and len(bounds) == k - 1
    for got, want in zip(gauss, want_gauss):
        assert all(printed_alike(g, w) for g, w in zip(got, want)), (got, want)
    for g, w in zip(bounds, want_bounds):
        assert abs(float(g) - float(w)) <= 2e-4 * float(w), (g, w)
    bed = open(out + ".roh.bed", "rb").read()
    assert bed == gzip.open(os.path.join(E2E, tag + ".roh.bed.gz"), "rb").read()
    # two shards on the one GPU: the pooled lengths arrive in the same order, so the same bits
    two, err2 = run(tmp_path / "b", TINY, "--winsize", "30", "--lod-cutoff", "-12", "--nclust", str(k), "--devices", "0,0")
    assert open(two + ".roh.bed", "rb").read() == bed
    keep = lambda e: [l for l in e.splitlines() if l.startswith(("Gaussian class", "Selected ROH size", "GMM with"))]
    assert keep(err2) == keep(err) and len(keep(err)) == k + 2


def test_refusals_and_the_runs_without_the_flag(tmp_path):
    _, err = run(tmp_path / "a", TINY, "--winsize", "30", "--lod-cutoff", "-12", "--nclust", "3", "--size-bounds", "50000", "200000", ok=False)
    assert "--nclust and --size-bounds exclude each other" in err
    _, err = run(tmp_path / "a", TINY, "--winsize", "30", "--lod-cutoff", "-12", ok=False)
    assert "--lod-cutoff writes the ROH calls and needs --size-bounds (the size classes otherwise come from GARLIC's GMM stage, " \
           "Phase II, not part of this tool)" in err
    for bad in ("0", "-2", "9"):
        _, err = run(tmp_path / "a", TINY, "--winsize", "30", "--lod-cutoff", "-12", "--nclust", bad, ok=False)
        assert "GMM clusters" in err
    r = subprocess.run([TOOL], capture_output=True, text=True)
    assert r.returncode != 0 and "--nclust K" in r.stderr
    # user bounds as before: the golden of the run with --size-bounds, no GMM line
    out, err = run(tmp_path / "b", TINY, "--winsize", "30", "--lod-cutoff", "-12", "--size-bounds", "50000", "200000")
    assert open(out + ".roh.bed", "rb").read() == gzip.open(os.path.join(E2E, "ref.roh.bed.gz"), "rb").read()
    assert "Gaussian class" not in err and "Selected ROH size boundaries" not in err


NSNP, NIND, W = 6000, 40, 60


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    """one chromosome, 6000 SNPs 1 kb apart, 40 individuals; every individual carries runs of about 150, 450 and 1100 SNPs
    in which both copies are the same haplotype: a bimodal score density and three size classes"""
    d = tmp_path_factory.mktemp("gmm_tool")
    rng = np.random.default_rng(9971)
    freq = rng.uniform(0.15, 0.85, NSNP)
    hap = (rng.random((NSNP, NIND, 2)) < freq[:, None, None]).astype(np.uint8)
    for i in range(NIND):
        starts = rng.permutation(4)[:3] * 1500 + rng.integers(0, 300, 3)
        for a, size in zip(starts, (150, 450, 1100)):
            b = int(a) + int(size * rng.uniform(0.85, 1.15))
            hap[int(a):b, i, 1] = hap[int(a):b, i, 0]
    letters = np.array(["A", "G"])
    with open(d / "syn.tped", "w") as f:
        for l in range(NSNP):
            f.write("1 rs%d 0 %d %s\n" % (l, 10000 + 1000 * l, " ".join(letters[hap[l].reshape(-1)])))
    with open(d / "syn.tfam", "w") as f:
        for i in range(NIND):
            f.write("POP ind%d 0 0 0 -9\n" % i)
    with open(d / "syn.centromeres.txt", "w") as f:
        f.write("1 90000000 90040000\n")
    return ["--tped", str(d / "syn.tped"), "--tfam", str(d / "syn.tfam"), "--centromere", str(d / "syn.centromeres.txt"),
            "--error", "0.001", "--kde-seed", "7"]


def test_kde_and_nclust_need_no_user_numbers(gpu_ctx, planted, tmp_path):
    """--kde --nclust 3: the cutoff from the density, the bounds from the mixture; the same calls as the run that is handed
    the cutoff (all its digits, from the density of the sorted feed) and the printed bounds (lengths are whole bp, the
    boundaries are printed to a tenth of a bp or finer)"""
    out, err = run(tmp_path / "a", planted, "--winsize", str(W), "--kde", "--nclust", "3")
    assert sorted(os.listdir(tmp_path / "a")) == ["mine.%dSNPs.kde" % W, "mine.freq.gz", "mine.roh.bed"]
    gauss, bounds = printed(err)
    assert len(gauss) == 3 and len(bounds) == 2 and float(bounds[0]) < float(bounds[1])
    assert all(float(b) < 1e6 for b in bounds)
    plain, _ = run(tmp_path / "feed", planted, "--winsize", str(W), "--sorted-feed")
    k = gpu_ctx.feed_kde(np.fromfile("%s.%dSNPs.lod.sorted.f64" % (plain, W), dtype=np.float64))
    cutoff = kde_cases.min_between_modes(k["x"], k["y"], W)[0]
    assert re.findall(r"^Selected LOD score cutoff: (\S+)$", err, re.M) == ["%g" % cutoff]
    by_hand, _ = run(tmp_path / "b", planted, "--winsize", str(W), "--lod-cutoff", repr(float(cutoff)), "--size-bounds", *bounds)
    bed = open(out + ".roh.bed", "rb").read()
    assert bed == open(by_hand + ".roh.bed", "rb").read()
    classes = [l.split(b"\t")[3] for l in bed.splitlines() if not l.startswith(b"track")]
    assert len(classes) >= 3 * NIND and set(classes) == {b"A", b"B", b"C"}
    # --kde alone still writes no calls
    run(tmp_path / "c", planted, "--winsize", str(W), "--kde")
    assert sorted(os.listdir(tmp_path / "c")) == ["mine.%dSNPs.kde" % W, "mine.freq.gz"]
