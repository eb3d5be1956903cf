"""GPU: garlic-lod --bfile against garlic-lod --tped on twin files written from one genotype matrix
(garlic_amd.synth.write_bed_and_tped): byte-identical outputs.  The TPED path is pinned to the reference's prebuilt binary by
tests/golden/e2e, so equality with it is equality with the reference under the het convention "A1 A2"."""
import filecmp
import glob
import gzip
import os
import subprocess

import numpy as np
import pytest

from garlic_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E2E = os.path.join(ROOT, "tests", "golden", "e2e")
TOOL = os.path.join(ROOT, "garlic_amd", "host", "garlic-lod")
COMMON = ["--centromere", os.path.join(E2E, "tiny.centromeres.txt"), "--kde-subsample", "0", "--winsize", "30", "--raw-lod"]
MODES = {
    "unweighted": ["--error", "0.001", "--lod-cutoff", "-12", "--size-bounds", "50000", "200000"],
    "weighted": ["--error", "0.001", "--weighted", "--map", os.path.join(E2E, "tiny.map"), "--ld-subsample", "11", "--ld-seed", "5",
                 "--lod-cutoff", "-4", "--size-bounds", "50000", "200000"],
    "tgls": ["--tgls", os.path.join(E2E, "tiny.tgls.gz"), "--gl-type", "GQ", "--lod-cutoff", "-11", "--size-bounds", "50000", "200000"],
}


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    """6,000 SNPs x 24 individuals on the chromosomes and positions of the e2e fixture (so its map, centromeres and
    likelihoods apply), genotypes of our own: all-missing SNPs, monomorphic SNPs of both alleles, SNPs that begin with
    missing genotypes, alleles that differ by row"""
    d = tmp_path_factory.mktemp("twin")
    chrs, pos = [], []
    with gzip.open(os.path.join(E2E, "tiny.tped.gz"), "rt") as f:
        for line in f:
            t = line.split(None, 4)
            chrs.append(t[0])
            pos.append(int(float(t[3])))
    n = len(chrs)
    rng = np.random.default_rng(2024)
    p = rng.uniform(0.05, 0.95, size=(n, 1))
    u = rng.random((n, 24))
    codes = np.where(u < (1 - p) ** 2, 3, np.where(u < (1 - p) ** 2 + 2 * p * (1 - p), 2, 0)).astype(np.uint8)
    codes[rng.random(codes.shape) < 0.03] = 1
    codes[::211] = 1                         # all missing
    codes[5::307] = 0                        # monomorphic A1
    codes[9::401] = 3                        # monomorphic A2
    codes[13::97, :5] = 1                    # the counted allele is found behind missing genotypes
    codes[0] = 1                             # the first row is dropped; the last one stays (and is polymorphic)
    codes[n - 1] = np.arange(24) % 4
    letters = np.array(list("ACGT"))
    a1 = letters[rng.integers(0, 4, size=n)]
    a2 = letters[(np.searchsorted(letters, a1) + rng.integers(1, 4, size=n)) % 4]
    prefix = str(d / "X")
    synth.write_bed_and_tped(prefix, codes, chrs, pos, a1=list(a1), a2=list(a2))
    return prefix


def run(tmp, inputs, *extra, ok=True):
    out = str(tmp / "mine")
    r = subprocess.run([TOOL, *inputs, "--out", out, *COMMON, *extra], capture_output=True, text=True)
    if ok:
        assert r.returncode == 0, r.stderr[-2000:]
        return out
    return r


def same_files(a, b):
    names = sorted(os.path.basename(p)[len("mine"):] for p in glob.glob(a + "*"))
    assert names == sorted(os.path.basename(p)[len("mine"):] for p in glob.glob(b + "*"))
    assert ".freq.gz" in names and ".roh.bed" in names and sum(n.endswith(".raw.lod.windows.gz") for n in names) == 3
    assert any(n.endswith(".lod.f64") for n in names)
    for n in names:
        assert filecmp.cmp(a + n, b + n, shallow=False), n


@pytest.mark.parametrize("mode", sorted(MODES))
def test_bfile_equals_the_twin_tped(tmp_path, twin, mode):
    (tmp_path / "bed").mkdir(), (tmp_path / "tped").mkdir(), (tmp_path / "three").mkdir()
    a = run(tmp_path / "bed", ["--bfile", twin], *MODES[mode])
    b = run(tmp_path / "tped", ["--tped", twin + ".tped", "--tfam", twin + ".tfam"], *MODES[mode])
    same_files(a, b)
    c = run(tmp_path / "three", ["--bed", twin + ".bed", "--bim", twin + ".bim", "--fam", twin + ".fam"], *MODES[mode])
    same_files(a, c)


def test_bfile_refuses_phased_and_tped(tmp_path, twin):
    r = run(tmp_path, ["--bfile", twin], *MODES["unweighted"], "--phased", ok=False)
    assert r.returncode != 0 and "phase" in r.stderr
    r = run(tmp_path, ["--bfile", twin, "--tped", twin + ".tped", "--tfam", twin + ".tfam"], *MODES["unweighted"], ok=False)
    assert r.returncode != 0 and "exclude" in r.stderr


def test_sharded_bfile_equals_single(tmp_path, twin):
    """several shards on GPU 0, each with its own context and column block of the one image"""
    outs = []
    for k, devs in enumerate(("0", "0,0", "0,0,0,0,0")):
        (tmp_path / str(k)).mkdir()
        outs.append(run(tmp_path / str(k), ["--bfile", twin], *MODES["weighted"], "--devices", devs))
    for other in outs[1:]:
        same_files(outs[0], other)


def test_two_gpus_equal_one(tmp_path, twin):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two visible devices")
    (tmp_path / "one").mkdir(), (tmp_path / "two").mkdir()
    same_files(run(tmp_path / "one", ["--bfile", twin], *MODES["unweighted"], "--gpus", "1"),
               run(tmp_path / "two", ["--bfile", twin], *MODES["unweighted"], "--gpus", "2"))


def test_cache_written_from_bed_loads_to_the_same_outputs(tmp_path, twin):
    cache = str(tmp_path / "X.g2b")
    (tmp_path / "bed").mkdir(), (tmp_path / "cache").mkdir()
    a = run(tmp_path / "bed", ["--bfile", twin], *MODES["unweighted"], "--genotype-cache", cache)
    assert os.path.getsize(cache) > 0
    b = run(tmp_path / "cache", ["--tped", twin + ".tped", "--tfam", twin + ".tfam"], *MODES["unweighted"], "--genotype-cache", cache)
    same_files(a, b)
