"""GPU: garlic-lod --vcf against garlic-lod --tped --tfam on twin files written from one phased genotype matrix
(garlic_amd.synth.write_vcf_and_tped: the TPED / TFAM are what vcf2tped.pl writes from the VCF; tests/test_vcf_cpu.py pins
that to the converter's own output): byte-identical outputs.  The TPED path is pinned to the reference's prebuilt binary by
tests/golden/e2e."""
import filecmp
import glob
import gzip
import os
import shutil
import subprocess

import numpy as np
import pytest

from garlic_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E2E = os.path.join(ROOT, "tests", "golden", "e2e")
GOLDEN = os.path.join(ROOT, "tests", "golden", "vcf")
TOOL = os.path.join(ROOT, "garlic_amd", "host", "garlic-lod")
COMMON = ["--centromere", os.path.join(E2E, "tiny.centromeres.txt"), "--kde-subsample", "0", "--winsize", "30"]
MODES = {
    "unweighted": ["--raw-lod", "--error", "0.001", "--lod-cutoff", "-12", "--size-bounds", "50000", "200000"],
    "weighted_phased": ["--raw-lod", "--error", "0.001", "--weighted", "--phased", "--map", os.path.join(E2E, "tiny.map"), "--ld-subsample", "11",
                        "--ld-seed", "5", "--lod-cutoff", "-4", "--size-bounds", "50000", "200000"],
    "tgls": ["--raw-lod", "--tgls", os.path.join(E2E, "tiny.tgls.gz"), "--gl-type", "GQ", "--lod-cutoff", "-11", "--size-bounds", "50000", "200000"],
    "kde_nclust": ["--error", "0.001", "--kde", "--nclust", "3"],
}


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    """6,000 SNPs x 24 individuals on the chromosomes and positions of the e2e fixture: all-missing rows, monomorphic rows of
    both alleles, rows that begin with missing genotypes, and rows whose first non-missing genotype is a 1|0 het -- on those
    the .bed rule (a het reads "A1 A2") would count the other allele, so a tool that ignored the order plane fails here"""
    d = tmp_path_factory.mktemp("vcftwin")
    chrs, pos = [], []
    with gzip.open(os.path.join(E2E, "tiny.tped.gz"), "rt") as f:
        for line in f:
            t = line.split(None, 4)
            chrs.append(t[0])
            pos.append(int(float(t[3])))
    n = len(chrs)
    rng = np.random.default_rng(2025)
    p = rng.uniform(0.05, 0.95, size=(n, 1))
    u = rng.random((n, 24))
    codes = np.where(u < (1 - p) ** 2, 3, np.where(u < (1 - p) ** 2 + 2 * p * (1 - p), 2, 0)).astype(np.uint8)
    codes[rng.random(codes.shape) < 0.03] = 1
    order = rng.integers(0, 2, size=codes.shape).astype(np.uint8)
    codes[17::53, 0] = 2                     # a 1|0 het first
    order[17::53, 0] = 1
    codes[29::61, :3] = 1                    # ./. ./. ./. and then a 1|0 het
    codes[29::61, 3] = 2
    order[29::61, 3] = 1
    codes[::211] = 1                         # all missing
    codes[5::307] = 0                        # monomorphic REF
    codes[9::401] = 3                        # monomorphic ALT
    codes[13::97, :5] = 1
    codes[0] = 1
    codes[n - 1] = np.arange(24) % 4
    order[codes == 3] = 1
    order[(codes == 0) | (codes == 1)] = 0
    first_het_alt = sum(1 for r in range(n) for nm in [np.flatnonzero(codes[r] != 1)] if nm.size and codes[r, nm[0]] == 2 and order[r, nm[0]])
    assert first_het_alt > 100
    letters = np.array(list("ACGT"))
    a1 = letters[rng.integers(0, 4, size=n)]
    a2 = letters[(np.searchsorted(letters, a1) + rng.integers(1, 4, size=n)) % 4]
    prefix = str(d / "X")
    synth.write_vcf_and_tped(prefix, codes, order, chrs, pos, a1=list(a1), a2=list(a2),
                             extra_subfields=lambda r, j: "%d,0.%d" % (r % 50, j) if (r + j) % 3 == 0 else "")
    with open(prefix + ".vcf", "rb") as f, gzip.open(prefix + ".vcf.gz", "wb") as g:
        shutil.copyfileobj(f, g)
    return prefix


def run(tmp, inputs, *extra, ok=True):
    tmp.mkdir(exist_ok=True)
    out = str(tmp / "mine")
    r = subprocess.run([TOOL, *inputs, "--out", out, *COMMON, *extra], capture_output=True, text=True)
    if ok:
        assert r.returncode == 0, r.stderr[-2000:]
        return out
    return r


def same_files(a, b, roh=True):
    names = sorted(os.path.basename(p)[len("mine"):] for p in glob.glob(a + "*"))
    assert names == sorted(os.path.basename(p)[len("mine"):] for p in glob.glob(b + "*"))
    assert ".freq.gz" in names and (not roh or ".roh.bed" in names) and len(names) >= 3, names
    for n in names:
        assert os.path.getsize(a + n) > 0, n
        assert filecmp.cmp(a + n, b + n, shallow=False), n


def tped_of(prefix):
    return ["--tped", prefix + ".tped", "--tfam", prefix + ".tfam"]


@pytest.mark.parametrize("mode", sorted(MODES))
def test_vcf_equals_the_twin_tped(tmp_path, twin, mode):
    a = run(tmp_path / "vcf", ["--vcf", twin + ".vcf"], *MODES[mode])
    b = run(tmp_path / "tped", tped_of(twin), *MODES[mode])
    same_files(a, b)


def test_gz_and_tfam(tmp_path, twin):
    a = run(tmp_path / "gz", ["--vcf", twin + ".vcf.gz", "--tfam", twin + ".tfam"], *MODES["weighted_phased"])
    b = run(tmp_path / "tped", tped_of(twin), *MODES["weighted_phased"])
    same_files(a, b)


def test_sharded_vcf_equals_single(tmp_path, twin):
    """several shards on GPU 0, each with its own context, column block and phase fill; five shards begin inside a byte of
    the order plane"""
    outs = [run(tmp_path / str(k), ["--vcf", twin + ".vcf"], *MODES["weighted_phased"], "--devices", devs)
            for k, devs in enumerate(("0", "0,0", "0,0,0,0,0"))]
    for other in outs[1:]:
        same_files(outs[0], other)


def test_golden_case_through_the_tool(tmp_path):
    """case1.vcf against the case1.tped that vcf2tped.pl wrote from it"""
    common = ["--error", "0.001", "--winsize", "3", "--raw-lod", "--lod-cutoff", "0", "--size-bounds", "1000", "5000"]
    case = os.path.join(GOLDEN, "case1")
    a = run(tmp_path / "vcf", ["--vcf", case + ".vcf"], *common)
    b = run(tmp_path / "tped", tped_of(case), *common)
    same_files(a, b, roh=False)


def test_cache_written_from_vcf_loads_to_the_same_outputs(tmp_path, twin):
    cache = str(tmp_path / "X.g2b")
    a = run(tmp_path / "vcf", ["--vcf", twin + ".vcf"], *MODES["weighted_phased"], "--genotype-cache", cache)
    assert os.path.getsize(cache) > 0
    b = run(tmp_path / "cache", tped_of(twin), *MODES["weighted_phased"], "--genotype-cache", cache)
    same_files(a, b)


def test_usage_errors(tmp_path, twin):
    vcf = ["--vcf", twin + ".vcf"]
    for extra in (["--tped", twin + ".tped"], ["--bfile", twin], ["--bed", twin + ".bed"], ["--bim", "x"], ["--fam", "x"],
                  ["--keep", "x"], ["--pops", "x"]):
        r = run(tmp_path, vcf + extra, *MODES["unweighted"], ok=False)
        assert r.returncode != 0 and "--vcf" in r.stderr, (extra, r.stderr[-300:])
    r = run(tmp_path, tped_of(twin), "--vcf-biallelic-snps-only", *MODES["unweighted"], ok=False)
    assert r.returncode != 0 and "--vcf" in r.stderr


def edited(twin, tmp_path, edit):
    lines = open(twin + ".vcf").read().split("\n")
    first = next(k for k, ln in enumerate(lines) if ln and not ln.startswith("#"))
    edit(lines, first)
    path = str(tmp_path / "edited.vcf")
    open(path, "w").write("\n".join(lines))
    return path, first


def test_multi_allelic_refusal_and_skip_count(tmp_path, twin):
    def edit(lines, first):
        for k in (first + 10, first + 20, first + 30):
            t = lines[k].split("\t")
            t[4] = {first + 10: "G,T", first + 20: "<DEL>", first + 30: "."}[k]
            lines[k] = "\t".join(t)
    path, first = edited(twin, tmp_path, edit)
    r = run(tmp_path / "refused", ["--vcf", path], *MODES["unweighted"], ok=False)
    assert r.returncode != 0 and "line %d of" % (first + 11) in r.stderr and "G,T" in r.stderr, r.stderr[-500:]
    r = run(tmp_path / "skipped", ["--vcf", path, "--vcf-biallelic-snps-only"], *MODES["unweighted"], ok=False)
    assert r.returncode == 0 and "Left out 3 lines" in r.stderr, r.stderr[-500:]
    # the same run from a TPED without those three lines
    drop = {10, 20, 30}
    tped = [ln for k, ln in enumerate(open(twin + ".tped").read().splitlines()) if k not in drop]
    open(str(tmp_path / "less.tped"), "w").write("".join(ln + "\n" for ln in tped))
    b = run(tmp_path / "tped", ["--tped", str(tmp_path / "less.tped"), "--tfam", twin + ".tfam"], *MODES["unweighted"])
    same_files(str(tmp_path / "skipped" / "mine"), b)


@pytest.mark.parametrize("gt,what", [("./1", "half-missing"), ("1", "haploid"), ("0|2", "allele index")])
def test_genotype_offences_fail_the_run_with_line_and_sample(tmp_path, twin, gt, what):
    def edit(lines, first):
        t = lines[first + 40].split("\t")
        t[9 + 6] = gt
        lines[first + 40] = "\t".join(t)
    path, first = edited(twin, tmp_path, edit)
    for flags in ([], ["--vcf-biallelic-snps-only"]):
        r = run(tmp_path / "bad", ["--vcf", path, *flags], *MODES["unweighted"], ok=False)
        assert r.returncode != 0 and "line %d of" % (first + 41) in r.stderr and "ind6" in r.stderr and what in r.stderr, r.stderr[-500:]
