"""GPU: garlic-lod --features with the counting genotypes as a PLINK file set (--bfile-counting).  The golden cases of
tests/golden/features, their TPED lines converted to .bed / .bim / .fam, give the table the reference's
count_features_in_roh.pl printed, byte for byte.  On a planted .bed / TPED twin the table counted from the .bed equals the
one counted from the twin TPED, byte for byte, also under --keep; the feature file there annotates A1 alleles, A2 alleles,
alleles that are neither, the allele `0` and sites the .bim does not have."""
import os
import subprocess

import numpy as np
import pytest

import feature_cases as fc
from garlic_amd import synth
from test_feature_bed_cpu import golden_bed

pytestmark = pytest.mark.gpu
TOOL = os.path.join(fc.ROOT, "garlic_amd", "host", "garlic-lod")
NSNP, NIND, W = 6000, 40, 60


@pytest.mark.parametrize("case", fc.GOLDEN_CASES)
def test_roh_bed_on_the_converted_goldens_reproduces_the_scripts_table(case, tmp_path):
    prefix = golden_bed(case, tmp_path)          # asserts at most two alleles per line, but for feature_bed_cases.THREE_ALLELES
    out = str(tmp_path / "mine")
    r = subprocess.run([TOOL, "--roh-bed", fc.golden_path(case, "roh.bed"), "--features", fc.golden_path(case, "features.txt"),
                        "--bfile-counting", prefix, "--out", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(out + ".feature.counts", "rb").read() == open(fc.golden_path(case, "expected.counts"), "rb").read()
    # the three files named one by one
    r = subprocess.run([TOOL, "--roh-bed", fc.golden_path(case, "roh.bed"), "--features", fc.golden_path(case, "features.txt"),
                        "--bed-counting", prefix + ".bed", "--bim-counting", prefix + ".bim", "--fam-counting", prefix + ".fam",
                        "--out", out + "3"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(out + "3.feature.counts", "rb").read() == open(fc.golden_path(case, "expected.counts"), "rb").read()


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    """one chromosome, 6000 SNPs 1 kb apart, 40 individuals with planted runs of about 150, 450 and 1100 homozygous SNPs (the
    data of tests/test_gpu_host_tool_gmm.py: a bimodal score density, three size classes), 2 % missing, as .bed / .bim / .fam
    and as the twin TPED / TFAM with per-row allele letters; the feature file; a keep file of every other individual"""
    d = tmp_path_factory.mktemp("features_bed_tool")
    rng = np.random.default_rng(9971)
    freq = rng.uniform(0.15, 0.85, NSNP)
    hap = (rng.random((NSNP, NIND, 2)) < freq[:, None, None]).astype(np.uint8)
    for i in range(NIND):
        starts = rng.permutation(4)[:3] * 1500 + rng.integers(0, 300, 3)
        for a, size in zip(starts, (150, 450, 1100)):
            b = int(a) + int(size * rng.uniform(0.85, 1.15))
            hap[int(a):b, i, 1] = hap[int(a):b, i, 0]
    codes = np.where(hap[:, :, 0] != hap[:, :, 1], 2, np.where(hap[:, :, 0] == 1, 3, 0)).astype(np.uint8)
    codes[rng.random(codes.shape) < 0.02] = 1
    letters = np.array(list("ACGT"))
    a1 = letters[rng.integers(0, 4, size=NSNP)]
    a2 = letters[(np.searchsorted(letters, a1) + rng.integers(1, 4, size=NSNP)) % 4]
    pos = 10000 + 1000 * np.arange(NSNP)
    prefix = str(d / "syn")
    synth.write_bed_and_tped(prefix, codes, ["1"] * NSNP, pos, a1=list(a1), a2=list(a2), pad_bits=0xFF)
    with open(prefix + ".centromeres.txt", "w") as f:
        f.write("1 90000000 90040000\n")
    effects = ["benign", "damaging", "lof"]
    drawn = {"a1": 0, "a2": 0, "neither": 0, "both": 0, "zero": 0, "absent": 0}
    with open(prefix + ".features.txt", "w") as f:
        for l in range(0, NSNP, 3):
            kind = ("a1", "a2", "neither", "both", "a1", "a2", "zero")[(l // 3) % 7]
            other = [c for c in "ACGT" if c not in (a1[l], a2[l])][0]
            for allele in {"a1": [a1[l]], "a2": [a2[l]], "neither": [other], "both": [a1[l], a2[l]], "zero": ["0", a2[l]]}[kind]:
                f.write("chr1:%d N %s %s\n" % (pos[l], allele, effects[(l + ord(allele)) % 3]))
            drawn[kind] += 1
            if l % 30 == 0:
                f.write("chr1:%d N A lof\n" % (pos[l] + 7))                 # between two SNPs: not in the .bim
                drawn["absent"] += 1
    assert all(v > 100 for v in drawn.values()), drawn
    with open(prefix + ".keep", "w") as f:
        f.write("".join("POP ind%d\n" % i for i in range(0, NIND, 2)))
    return prefix


def run(d, prefix, *extra):
    os.makedirs(str(d))
    out = os.path.join(str(d), "mine")
    r = subprocess.run([TOOL, "--bfile", prefix, "--centromere", prefix + ".centromeres.txt", "--error", "0.001", "--kde-seed", "7",
                        "--winsize", str(W), "--kde", "--nclust", "3", "--features", prefix + ".features.txt", "--out", out, *extra],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out + ".feature.counts"


@pytest.mark.parametrize("keep", [False, True], ids=["everyone", "keep"])
def test_table_from_the_bed_equals_the_table_from_the_twin_tped(twin, tmp_path, keep):
    extra = ["--keep", twin + ".keep"] if keep else []
    from_bed = run(tmp_path / "bed", twin, "--bfile-counting", twin, *extra)
    from_tped = run(tmp_path / "tped", twin, "--tped-counting", twin + ".tped", *extra)
    assert open(from_bed, "rb").read() == open(from_tped, "rb").read()
    cols, rows = fc.read_table(from_bed)
    assert cols == [e + k for e in ("benign", "damaging", "lof") for k in ("A", "B", "C", "NONE")]
    assert list(rows) == ["ind%d" % i for i in range(NIND)]                 # the counting .fam's individuals, kept or not
    inside = {iid: sum(v[j] for j in range(12) if j % 4 != 3) for iid, v in rows.items()}
    outside = sum(sum(v[3::4]) for v in rows.values())
    assert outside > 1000 and sum(inside.values()) > 1000, (outside, sum(inside.values()))
    if keep:      # an individual that is not in the run has no ROH: all its homozygotes are outside
        assert all(inside["ind%d" % i] == 0 for i in range(1, NIND, 2)) and all(inside["ind%d" % i] > 0 for i in range(0, NIND, 2))


def test_bfile_counting_with_tped_counting_is_a_usage_error(twin):
    r = subprocess.run([TOOL, "--bfile", twin, "--centromere", twin + ".centromeres.txt", "--error", "0.001", "--winsize", str(W), "--kde",
                        "--nclust", "3", "--features", twin + ".features.txt", "--out", twin + ".never", "--bfile-counting", twin,
                        "--tped-counting", twin + ".tped"], capture_output=True, text=True)
    assert r.returncode != 0 and "usage:" in r.stderr and "exclude each other" in r.stderr.split("\n")[0]
    assert not os.path.exists(twin + ".never.feature.counts")
