"""GPU: garlic-lod --features end to end.  --roh-bed on the golden cases of tests/golden/features gives the table the
reference's count_features_in_roh.pl printed, byte for byte.  On the tiny data set of tests/golden/e2e the table written
right after the .roh.bed equals the one --roh-bed makes from that very file, on one shard and on two; a fourth size class
gets its own columns and no genotype leaves the table."""
import gzip
import os
import subprocess

import pytest

import feature_cases as fc
from test_feature_counts_cpu import joined_tped
from test_gpu_host_tool import E2E, TOOL, run_tool

pytestmark = pytest.mark.gpu
CALLS = ["--winsize", "30", "--lod-cutoff", "-12"]
EFFECTS = ["benign", "damaging", "lof"]
THREE, FOUR = ["50000", "100000"], ["20000", "50000", "100000"]     # the calls at this cutoff run from under 20 kb to over 100 kb


def fresh(d):
    os.makedirs(str(d))
    return d


def from_bed(d, bed, features, tped, tfam=None):
    os.makedirs(str(d), exist_ok=True)
    out = os.path.join(str(d), "again")
    cmd = [TOOL, "--roh-bed", bed, "--features", features, "--tped-counting", tped, "--out", out]
    r = subprocess.run(cmd + (["--tfam-counting", tfam] if tfam else []), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out + ".feature.counts"


@pytest.mark.parametrize("case", fc.GOLDEN_CASES)
def test_roh_bed_reproduces_the_scripts_table(case, tmp_path):
    tped, _ = joined_tped(case, tmp_path)            # the TFAM is found beside it
    table = from_bed(tmp_path, fc.golden_path(case, "roh.bed"), fc.golden_path(case, "features.txt"), tped)
    assert open(table, "rb").read() == open(fc.golden_path(case, "expected.counts"), "rb").read()


@pytest.fixture(scope="module")
def counting(tmp_path_factory):
    """a counting TPED of its own from tiny.tped.gz -- four lines of five, plain text -- and a feature file that annotates
    one allele at two positions of three and both alleles, with different effects, at every seventh"""
    d = tmp_path_factory.mktemp("features_tool")
    tped, features = str(d / "counting.chrs.tped"), str(d / "features.txt")
    with gzip.open(os.path.join(E2E, "tiny.tped.gz"), "rt") as f, open(tped, "w") as t, open(features, "w") as a:
        for k, line in enumerate(f):
            if k % 5 == 4:
                continue
            t.write(line)
            tok = line.split()
            alleles = sorted(set(tok[4:]) - {"0"})
            if k % 3 == 2 or not alleles:
                continue
            a.write("chr%s:%s N %s %s\n" % (tok[0], tok[3], alleles[0], EFFECTS[k % 3]))
            if k % 7 == 0 and len(alleles) > 1:
                a.write("chr%s:%s N %s %s\n" % (tok[0], tok[3], alleles[1], EFFECTS[(k + 1) % 3]))
    return tped, os.path.join(E2E, "tiny.tfam"), features


def test_table_in_the_pipeline_equals_the_table_from_its_roh_bed(counting, tmp_path):
    tped, tfam, features = counting
    flags = ["--features", features, "--tped-counting", tped, "--tfam-counting", tfam]
    out = run_tool(fresh(tmp_path / "one"), *CALLS, "--size-bounds", *THREE, *flags)
    mine = open(out + ".feature.counts", "rb").read()
    cols, rows = fc.read_table(out + ".feature.counts")
    assert cols == [e + k for e in EFFECTS for k in ("A", "B", "C", "NONE")] and len(rows) == 24
    inside = sum(sum(v[j] for j in range(12) if j % 4 != 3) for v in rows.values())
    outside = sum(sum(v[3::4]) for v in rows.values())
    assert inside > 100 and outside > 100, (inside, outside)
    assert open(from_bed(tmp_path / "bed", out + ".roh.bed", features, tped, tfam), "rb").read() == mine
    # two shards on the one GPU: the counting individuals are not sharded, the calls are the same
    two = run_tool(fresh(tmp_path / "two"), *CALLS, "--size-bounds", *THREE, *flags, "--devices", "0,0")
    assert open(two + ".roh.bed", "rb").read() == open(out + ".roh.bed", "rb").read()
    assert open(two + ".feature.counts", "rb").read() == mine
    # four classes: A B C D NONE, and every individual's genotypes are all still there
    four = run_tool(fresh(tmp_path / "four"), *CALLS, "--size-bounds", *FOUR, *flags)
    cols4, rows4 = fc.read_table(four + ".feature.counts")
    assert cols4 == [e + k for e in EFFECTS for k in ("A", "B", "C", "D", "NONE")]
    assert b"\tD\t" in open(four + ".roh.bed", "rb").read() and b"\tC\t" in open(out + ".roh.bed", "rb").read()
    for iid, v in rows.items():
        for e in range(3):
            assert sum(v[4 * e: 4 * e + 4]) == sum(rows4[iid][5 * e: 5 * e + 5]), (iid, e)
    assert open(from_bed(tmp_path / "bed4", four + ".roh.bed", features, tped, tfam), "rb").read() == open(four + ".feature.counts", "rb").read()


def test_window_size_in_the_name_where_the_roh_bed_carries_it(counting, tmp_path):
    tped, tfam, features = counting
    out = run_tool(fresh(tmp_path / "multi"), "--winsize-multi", "30", "40", "--lod-cutoff", "-12", "--size-bounds", "50000", "200000",
                   "--features", features, "--tped-counting", tped, "--tfam-counting", tfam)
    for W in (30, 40):
        assert os.path.exists("%s.%dSNPs.roh.bed" % (out, W)) and os.path.exists("%s.%dSNPs.feature.counts" % (out, W))
