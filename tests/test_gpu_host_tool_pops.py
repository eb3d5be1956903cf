"""GPU: garlic-lod --keep / --pops on a PLINK file set with three family IDs interleaved in its .fam, against garlic-lod --bfile
on per-population file sets written from the same genotype matrix's columns: byte-identical outputs, file for file.  (The
--bfile path is pinned to the TPED path by tests/test_gpu_host_tool_bed.py, and that to the reference by tests/golden/e2e.)"""
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
    "tgls": ["--tgls", None, "--gl-type", "GQ", "--lod-cutoff", "-11", "--size-bounds", "50000", "200000"],
}
# family ID of each of the 24 individuals: 10 / 9 / 5 members, interleaved
FIDS = ["EAST", "WEST", "EAST", "ISLE", "WEST", "EAST", "WEST", "EAST", "ISLE", "WEST", "EAST", "EAST",
        "WEST", "ISLE", "WEST", "EAST", "WEST", "EAST", "ISLE", "WEST", "EAST", "WEST", "ISLE", "EAST"]
POPS = ["EAST", "WEST", "ISLE"]      # first-seen order


def members(pop):
    return [i for i, f in enumerate(FIDS) if f == pop]


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    """the 6,000-SNP x 24-individual twin of test_gpu_host_tool_bed.py with three family IDs in its .fam; per population a file
    set (and TPED twin) of its columns with the same individual IDs and that family ID alone, its keep file, and its columns
    of the likelihood file"""
    d = tmp_path_factory.mktemp("pops")
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
    codes[0] = 1
    codes[n - 1] = np.arange(24) % 4
    letters = np.array(list("ACGT"))
    a1 = letters[rng.integers(0, 4, size=n)]
    a2 = letters[(np.searchsorted(letters, a1) + rng.integers(1, 4, size=n)) % 4]
    assert sorted(set(FIDS), key=FIDS.index) == POPS and [len(members(q)) for q in POPS] == [10, 9, 5]

    def fam_lines(idx):
        return "".join("%s ind%d 0 0 0 -9\n" % (FIDS[i], i) for i in idx)

    full = str(d / "X")
    synth.write_bed_and_tped(full, codes, chrs, pos, a1=list(a1), a2=list(a2))
    os.remove(full + ".tped"), os.remove(full + ".tfam")
    with open(full + ".fam", "w") as f:
        f.write(fam_lines(range(24)))
    with gzip.open(os.path.join(E2E, "tiny.tgls.gz"), "rt") as f:
        tgls = [line.split() for line in f]
    assert all(len(t) == 24 + 4 for t in tgls)
    out = {"full": full, "tgls": os.path.join(E2E, "tiny.tgls.gz"), "pop": {}}
    for q in POPS:
        idx = members(q)
        prefix = str(d / q)
        synth.write_bed_and_tped(prefix, codes[:, idx], chrs, pos, a1=list(a1), a2=list(a2))
        for ext in (".fam", ".tfam"):
            with open(prefix + ext, "w") as f:
                f.write(fam_lines(idx))
        # the keep file in another order than the .fam, with further columns, a blank line and a pair twice
        with open(prefix + ".keep", "w") as f:
            f.write("".join("%s ind%d extra\n" % (q, i) for i in reversed(idx)) + "\n%s ind%d\n" % (q, idx[0]))
        with open(prefix + ".tgls", "w") as f:
            for t in tgls:
                f.write(" ".join(t[:4] + [t[4 + i] for i in idx]) + "\n")
        out["pop"][q] = prefix
    return out


def mode_args(mode, tgls):
    return [tgls if a is None else a for a in MODES[mode]]


def run(tmp, inputs, *extra, ok=True, name="mine"):
    os.makedirs(str(tmp), exist_ok=True)
    out = os.path.join(str(tmp), name)
    r = subprocess.run([TOOL, *inputs, "--out", out, *COMMON, *extra], capture_output=True, text=True)
    if ok:
        assert r.returncode == 0, r.stderr[-2000:]
        return out
    return r


def same_files(a, b):
    """the files a* and b*: the same names behind the prefix, the same bytes"""
    names = sorted(p[len(a):] for p in glob.glob(a + "*"))
    assert names == sorted(p[len(b):] for p in glob.glob(b + "*")), (a, b)
    assert ".freq.gz" in names and ".roh.bed" in names and sum(n.endswith(".raw.lod.windows.gz") for n in names) == 3
    assert any(n.endswith(".lod.f64") for n in names)
    for n in names:
        assert filecmp.cmp(a + n, b + n, shallow=False), n


@pytest.mark.parametrize("mode", sorted(MODES))
def test_keep_equals_the_per_population_file_set(tmp_path, sets, mode):
    for q in POPS:
        prefix = sets["pop"][q]
        a = run(tmp_path / q / "keep", ["--bfile", sets["full"], "--keep", prefix + ".keep"], *mode_args(mode, sets["tgls"]))
        b = run(tmp_path / q / "own", ["--bfile", prefix], *mode_args(mode, prefix + ".tgls"))
        same_files(a, b)
        assert any((".%s." % q) in os.path.basename(p) for p in glob.glob(a + "*"))      # the kept individuals' FID names the population


def test_pops_all_equals_the_three_per_population_runs(tmp_path, sets):
    args = mode_args("unweighted", None)
    a = run(tmp_path / "pops", ["--bfile", sets["full"], "--pops", "all"], *args)
    for q in POPS:
        b = run(tmp_path / "own", ["--bfile", sets["pop"][q]], *args, name="mine." + q)
        same_files(a + "." + q, b)
    # nothing besides the three populations' files
    assert len(glob.glob(a + "*")) == sum(len(glob.glob(a + "." + q + "*")) for q in POPS)
    # a list of names: those populations only, in the order given
    c = run(tmp_path / "two", ["--bed", sets["full"] + ".bed", "--bim", sets["full"] + ".bim", "--fam", sets["full"] + ".fam",
                               "--pops", "ISLE", "EAST"], *args)
    assert not glob.glob(c + ".WEST*")
    for q in ("ISLE", "EAST"):
        same_files(c + "." + q, a + "." + q)


def test_keep_on_three_shards_equals_one_device(tmp_path, sets):
    keep = ["--bfile", sets["full"], "--keep", sets["pop"]["EAST"] + ".keep"]
    same_files(run(tmp_path / "one", keep, *mode_args("weighted", None)),
               run(tmp_path / "three", keep, *mode_args("weighted", None), "--devices", "0,0,0"))


def test_cache_written_under_keep_loads_into_the_twin_tped_run(tmp_path, sets):
    prefix = sets["pop"]["WEST"]
    cache = str(tmp_path / "west.g2b")
    args = mode_args("unweighted", None)
    a = run(tmp_path / "keep", ["--bfile", sets["full"], "--keep", prefix + ".keep"], *args, "--genotype-cache", cache)
    assert os.path.getsize(cache) > 0
    b = run(tmp_path / "cache", ["--tped", prefix + ".tped", "--tfam", prefix + ".tfam"], *args, "--genotype-cache", cache)
    same_files(a, b)
    c = run(tmp_path / "tped", ["--tped", prefix + ".tped", "--tfam", prefix + ".tfam"], *args)
    same_files(a, c)


def test_refusals(tmp_path, sets):
    full, east = sets["full"], sets["pop"]["EAST"]
    args = mode_args("unweighted", None)
    tped = ["--tped", east + ".tped", "--tfam", east + ".tfam"]
    cases = [
        (tped + ["--keep", east + ".keep"], "--tped"),
        (tped + ["--pops", "all"], "--tped"),
        (["--bfile", full, "--keep", east + ".keep", "--pops", "all"], "--pops"),
        (["--bfile", full, "--pops", "all", "--freq-file", str(tmp_path / "f.freq.gz")], "--freq-file"),
        (["--bfile", full, "--pops", "all", "--genotype-cache", str(tmp_path / "c.g2b")], "--genotype-cache"),
        (["--pops", "all", "--roh-bed", str(tmp_path / "x.roh.bed"), "--features", "f", "--tped-counting", "t"], "--roh-bed"),
        (["--bfile", full, "--pops", "EAST", "NORTH"], "NORTH"),
    ]
    for inputs, word in cases:
        r = run(tmp_path, inputs, *args, ok=False)
        assert r.returncode != 0 and word in r.stderr and "ERROR" in r.stderr, (inputs, r.stderr[-500:])
    assert not glob.glob(str(tmp_path / "mine*"))                    # refused before anything was written
    # a keep file over two family IDs: the single-population check, over the kept individuals
    mixed = tmp_path / "mixed.keep"
    mixed.write_text("EAST ind0\nWEST ind1\n")
    r = run(tmp_path, ["--bfile", full, "--keep", str(mixed)], *args, ok=False)
    assert r.returncode != 0 and "multiple population IDs" in r.stderr
    unknown = tmp_path / "unknown.keep"
    unknown.write_text("EAST ind0\nEAST ind1\n")
    r = run(tmp_path, ["--bfile", full, "--keep", str(unknown)], *args, ok=False)
    assert r.returncode != 0 and "(EAST ind1)" in r.stderr and "line 2" in r.stderr
    # without the new flags: as before
    r = run(tmp_path, ["--bfile", full], *args, ok=False)
    assert r.returncode != 0 and "multiple population IDs" in r.stderr
