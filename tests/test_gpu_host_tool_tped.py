"""GPU: garlic-lod --tped through the device reader (garlic_bed_set_rows_tped; opt-in through GARLIC_TPED_DEVICE_READER=1,
because the one load-phase measurement made, profiles/tped_parse_ab.txt, showed it slower than the host reader) against the
same command under GARLIC_TPED_HOST_READER=1: byte-identical file sets.  The host reader is pinned to the reference's
prebuilt binary by tests/golden/e2e."""
import filecmp
import glob
import gzip
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E2E = os.path.join(ROOT, "tests", "golden", "e2e")
TOOL = os.path.join(ROOT, "garlic_amd", "host", "garlic-lod")
COMMON = ["--centromere", os.path.join(E2E, "tiny.centromeres.txt"), "--kde-subsample", "0", "--winsize", "30"]
UNWEIGHTED = ["--raw-lod", "--error", "0.001", "--lod-cutoff", "-12", "--size-bounds", "50000", "200000"]
WEIGHTED = ["--raw-lod", "--error", "0.001", "--weighted", "--phased", "--map", os.path.join(E2E, "tiny.map"), "--ld-subsample", "11",
            "--ld-seed", "5", "--lod-cutoff", "-4", "--size-bounds", "50000", "200000"]
MODES = {
    "unweighted": UNWEIGHTED,
    "weighted_phased": WEIGHTED,
    "tgls": ["--raw-lod", "--tgls", os.path.join(E2E, "tiny.tgls.gz"), "--gl-type", "GQ", "--lod-cutoff", "-11", "--size-bounds", "50000", "200000"],
    "kde_nclust": ["--error", "0.001", "--kde", "--nclust", "3"],
    "resample": UNWEIGHTED + ["--resample", "50", "--resample-seed", "7"],
    "two_shards": WEIGHTED + ["--devices", "0,0"],
}
NIND = 24


@pytest.fixture(scope="module")
def tped(tmp_path_factory):
    """6,000 SNPs x 24 individuals on the chromosomes and positions of the e2e fixture: all-missing lines, monomorphic lines,
    lines that begin with missing and with half-missing genotypes (among them `0 x` in front of a complete genotype of the
    other allele), third alleles, lines that end in \\r\\n and lines with double blanks"""
    d = tmp_path_factory.mktemp("tped")
    leads = []
    with gzip.open(os.path.join(E2E, "tiny.tped.gz"), "rt") as f:
        for line in f:
            t = line.split(None, 4)
            leads.append(t[:4])
    n = len(leads)
    rng = np.random.default_rng(2026)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    a = letters[rng.integers(0, 4, size=n)]
    b = letters[(np.searchsorted(letters, a) + rng.integers(1, 4, size=n)) % 4]
    p = rng.uniform(0.05, 0.95, size=(n, 1))
    al = np.where(rng.random((n, 2 * NIND)) < p, a[:, None], b[:, None]).astype(np.uint8)
    miss = rng.random((n, NIND)) < 0.03
    al[:, 0::2][miss] = ord("0")
    al[:, 1::2][miss] = ord("0")
    half = rng.random((n, 2 * NIND)) < 0.01                  # half-missing genotypes, either side
    al[half] = ord("0")
    third = rng.random((n, 2 * NIND)) < 0.004
    al[third] = letters[rng.integers(0, 4, size=int(third.sum()))]
    al[::211] = ord("0")                                     # all missing
    al[5::307] = a[5::307, None]                             # monomorphic
    al[13::97, :10] = ord("0")                               # begins with missing genotypes
    al[17::53, 0] = ord("0")                                 # `0 x` first, then a complete genotype of the other allele
    al[17::53, 1] = a[17::53]
    al[17::53, 2:4] = b[17::53, None]
    al[29::61, :6] = ord("0")
    al[29::61, 6] = b[29::61]
    al[29::61, 7] = ord("0")                                 # `x 0` behind three missing genotypes
    al[0] = ord("0")
    lines = []
    for r in range(n):
        sep = b"  " if r % 7 == 3 else b"\t" if r % 7 == 5 else b" "
        nl = b"\r\n" if r % 5 == 2 else b"\n"
        lines.append(sep.join([x.encode() for x in leads[r]] + [bytes([v]) for v in al[r]]) + nl)
    path = str(d / "X.tped")
    open(path, "wb").write(b"".join(lines))
    with gzip.open(path + ".gz", "wb") as g:
        g.write(b"".join(lines))
    with open(str(d / "X.tfam"), "w") as f:
        f.write("".join("POP ind%d 0 0 0 -9\n" % i for i in range(NIND)))
    glued = list(lines)
    k = 1234
    t = glued[k].split()
    t[4 + 9] = t[4 + 9] + b"A"                                # one glued `xA`: the line keeps its column count
    glued[k] = b" ".join(t) + b"\n"
    open(str(d / "glued.tped"), "wb").write(b"".join(glued))
    return str(d / "X"), str(d / "glued.tped"), k + 1


def run(tmp, tped_path, tfam, *extra, host_reader=False):
    tmp.mkdir(exist_ok=True)
    out = str(tmp / "mine")
    env = dict(os.environ)
    env.pop("GARLIC_TPED_HOST_READER", None)
    env["GARLIC_TPED_DEVICE_READER"] = "1"
    if host_reader:
        env["GARLIC_TPED_HOST_READER"] = "1"
    r = subprocess.run([TOOL, "--tped", tped_path, "--tfam", tfam, "--out", out, *COMMON, *extra], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    return out, r.stderr


def same_files(a, b):
    names = sorted(os.path.basename(p)[len("mine"):] for p in glob.glob(a + "*"))
    assert names == sorted(os.path.basename(p)[len("mine"):] for p in glob.glob(b + "*"))
    assert ".freq.gz" in names and ".roh.bed" in names and len(names) >= 3, names
    for n in names:
        assert os.path.getsize(a + n) > 0, n
        assert filecmp.cmp(a + n, b + n, shallow=False), n


@pytest.mark.parametrize("mode", sorted(MODES))
def test_device_reader_equals_host_reader(tmp_path, tped, mode):
    prefix, _, _ = tped
    a, err = run(tmp_path / "device", prefix + ".tped", prefix + ".tfam", *MODES[mode])
    assert "TPED device reader" not in err and "TPED parsed on device" in err
    b, err = run(tmp_path / "host", prefix + ".tped", prefix + ".tfam", *MODES[mode], host_reader=True)
    assert "TPED parsed on device" not in err
    same_files(a, b)


def test_gz(tmp_path, tped):
    prefix, _, _ = tped
    a, err = run(tmp_path / "device", prefix + ".tped.gz", prefix + ".tfam", *MODES["weighted_phased"])
    assert "TPED device reader" not in err
    b, _ = run(tmp_path / "host", prefix + ".tped.gz", prefix + ".tfam", *MODES["weighted_phased"], host_reader=True)
    same_files(a, b)
    c, _ = run(tmp_path / "plain", prefix + ".tped", prefix + ".tfam", *MODES["weighted_phased"])
    same_files(a, c)


def test_cache_written_from_the_device_reader_loads_to_the_same_outputs(tmp_path, tped):
    prefix, _, _ = tped
    cache = str(tmp_path / "X.g2b")
    a, _ = run(tmp_path / "first", prefix + ".tped", prefix + ".tfam", *MODES["weighted_phased"], "--genotype-cache", cache)
    assert os.path.getsize(cache) > 0
    b, err = run(tmp_path / "cached", prefix + ".tped", prefix + ".tfam", *MODES["weighted_phased"], "--genotype-cache", cache)
    assert "Loaded genotype cache" in err
    same_files(a, b)


def test_a_refused_line_sends_the_file_to_the_host_reader(tmp_path, tped):
    prefix, glued, line = tped
    a, err = run(tmp_path / "device", glued, prefix + ".tfam", *MODES["unweighted"])
    notes = [ln for ln in err.splitlines() if ln.startswith("TPED device reader")]
    assert len(notes) == 1 and "line %d of" % line in notes[0] and "code 1" in notes[0] and "host reader" in notes[0], err[-1000:]
    b, err = run(tmp_path / "host", glued, prefix + ".tfam", *MODES["unweighted"], host_reader=True)
    assert "TPED device reader" not in err
    same_files(a, b)
