"""GPU: garlic-lod --tgls with and without --tgls-term-gb: every output file identical.

The tool fixture (tests/golden/e2e) has 24 individuals: one 64-individual block and, in the whole term matrix, a pad
block; a budget of one block forces the matrix into one slab.  The same fixture with every individual repeated nine
times (216 individuals, four blocks; written by the test) runs several slabs through the two buffers.  The tool says on
stderr what its last call did."""
import filecmp
import gzip
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E2E = os.path.join(ROOT, "tests", "golden", "e2e")
TOOL = os.path.join(ROOT, "garlic_amd", "host", "garlic-lod")
ROWS_PAD = 32 + 4160                   # the pad rows of a block of the term matrix (include/garlic_hip.h)
with gzip.open(os.path.join(E2E, "tiny.tped.gz"), "rt") as _f:
    NLOCI = sum(1 for _ in _f)         # SNPs of the fixture before the tool's monomorphic filter
FLAGS = ["--winsize", "30", "--gl-type", "GQ", "--raw-lod", "--kde-subsample", "0", "--lod-cutoff", "-11",
         "--size-bounds", "50000", "200000"]


def run(tmp_path, name, tped, tfam, tgls, *extra):
    out_dir = tmp_path / name
    out_dir.mkdir()
    cmd = [TOOL, "--tped", tped, "--tfam", tfam, "--tgls", tgls, "--centromere", os.path.join(E2E, "tiny.centromeres.txt"),
           "--out", str(out_dir / "o")] + FLAGS + list(extra)
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return str(out_dir), r.stderr


def assert_same_files(a, b):
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and len(names) >= 5, names      # .freq, .roh.bed, a .raw.lod.windows.gz per chromosome, feeds
    assert any(n.endswith(".roh.bed") for n in names) and any("raw.lod" in n for n in names)
    for n in names:
        if n.endswith(".gz"):
            assert gzip.open(os.path.join(a, n), "rb").read() == gzip.open(os.path.join(b, n), "rb").read(), n
        else:
            assert filecmp.cmp(os.path.join(a, n), os.path.join(b, n), shallow=False), n
        assert os.path.getsize(os.path.join(a, n)) > 0, n


def block_gb(nloci):
    """a block of the term matrix of a panel of this many SNPs, in the flag's unit"""
    return (ROWS_PAD + nloci) * 512 / 1e9


def test_fixture_with_and_without_the_flag(tmp_path):
    src = [os.path.join(E2E, n) for n in ("tiny.tped.gz", "tiny.tfam", "tiny.tgls.gz")]
    plain, _ = run(tmp_path, "plain", *src)
    # the monomorphic filter may drop SNPs: a block of the unfiltered panel holds a block of the kept one and is less than
    # the two blocks of its whole matrix (4192 pad rows each)
    slabs, err = run(tmp_path, "flag", *src, "--tgls-term-gb", "%.9f" % (block_gb(NLOCI) + 1e-9))
    assert_same_files(plain, slabs)
    assert re.search(r"TGLS terms .*: last call in 1 slabs of 1 blocks", err), err[-500:]


def test_four_blocks_forced_into_slabs(tmp_path):
    rep = 9
    tped, tfam, tgls = (str(tmp_path / n) for n in ("big.tped.gz", "big.tfam", "big.tgls.gz"))
    with gzip.open(os.path.join(E2E, "tiny.tped.gz"), "rt") as f, gzip.open(tped, "wt") as g:
        for line in f:
            w = line.split()
            g.write(" ".join(w[:4] + w[4:] * rep) + "\n")
    with gzip.open(os.path.join(E2E, "tiny.tgls.gz"), "rt") as f, gzip.open(tgls, "wt") as g:
        for line in f:
            w = line.split()
            g.write(" ".join(w[:4] + w[4:] * rep) + "\n")
    with open(tfam, "w") as g:
        for k in range(24 * rep):
            g.write("POP ind%d 0 0 0 -9\n" % k)
    plain, _ = run(tmp_path, "plain", tped, tfam, tgls)
    # two blocks of the unfiltered panel: one-block slabs whatever the filter keeps (two-block slabs if it keeps little),
    # less than the five blocks of the whole matrix
    slabs, err = run(tmp_path, "flag", tped, tfam, tgls, "--tgls-term-gb", "%.9f" % (2 * block_gb(NLOCI) + 1e-9))
    m = re.search(r"TGLS terms .*: last call in (\d+) slabs of (\d+) blocks", err)
    assert m and int(m.group(1)) >= 2 and int(m.group(1)) * int(m.group(2)) >= 4, err[-500:]
    assert_same_files(plain, slabs)
