"""GPU: garlic-lod --weighted --tgls with and without --tgls-term-gb: every output file identical, the .roh.bed among them,
and the tool's log says that its last call -- a weighted one -- ran in slabs.

The tool fixture (tests/golden/e2e) with every individual repeated nine times (216 individuals, four blocks; written by the
test, as tests/test_gpu_host_tool_slabs.py does) under the smallest budget there is: the buffers of one-block slabs."""
import gzip
import os
import re
import subprocess

import pytest

from test_gpu_host_tool_slabs import E2E, NLOCI, TOOL, assert_same_files, block_gb

pytestmark = pytest.mark.gpu
FLAGS = ["--winsize", "30", "--gl-type", "GQ", "--raw-lod", "--kde-subsample", "0", "--weighted", "--map", os.path.join(E2E, "tiny.map"),
         "--ld-subsample", "0", "--lod-cutoff", "-4", "--size-bounds", "50000", "200000"]


def run(tmp_path, name, tped, tfam, tgls, *extra):
    out_dir = tmp_path / name
    out_dir.mkdir()
    cmd = [TOOL, "--tped", tped, "--tfam", tfam, "--tgls", tgls, "--centromere", os.path.join(E2E, "tiny.centromeres.txt"),
           "--out", str(out_dir / "o")] + FLAGS + list(extra)
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return str(out_dir), r.stderr


def test_weighted_tgls_four_blocks_in_slabs(tmp_path):
    rep = 9
    tped, tfam, tgls = (str(tmp_path / n) for n in ("big.tped.gz", "big.tfam", "big.tgls.gz"))
    for src, dst in (("tiny.tped.gz", tped), ("tiny.tgls.gz", tgls)):
        with gzip.open(os.path.join(E2E, src), "rt") as f, gzip.open(dst, "wt") as g:
            for line in f:
                w = line.split()
                g.write(" ".join(w[:4] + w[4:] * rep) + "\n")
    with open(tfam, "w") as g:
        for k in range(24 * rep):
            g.write("POP ind%d 0 0 0 -9\n" % k)
    plain, _ = run(tmp_path, "plain", tped, tfam, tgls)
    # two blocks of the unfiltered panel: one-block slabs whatever the monomorphic filter keeps (two-block slabs if it keeps
    # little), less than the five blocks of the whole matrix
    slabs, err = run(tmp_path, "flag", tped, tfam, tgls, "--tgls-term-gb", "%.9f" % (2 * block_gb(NLOCI) + 1e-9))
    m = re.search(r"TGLS terms .*: last call in (\d+) slabs of (\d+) blocks", err)
    assert m and int(m.group(1)) >= 2 and int(m.group(1)) * int(m.group(2)) >= 4, err[-500:]
    assert_same_files(plain, slabs)
    bed = [n for n in os.listdir(slabs) if n.endswith(".roh.bed")]
    assert len(bed) == 1 and sum(1 for line in open(os.path.join(slabs, bed[0])) if not line.startswith("track")) > 0
