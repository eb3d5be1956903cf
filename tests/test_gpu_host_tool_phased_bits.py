"""GPU: garlic-lod --weighted --phased from the genotype cache, whose firstCopy rows now reach the device as bit rows
(garlic_panel_set_phase_bits), against the same run from the TPED (one byte per genotype, garlic_panel_set_phase): the same
files, byte for byte -- and the raw windows against those the reference's prebuilt binary wrote (tests/golden/e2e/refp.*)."""
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
WEIGHTED = ["--winsize", "30", "--weighted", "--phased", "--map", os.path.join(E2E, "tiny.map"), "--ld-subsample", "0"]


def run_tool(outdir, *extra):
    outdir.mkdir()
    out = str(outdir / "mine")
    cmd = [TOOL, "--tped", os.path.join(E2E, "tiny.tped.gz"), "--tfam", os.path.join(E2E, "tiny.tfam"),
           "--centromere", os.path.join(E2E, "tiny.centromeres.txt"), "--error", "0.001", "--out", out, "--kde-subsample", "0"]
    r = subprocess.run(cmd + list(extra), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out, r.stderr


def outputs(out):
    return sorted(os.path.basename(p)[len("mine"):] for p in glob.glob(out + "*"))


def read_rows(path):
    with gzip.open(path, "rt") as f:
        return [line.split() for line in f]


@pytest.mark.parametrize("devices", ["0", "0,0,0"])
@pytest.mark.parametrize("what,flags,suffix", [("raw windows", ["--raw-lod"], ".raw.lod.windows.gz"),
                                               ("segments", ["--cm", "--lod-cutoff", "-4", "--size-bounds", "0.05", "0.2"], ".roh.bed")])
def test_cache_run_writes_the_tped_runs_files(tmp_path, what, flags, suffix, devices):
    """TPED run; a run that writes the cache; a run that loads it (packed genotypes, packed phase) -- on one device and on
    three shards of 8 individuals (24 individuals: every shard begins on a byte of the phase rows)"""
    cache = str(tmp_path / "tiny.g2b")
    tped, _ = run_tool(tmp_path / "tped", *WEIGHTED, *flags, "--devices", devices)
    run_tool(tmp_path / "write", *WEIGHTED, *flags, "--devices", devices, "--genotype-cache", cache)
    cached, log = run_tool(tmp_path / "load", *WEIGHTED, *flags, "--devices", devices, "--genotype-cache", cache)
    assert "Loaded genotype cache" in log
    names = outputs(tped)
    assert names == outputs(cached) and any(n.endswith(suffix) for n in names), names
    for n in names:
        assert filecmp.cmp(tped + n, cached + n, shallow=False), (what, n)


def test_uneven_shards_take_the_shifted_rows(tmp_path):
    """five shards of 5, 5, 5, 5 and 4 individuals: four of them begin inside a byte of the phase rows"""
    cache = str(tmp_path / "tiny.g2b")
    flags = [*WEIGHTED, "--raw-lod", "--devices", "0,0,0,0,0"]
    tped, _ = run_tool(tmp_path / "tped", *flags)
    run_tool(tmp_path / "write", *flags, "--genotype-cache", cache)
    cached, _ = run_tool(tmp_path / "load", *flags, "--genotype-cache", cache)
    names = outputs(tped)
    assert any(n.endswith(".raw.lod.windows.gz") for n in names)
    for n in names:
        assert filecmp.cmp(tped + n, cached + n, shallow=False), n


def test_cache_run_matches_reference_binary(tmp_path):
    """the raw windows of the cached --phased run against the prebuilt reference's (6 printed digits; its own, older libm)"""
    cache = str(tmp_path / "tiny.g2b")
    flags = ["--winsize", "30", "--raw-lod", "--weighted", "--phased", "--map", os.path.join(E2E, "tiny.map")]
    run_tool(tmp_path / "write", *flags, "--genotype-cache", cache)
    out, _ = run_tool(tmp_path / "load", *flags, "--genotype-cache", cache)
    n_tok = n_same = 0
    refs = sorted(glob.glob(os.path.join(E2E, "refp.POP.*.raw.lod.windows.gz")))
    assert len(refs) == 3
    for ref in refs:
        a, b = read_rows(ref), read_rows(out + os.path.basename(ref)[4:])
        assert len(a) == len(b) == 24
        for ra, rb in zip(a, b):
            assert len(ra) == len(rb)
            assert [x == "NA" for x in ra] == [x == "NA" for x in rb]
            va = np.array([float(x) for x in ra if x != "NA"])
            vb = np.array([float(x) for x in rb if x != "NA"])
            assert np.allclose(va, vb, rtol=2e-5, atol=2e-6)
            n_tok += len(ra)
            n_same += sum(x == y for x, y in zip(ra, rb))
    assert n_tok > 100000 and n_same / n_tok > 0.999, (n_same, n_tok)
