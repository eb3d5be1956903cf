"""GPU: garlic-lod --weighted --winsize-multi computes the LD weights of all sizes once (LodEngine::ldWeightsMulti) and
writes byte-identical files to a run under GARLIC_LD_MULTI_SOLO=1, where every size has an LD pass of its own -- feeds,
.roh.bed and raw LOD files, on one device and with the individuals sharded."""
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
COMMON = ["--weighted", "--winsize-multi", "40", "60", "--map", os.path.join(E2E, "tiny.map"), "--ld-subsample", "11", "--ld-seed", "5",
          "--kde-subsample", "0", "--error", "0.001"]


def run(tmp_path, name, *extra, solo=False):
    out_dir = tmp_path / name
    out_dir.mkdir()
    cmd = [TOOL, "--tped", os.path.join(E2E, "tiny.tped.gz"), "--tfam", os.path.join(E2E, "tiny.tfam"),
           "--centromere", os.path.join(E2E, "tiny.centromeres.txt"), "--out", str(out_dir / "o")] + COMMON + list(extra)
    env = dict(os.environ)
    env.pop("GARLIC_LD_MULTI_SOLO", None)
    if solo:
        env["GARLIC_LD_MULTI_SOLO"] = "1"
    r = subprocess.run(cmd, capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    return str(out_dir), r.stderr


def assert_same_files(a, b, suffixes):
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)), (names, sorted(os.listdir(b)))
    for s in suffixes:
        assert any(n.endswith(s) for n in names), (s, names)
    for n in names:
        if n.endswith(".gz"):
            assert gzip.open(os.path.join(a, n), "rb").read() == gzip.open(os.path.join(b, n), "rb").read(), n
        else:
            assert filecmp.cmp(os.path.join(a, n), os.path.join(b, n), shallow=False), n
        assert os.path.getsize(os.path.join(a, n)) > 0, n


def one_computation(err):
    return len(re.findall(r"Calculating LD weights", err)) == 1 and \
        re.search(r"Calculating LD weights with winsizes 40 60 \(one LD computation for 2 window sizes\)", err)


def test_feeds(tmp_path):
    shared, err = run(tmp_path, "shared")
    assert one_computation(err), err[-1000:]
    solo, err_solo = run(tmp_path, "solo", solo=True)
    assert one_computation(err_solo)              # the same call; the library runs one pass per size inside it
    assert_same_files(shared, solo, ["40SNPs.lod.f64", "60SNPs.lod.f64"])


def test_raw_lod_and_roh_calls(tmp_path):
    extra = ["--raw-lod", "--lod-cutoff", "-4", "--size-bounds", "50000", "200000"]
    shared, err = run(tmp_path, "shared", *extra)
    assert one_computation(err), err[-1000:]
    solo, _ = run(tmp_path, "solo", *extra, solo=True)
    assert_same_files(shared, solo, ["40SNPs.lod.f64", "60SNPs.lod.f64", "40SNPs.roh.bed", "60SNPs.roh.bed", ".gz"])


def test_sharded(tmp_path):
    """two shards (both on device 0): counts at the largest size, summed on the host, finished on every shard"""
    one, _ = run(tmp_path, "one")
    two, err = run(tmp_path, "two", "--devices", "0,0")
    assert one_computation(err), err[-1000:]
    assert_same_files(one, two, ["40SNPs.lod.f64", "60SNPs.lod.f64"])
