"""GPU: garlic-lod --vcf on a BGZF file through the device path (GARLIC_BGZF_DEVICE_INFLATE=1: blocks inflated and lines cut on
the device, host/bgzf_slabs.hpp) against the run on the plain text and the run with GARLIC_BGZF_HOST_INFLATE=1, every output
file byte for byte.  The VCF is the one tests/test_gpu_host_tool_vcf.py builds, written with three block sizes; every size runs
once with the 64 MB slab and once with slabs of 200,000 bytes, so that tails are carried from slab to slab."""
import os
import subprocess
import zlib

import pytest

import bgzf_cases as bc
import test_gpu_host_tool_vcf as hv
import test_gpu_host_tool_vcf_gl as hg

pytestmark = pytest.mark.gpu
twin = hv.twin
MARKER = "blocks inflated on the device"
NOTE = "read again by the host reader"
RUNS = {"phased": (False, hv.MODES["weighted_phased"]), "gq": (True, [*hg.MODES["unweighted"], "--vcf-gl-field", "GQ", "--gl-type", "GQ"])}
SIZES = {"65280": 65280, "1000": 1000, "bytes": lambda at: 1 if at < 200 else 65280}


@pytest.fixture(scope="module")
def texts(twin, tmp_path_factory):
    """{with GQ?: path of the plain .vcf}"""
    return {False: twin + ".vcf", True: hg.with_likelihoods(twin, str(tmp_path_factory.mktemp("bgzfgl") / "G")) + ".vcf"}


def tool(tmp, vcf, args, **env):
    """-> (out prefix, stderr)"""
    tmp.mkdir(exist_ok=True)
    out = str(tmp / "mine")
    r = subprocess.run([hv.TOOL, "--vcf", vcf, "--out", out, *hv.COMMON, *args], capture_output=True, text=True, env={**os.environ, **env})
    assert r.returncode == 0, r.stderr[-2000:]
    return out, r.stderr


@pytest.fixture(scope="module")
def plain_runs(texts, tmp_path_factory):
    d = tmp_path_factory.mktemp("bgzfplain")
    return {name: tool(d / name, texts[gq], args)[0] for name, (gq, args) in RUNS.items()}


@pytest.mark.parametrize("size", sorted(SIZES))
@pytest.mark.parametrize("name", sorted(RUNS))
def test_device_path_writes_the_files_of_the_plain_text(tmp_path, texts, plain_runs, name, size):
    gq, args = RUNS[name]
    data = open(texts[gq], "rb").read()
    path = str(tmp_path / "X.vcf.gz")
    blob = bc.write_bgzf(data, SIZES[size])
    open(path, "wb").write(blob)
    nblocks = len(bc.split(blob))
    a, err = tool(tmp_path / "device", path, args, GARLIC_BGZF_DEVICE_INFLATE="1")
    assert "X.vcf.gz: BGZF, %d %s" % (nblocks, MARKER) in err, err[-800:]
    hv.same_files(a, plain_runs[name])
    b, err = tool(tmp_path / "small", path, args, GARLIC_BGZF_DEVICE_INFLATE="1", GARLIC_BGZF_SLAB_BYTES="200000")
    assert MARKER in err and NOTE not in err, err[-800:]
    hv.same_files(b, plain_runs[name])
    c, err = tool(tmp_path / "host", path, args, GARLIC_BGZF_DEVICE_INFLATE="1", GARLIC_BGZF_HOST_INFLATE="1")
    assert MARKER not in err
    hv.same_files(c, plain_runs[name])
    if size == "65280":
        d, err = tool(tmp_path / "plain", texts[gq], args, GARLIC_BGZF_DEVICE_INFLATE="1")
        assert MARKER not in err and NOTE not in err
        hv.same_files(d, plain_runs[name])


@pytest.mark.parametrize("name", sorted(RUNS))
def test_broken_files_go_through_the_host_reader_with_a_note(tmp_path, texts, plain_runs, name):
    gq, args = RUNS[name]
    data = open(texts[gq], "rb").read()
    members = bc.split(bc.write_bgzf(data, 65280))
    assert len(members) > 4
    # the third block's CRC is wrong: the host reader refuses the file as well, so what is checked is the note and the refusal
    bad = members[2][:-8] + bytes([members[2][-8] ^ 1]) + members[2][-7:]
    path = str(tmp_path / "crc.vcf.gz")
    open(path, "wb").write(b"".join(members[:2] + [bad] + members[3:]))
    r = subprocess.run([hv.TOOL, "--vcf", path, "--out", str(tmp_path / "crc"), *hv.COMMON, *args], capture_output=True, text=True,
                       env={**os.environ, "GARLIC_BGZF_DEVICE_INFLATE": "1"})
    assert NOTE in r.stderr and "block 2" in r.stderr and MARKER not in r.stderr, r.stderr[-800:]
    h = subprocess.run([hv.TOOL, "--vcf", path, "--out", str(tmp_path / "crch"), *hv.COMMON, *args], capture_output=True, text=True)
    assert (r.returncode == 0) == (h.returncode == 0)
    # BGZF and then one plain gzip member: the same text, the same files
    cut = sum(len(m) for m in members[:3])
    head = sum(bc.isize_of(m) for m in members[:3])
    gz = zlib.compressobj(6, zlib.DEFLATED, 31)
    path = str(tmp_path / "mixed.vcf.gz")
    open(path, "wb").write(b"".join(members[:3]) + gz.compress(data[head:]) + gz.flush())
    assert cut > 0
    a, err = tool(tmp_path / "mixed", path, args, GARLIC_BGZF_DEVICE_INFLATE="1")
    assert NOTE in err and MARKER not in err, err[-800:]
    hv.same_files(a, plain_runs[name])
