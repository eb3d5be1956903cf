"""CPU: feature counts per ROH class -- the numpy restatement of tests/feature_cases.py reproduces the tables the reference's
count_features_in_roh.pl printed for tests/golden/features; what is declared (header, bindings, library, usage text); the
host readers, interval builders and table writer of garlic_amd/host/feature_counts.hpp in a stand-alone program under the
sanitizers; and garlic-lod --roh-bed, which without a device gets as far as the library's no-device error."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import feature_cases as fc
from garlic_amd import abi

ROOT = fc.ROOT
TOOL = os.path.join(ROOT, "garlic_amd", "host", "garlic-lod")
SCRIPT = "/root/reference/src/count_features_in_roh.pl"
NAMES = ["garlic_feature_set_create", "garlic_feature_set_destroy", "garlic_feature_set_rows", "garlic_feature_set_sites",
         "garlic_feature_counts", "garlic_feature_counts_info"]


def joined_tped(case, d):
    """the per-chromosome files of a golden case as the one file garlic-lod reads, and its TFAM"""
    tped, tfam = os.path.join(str(d), case + ".tped"), os.path.join(str(d), case + ".tfam")
    with open(tped, "w") as f:
        for c in (22, 23):
            f.write(open(fc.golden_path(case, "chr%d.tped" % c)).read())
    shutil.copy(fc.golden_path(case, "chr22.tfam"), tfam)
    return tped, tfam


@pytest.mark.parametrize("case", fc.GOLDEN_CASES)
def test_restatement_reproduces_the_scripts_tables(case):
    want = open(fc.golden_path(case, "expected.counts")).read()
    assert want.split("\n")[0].endswith("NONE ") and fc.golden_table(case) == want


def test_golden_cases_hold_what_they_are_for():
    text = {c: {w: open(fc.golden_path(c, w)).read() for w in ("features.txt", "roh.bed", "chr22.tped", "chr23.tped", "expected.counts")}
            for c in fc.GOLDEN_CASES}
    one = text["case1"]
    assert "chr22:100 A G dam" in one["features.txt"] and "chr22:100 A T ben" in one["features.txt"]      # two alleles at one position
    assert one["features.txt"].index("chr22:200 C T dam") < one["features.txt"].index("chr22:200 C T lof")   # a duplicate key
    assert " 0 0 " in one["chr22.tped"] and " A G " in one["chr22.tped"]                                  # missing, heterozygote
    assert "chr22\t100\t300\tA" in one["roh.bed"] and all(" %d " % p in one["chr22.tped"] for p in (100, 300, 399, 400))   # start, end, end - 1
    assert "Ind: I3 Pop" in one["roh.bed"] and "Ind: I5 Pop" not in one["roh.bed"] and "Ind: Z9 Pop" in one["roh.bed"]
    assert " 250 " in one["chr22.tped"] and "chr22:250" not in one["features.txt"]                         # an unannotated line
    assert text["case2"]["expected.counts"].startswith("LOF_2A LOF_2B LOF_2C LOF_2NONE ZetaA ")           # bytewise order


@pytest.mark.parametrize("case", fc.GOLDEN_CASES)
def test_the_script_still_prints_the_golden_table(case, tmp_path):
    if not (os.path.exists(SCRIPT) and shutil.which("perl")):
        pytest.skip("the reference's script or perl is not on this machine")
    for name in os.listdir(fc.GOLDEN):
        if name.startswith(case + "."):
            shutil.copy(os.path.join(fc.GOLDEN, name), str(tmp_path))
    out = str(tmp_path / "out.counts")
    r = subprocess.run(["perl", SCRIPT, case + ".features.txt", case + ".roh.bed", case + ".chr22.tped", "23", out], cwd=str(tmp_path),
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(out).read() == open(fc.golden_path(case, "expected.counts")).read()


def test_header_bindings_and_library_declare_the_feature_calls():
    hdr = open(os.path.join(ROOT, "include", "garlic_hip.h")).read()
    assert re.search(r"^#define GARLIC_HIP_ABI_VERSION 8$", hdr, re.M)
    assert re.search(r"^#define GARLIC_FEATURE_MAX_EFFECTS %d$" % abi.FEATURE_MAX_EFFECTS, hdr, re.M) and abi.FEATURE_MAX_EFFECTS >= 64
    assert re.search(r"^typedef struct garlic_feature_set garlic_feature_set;$", hdr, re.M)
    assert re.search(r"typedef struct garlic_roh_interval \{\s*int32_t ind, chr, start, stop, cls;\s*\} garlic_roh_interval;", hdr)
    history = re.search(r"^ \* 8:.*?\*/", hdr, re.M | re.S).group(0)
    lib = C.CDLL(abi.LIB_PATH)
    for name in NAMES:
        assert re.search(r"^int %s\(" % name, hdr, re.M), name
        assert re.search(r"\b%s\b" % name, history), (name, "is not in the history of ABI 8")
        assert name in abi.SYMBOLS and hasattr(lib, name), name
    assert abi.lib().garlic_hip_abi_version() == abi.ABI_VERSION == 8
    assert abi.ROH_INTERVAL.itemsize == 20 and abi.ROH_INTERVAL == fc.INTERVAL
    assert (abi.FEATURE_CHUNK_ROWS, abi.FEATURE_GROUP_EFFECTS, abi.FEATURE_MAX_EFFECTS) == (fc.CHUNK, fc.GROUP, fc.CAP)
    kernels = open(os.path.join(ROOT, "garlic_amd", "csrc", "feature_kernels.hpp")).read()
    for name, v in (("FEAT_CHUNK_ROWS", fc.CHUNK), ("FEAT_GROUP_EFFECTS", fc.GROUP), ("FEAT_MAX_EFFECTS", fc.CAP)):
        assert re.search(r"^constexpr int %s = %d;" % (name, v), kernels, re.M), name
    for a in ("set_rows", "set_sites", "counts", "counts_device", "info", "close", "__enter__", "__exit__"):
        assert callable(getattr(abi.FeatureSet, a)), a


def test_usage_lists_the_feature_flags():
    r = subprocess.run([TOOL], capture_output=True, text=True)
    assert r.returncode != 0
    for flag in ("--features", "--tped-counting", "--tfam-counting", "--roh-bed"):
        assert flag in r.stderr, flag
    assert "A .. <last letter> NONE" in r.stderr, "the class extension is documented in the usage text"
    # neither calls to count in, nor a run that makes them
    r = subprocess.run([TOOL, "--tped", "x.tped", "--tfam", "x.tfam", "--build", "hg19", "--error", "0.001", "--winsize", "30",
                        "--features", "f", "--tped-counting", "t.tped"], capture_output=True, text=True)
    assert r.returncode != 0 and "--features counts inside ROH calls" in r.stderr
    r = subprocess.run([TOOL, "--roh-bed", "x.roh.bed", "--features", "f"], capture_output=True, text=True)
    assert r.returncode != 0 and "need --features and --tped-counting" in r.stderr


def test_roh_bed_mode_reaches_the_device_library(tmp_path):
    """no parse error and no usage error: the inputs are read, then the library is asked for a device.  Where there is one the
    table is the script's (tests/test_gpu_host_tool_features.py checks that on the GPU machine)."""
    case = "case1"
    tped, _ = joined_tped(case, tmp_path)
    out = str(tmp_path / "mine")
    r = subprocess.run([TOOL, "--roh-bed", fc.golden_path(case, "roh.bed"), "--features", fc.golden_path(case, "features.txt"),
                        "--tped-counting", tped, "--out", out], capture_output=True, text=True)
    assert "usage:" not in r.stderr
    assert "Feature counts: 10 annotated alleles, 4 effects; 8 of 10 counting loci annotated, 5 individuals" in r.stderr
    if r.returncode == 0:
        assert open(out + ".feature.counts").read() == open(fc.golden_path(case, "expected.counts")).read()
    else:
        assert "garlic_ctx_create: no HIP device available" in r.stderr, r.stderr[-2000:]
        assert not os.path.exists(out + ".feature.counts")
    # a malformed feature line is the reader's error, with file and line
    bad = str(tmp_path / "bad.features")
    open(bad, "w").write("chr22:100 A G dam\nchr22 200 C T dam\n")
    r = subprocess.run([TOOL, "--roh-bed", fc.golden_path(case, "roh.bed"), "--features", bad, "--tped-counting", tped, "--out", out],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "bad.features:2: no colon" in r.stderr


@pytest.fixture(scope="module")
def unit_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("feature_counts_unit") / "feature_counts_unit")
    src = os.path.join(ROOT, "tests", "host_unit", "feature_counts_unit.cpp")
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                         "-fno-omit-frame-pointer", "-o", exe, src, "-lz"], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    return exe


def test_host_readers_builders_and_writer_under_the_sanitizers(unit_exe, tmp_path):
    args = []
    for case in fc.GOLDEN_CASES:
        tped, tfam = joined_tped(case, tmp_path)
        args += [fc.golden_path(case, "features.txt"), tped, tfam, fc.golden_path(case, "roh.bed"), fc.golden_path(case, "expected.counts")]
    run = subprocess.run([unit_exe, str(tmp_path)] + args, capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.endswith("feature_counts_unit ok\n"), (run.stdout + run.stderr)[-3000:]
    assert run.stdout.count("\n") == len(fc.GOLDEN_CASES) + 1
