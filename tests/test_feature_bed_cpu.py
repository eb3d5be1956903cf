"""CPU: feature counts from a PLINK .bed -- what is declared (header, history entry, bindings, library, usage text), the row
plan of garlic_amd/host/feature_bed.hpp in a stand-alone program under the sanitizers, the numpy restatement of the hom rows
on hand-made codes, the golden TPED lines as a .bed file set, and garlic-lod --bfile-counting as far as a machine without a
device gets: the files are read, then the library is asked for a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import feature_bed_cases as fb
import feature_cases as fc
from garlic_amd import abi

ROOT = fc.ROOT
TOOL = os.path.join(ROOT, "garlic_amd", "host", "garlic-lod")
NEW = ("garlic_feature_set_rows_bed", "garlic_feature_set_get_rows")


def test_header_bindings_and_library_declare_the_two_calls():
    hdr = open(os.path.join(ROOT, "include", "garlic_hip.h")).read()
    assert re.search(r"^#define GARLIC_HIP_ABI_VERSION 8$", hdr, re.M) and abi.ABI_VERSION == 8
    history = re.search(r"^ \* 8:.*?\*/", hdr, re.M | re.S).group(0)
    lib = C.CDLL(abi.LIB_PATH)
    text = open(os.path.join(ROOT, "garlic_amd", "abi.py")).read()
    for name in NEW:
        assert re.search(r"^int %s\(garlic_feature_set \*set," % name, hdr, re.M), name
        assert re.search(r"\b%s\b" % name, history), (name, "is not in the history of ABI 8")
        assert name in abi.SYMBOLS and hasattr(lib, name), name
        assert "L.%s.argtypes" % name in text, name
    assert re.search(r"garlic_feature_set_rows_bed,\s*\*?\s*garlic_feature_set_get_rows \(likewise\)", history)
    assert abi.lib().garlic_hip_abi_version() == 8
    assert callable(abi.FeatureSet.set_rows_bed) and callable(abi.FeatureSet.get_rows)


def test_restatement_on_hand_made_codes():
    codes = np.array([[0, 1, 2, 3, 0], [3, 3, 1, 0, 2]], dtype=np.uint8)
    hom = fb.hom_rows(codes, [1, 0, 0, 1], [1, 0, 1, 2])
    assert hom.tolist() == [[True, True, False, False, False], [True, False, False, False, True],
                            [False, False, False, True, False], [False] * 5]
    assert fb.hom_rows(codes, [], []).shape == (0, 5)
    for n_out in fb.ROW_COUNTS:
        for name, (file_row, allele) in fb.plans(n_out, fb.IMAGE_ROWS, np.random.default_rng(n_out)).items():
            assert file_row.shape == allele.shape == (n_out,) and (n_out == 0 or (0 <= file_row.min() and file_row.max() < fb.IMAGE_ROWS))
            if n_out > 1:
                assert 0 in file_row and fb.IMAGE_ROWS - 1 in file_row, (n_out, name)
            if n_out > 4:
                assert set(allele.tolist()) == {0, 1, 2}, (n_out, name)
    rep, sel = fb.plans(64, fb.IMAGE_ROWS, np.random.default_rng(0))["repeats"]
    assert rep[0] == rep[1] and (sel[0], sel[1]) == (0, 1)


def test_usage_lists_the_counting_bed_flags():
    r = subprocess.run([TOOL], capture_output=True, text=True)
    assert r.returncode != 0
    for flag in ("--bfile-counting", "--bed-counting", "--bim-counting", "--fam-counting"):
        assert flag in r.stderr, flag
    base = [TOOL, "--roh-bed", "x.roh.bed", "--features", "f"]
    for extra in (["--bfile-counting", "p", "--tped-counting", "t.tped"], ["--bfile-counting", "p", "--tfam-counting", "t.tfam"],
                  ["--bed-counting", "p.bed", "--bim-counting", "p.bim", "--fam-counting", "p.fam", "--tped-counting", "t.tped"]):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        assert r.returncode != 0 and "usage:" in r.stderr and "exclude each other" in r.stderr.split("\n")[0], extra
    r = subprocess.run(base + ["--bed-counting", "p.bed"], capture_output=True, text=True)
    assert r.returncode != 0 and "go together" in r.stderr.split("\n")[0]
    r = subprocess.run(base + ["--bfile-counting", "p", "--bim-counting", "q.bim"], capture_output=True, text=True)
    assert r.returncode != 0 and "exclude each other" in r.stderr.split("\n")[0]
    # no counting input at all: the error it always was
    r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode != 0 and r.stderr.split("\n")[0] == "ERROR: feature counts need --features and --tped-counting"
    # a run that writes no calls: as with --tped-counting
    r = subprocess.run([TOOL, "--tped", "x.tped", "--tfam", "x.tfam", "--build", "hg19", "--error", "0.001", "--winsize", "30",
                        "--features", "f", "--bfile-counting", "p"], capture_output=True, text=True)
    assert r.returncode != 0 and "--features counts inside ROH calls" in r.stderr


def golden_bed(case, d):
    """a golden case's TPED lines as case.bed / .bim / .fam in d"""
    iids = [line.split()[1] for line in open(fc.golden_path(case, "chr22.tfam")).read().splitlines()]
    lines = [line for _c, line in fc.golden_tped_lines(case)]
    return fb.tped_lines_to_bed(lines, os.path.join(str(d), case), iids, three_alleles=fb.THREE_ALLELES if case == "case1" else None)


def test_roh_bed_mode_reads_the_file_set_and_reaches_the_device_library(tmp_path):
    case = "case1"
    prefix = golden_bed(case, tmp_path)
    assert os.path.getsize(prefix + ".bed") == 3 + 10 * 2           # 10 lines x 5 individuals
    out = str(tmp_path / "mine")
    cmd = [TOOL, "--roh-bed", fc.golden_path(case, "roh.bed"), "--features", fc.golden_path(case, "features.txt"), "--out", out]
    r = subprocess.run(cmd + ["--bfile-counting", prefix], capture_output=True, text=True)
    assert "usage:" not in r.stderr
    assert "Feature counts: 10 annotated alleles, 4 effects; 8 of 10 counting loci annotated, 5 individuals" in r.stderr
    if r.returncode == 0:
        assert open(out + ".feature.counts").read() == open(fc.golden_path(case, "expected.counts")).read()
    else:
        assert "garlic_ctx_create: no HIP device available" in r.stderr, r.stderr[-2000:]
        assert not os.path.exists(out + ".feature.counts")
    # a two-character allele: the reader's error, with file and line
    bim = open(prefix + ".bim").read().splitlines()
    f = bim[2].split("\t")
    f[4] = "AT"
    bim[2] = "\t".join(f)
    open(str(tmp_path / "bad.bim"), "w").write("\n".join(bim) + "\n")
    r = subprocess.run(cmd + ["--bed-counting", prefix + ".bed", "--bim-counting", str(tmp_path / "bad.bim"), "--fam-counting", prefix + ".fam"],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "bad.bim:3: allele \"AT\" is not a single character" in r.stderr
    # an individual-major .bed is refused
    data = bytearray(open(prefix + ".bed", "rb").read())
    data[2] = 0
    open(str(tmp_path / "im.bed"), "wb").write(bytes(data))
    r = subprocess.run(cmd + ["--bed-counting", str(tmp_path / "im.bed"), "--bim-counting", prefix + ".bim", "--fam-counting", prefix + ".fam"],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "individual-major" in r.stderr


def test_row_plan_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "feature_bed_unit")
    src = os.path.join(ROOT, "tests", "host_unit", "feature_bed_unit.cpp")
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                         "-fno-omit-frame-pointer", "-o", exe, src, "-lz"], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    run = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout == "feature_bed_unit ok\n", (run.stdout + run.stderr)[-3000:]
