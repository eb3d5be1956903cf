"""CPU: the numpy restatement of the VCF door (tests/vcf_cases.py) against the reference's own converter and TPED loop on the
golden case, the synth twin writer against the same converter's output, and garlic_amd/host/vcf_lines.hpp as a stand-alone
program under ASan + UBSan."""
import os
import subprocess

import numpy as np

import vcf_cases as vc
from garlic_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "vcf")


def golden_case():
    text = open(os.path.join(GOLDEN, "case1.vcf"), "rb").read()
    begins, at = [], 0
    for ln in text.splitlines(keepends=True):
        if not ln.startswith(b"#"):
            begins.append(at)
        at += len(ln)
    header = [ln for ln in text.split(b"\n") if ln.startswith(b"#CHROM")][0]
    nind = len(header.split(b"\t")) - 9
    tped = open(os.path.join(GOLDEN, "case1.tped")).read().splitlines()
    return text, np.array(begins + [len(text)], dtype=np.int64), nind, tped


def test_restatement_equals_the_tped_read_of_the_converters_output():
    """case1.vcf through vcf_cases == case1.tped (written by vcf2tped.pl) through the reference's TPED loop: genotypes as copies
    of the counted allele, the counted allele's letter, nalleles, total, and firstCopy.  firstCopy is compared at every
    non-missing genotype and on the rows without a counted allele (all ones); the reference's loop leaves `true` at a missing
    genotype in front of the row's first allele and `false` at one behind it, which nothing reads (the reference's r2,
    src/garlic-data.cpp:596, passes over a pair unless both genotypes are != -9, and firstCopy is read nowhere else), and
    the door defines both as false."""
    text, lb, nind, tped = golden_case()
    assert nind == 7 and len(tped) == len(lb) - 1 == 30
    _, _, status, codes, order = vc.parse_slab(text, lb, nind)
    assert not status.any()
    counts, counted = vc.census(codes, order)
    geno = vc.recode(codes, counted)
    fc = vc.first_copy(codes, order, counted)
    kinds = set()
    for r, line in enumerate(tped):
        cols = text[lb[r]:lb[r + 1]].split(b"\t")
        ref, alt = cols[3].decode(), cols[4].decode()
        one, data, ref_fc, nalleles, total = vc.tped_read(line)
        assert one == {0: ref, 1: alt, 2: "0"}[int(counted[r])], r
        assert np.array_equal(geno[r], data), r
        assert (counts[r, 0], counts[r, 1]) == (nalleles, total), r
        live = data != -9
        assert np.array_equal(fc[r][live], ref_fc[live]), r
        if counted[r] == 2:
            assert fc[r].all() and ref_fc.all(), r
        nm = np.flatnonzero(codes[r] != vc.MISS)
        first = (int(codes[r, nm[0]]), int(order[r, nm[0]]), bool(nm[0] > 0)) if nm.size else None
        kinds.add(first)
    # the case holds what it is there for: rows that begin with 1|0, with ./. then 1|0, all-missing rows, both monomorphic kinds
    assert (2, 1, False) in kinds and (2, 1, True) in kinds and (2, 0, False) in kinds and None in kinds
    assert any((codes[r] == 0).all() for r in range(30)) and any((codes[r] == 3).all() for r in range(30))
    # and a row on which the .bed rule (a het reads "A1 A2") would count the other allele
    _, bed_counted = vc.census(codes)
    assert (bed_counted != counted).any()


def test_synth_twin_is_what_the_converter_writes(tmp_path):
    """synth.write_vcf_and_tped from the golden case's genotypes reproduces case1.tped and case1.tfam byte for byte, and its VCF
    parses back to the same codes and order bits"""
    text, lb, nind, _ = golden_case()
    _, _, _, codes, order = vc.parse_slab(text, lb, nind)
    cols = [text[lb[r]:lb[r + 1]].split(b"\t") for r in range(30)]
    prefix = str(tmp_path / "twin")
    synth.write_vcf_and_tped(prefix, codes, order, [c[0].decode() for c in cols], [int(c[1]) for c in cols],
                             a1=[c[3].decode() for c in cols], a2=[c[4].decode() for c in cols],
                             names=[c[2].decode() for c in cols], samples=["S%d" % (i + 1) for i in range(7)],
                             extra_subfields=lambda r, j: "9,%d" % j if r % 3 == 0 else "")
    for ext in (".tped", ".tfam"):
        assert open(prefix + ext, "rb").read() == open(os.path.join(GOLDEN, "case1" + ext), "rb").read(), ext
    twin = open(prefix + ".vcf", "rb").read()
    begins, at = [], 0
    for ln in twin.splitlines(keepends=True):
        if not ln.startswith(b"#"):
            begins.append(at)
        at += len(ln)
    _, _, status, codes2, order2 = vc.parse_slab(twin, np.array(begins + [len(twin)]), nind)
    assert not status.any() and np.array_equal(codes2, codes) and np.array_equal(order2, order)


def test_restatement_on_its_own_offences():
    """the numpy model against expectations written by hand (it passes without the library: it guards the model the GPU tests
    compare with; where two offence codes border on each other -- `12/0`, `0|10` an allele index, a NUL a bad byte -- the model
    states the header's rule, as the kernel does)"""
    rng = np.random.default_rng(5)
    codes, order = vc.random_genotypes(rng, 3, 5)
    lines = vc.make_lines(rng, codes, order)
    for name, col, code in vc.OFFENCES:
        parts = lines[1].rstrip(b"\n").split(b"\t")
        parts[9 + 2] = col
        assert vc.parse_line(b"\t".join(parts) + b"\n", 5)[2] == (code, 2), name
    assert vc.parse_line(lines[0], 6)[2] == (vc.FEW_COLUMNS, 5)
    assert vc.parse_line(lines[0], 4)[2] == (vc.MANY_COLUMNS, 4)
    assert vc.parse_line(b"1\t2\n", 4)[2] == (vc.FEW_COLUMNS, 0)
    got = vc.parse_line(lines[2], 5)
    assert got[2] == (0, 0) and np.array_equal(got[0], codes[2]) and np.array_equal(got[1], order[2])


def test_vcf_lines_unit_under_sanitizers(tmp_path):
    """tests/host_unit/vcf_lines_unit.cpp, compiled here with ASan + UBSan: a stand-alone program, nothing loaded into python"""
    exe = str(tmp_path / "vcf_lines_unit")
    src = os.path.join(ROOT, "tests", "host_unit", "vcf_lines_unit.cpp")
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                         "-o", exe, src, "-lz"], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "vcf_lines_unit ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
