"""CPU: the Python restatement of the TPED door (tests/tped_cases.py) against the twins that garlic_amd.synth writes next to a
.bed and next to a VCF -- on files with neither a half-missing genotype nor a third allele it must agree with the census
rule the images already follow --, against hand-written half-missing and third-allele lines, on its own offences, and
garlic_amd/host/tped_lines.hpp as a stand-alone program under ASan + UBSan."""
import gzip
import os
import subprocess

import numpy as np

import tped_cases as tc
import vcf_cases as vc
from garlic_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def parsed_file(path, nind):
    text = open(path, "rb").read()
    lines = text.splitlines(keepends=True)
    text, lb = tc.slab_of(lines)
    got = tc.parse_slab(text, lb, nind)
    assert not got["status"].any()
    return got


def test_restatement_equals_the_bed_census_on_the_bed_twin(tmp_path):
    rng = np.random.default_rng(11)
    rows, nind = 60, 13
    codes = rng.choice(np.array([0, 1, 2, 3], dtype=np.uint8), size=(rows, nind), p=[0.4, 0.1, 0.3, 0.2])
    codes[0] = 1
    codes[1, :3] = 1
    codes[1, 3] = 3                        # the first non-missing genotype is hom A2: the TPED line counts A2
    codes[2] = 3
    letters = np.array(list("ACGT"))
    a1 = letters[rng.integers(0, 4, size=rows)]
    a2 = letters[(np.searchsorted(letters, a1) + rng.integers(1, 4, size=rows)) % 4]
    prefix = str(tmp_path / "twin")
    synth.write_bed_and_tped(prefix, codes, ["1"] * rows, np.arange(rows) * 100 + 5, a1=list(a1), a2=list(a2))
    got = parsed_file(prefix + ".tped", nind)
    counts, counted = vc.census(codes)
    assert np.array_equal(got["counts"], counts)
    assert np.array_equal(got["counted"] == 2, counted == 2)
    want_letter = np.where(counted == 0, a1, np.where(counted == 1, a2, "0"))
    assert [chr(c) for c in got["allele"]] == list(want_letter)
    # the same genotypes as copies of the counted allele, whichever of the two letters the image calls A1
    assert np.array_equal(vc.recode(got["codes"], got["counted"]), vc.recode(codes, counted))
    assert (counted == 1).any() and (counted == 2).any()
    # the order bit of such a line: set exactly on hom "A2" of the TPED image (a het reads "A1 A2" with A1 first, or "A2 A1")
    flipped = counted == 1
    assert np.array_equal(got["order"][~flipped], (codes[~flipped] == 3).astype(np.uint8))


def test_restatement_equals_the_vcf_census_on_the_vcf_twin(tmp_path):
    rng = np.random.default_rng(12)
    codes, order = vc.random_genotypes(rng, 50, 11)
    prefix = str(tmp_path / "twin")
    synth.write_vcf_and_tped(prefix, codes, order, ["2"] * 50, np.arange(50) * 10 + 1)
    got = parsed_file(prefix + ".tped", 11)
    counts, counted = vc.census(codes, order)
    assert np.array_equal(got["counts"], counts)
    assert np.array_equal(got["counted"] == 2, counted == 2)
    assert np.array_equal(vc.recode(got["codes"], got["counted"]), vc.recode(codes, counted))
    fc_vcf = vc.first_copy(codes, order, counted)
    fc_tped = vc.first_copy(got["codes"], got["order"], got["counted"])
    assert np.array_equal(fc_vcf, fc_tped)
    # and the reference's own firstCopy wherever a genotype is not missing
    alleles, _ = tc.tped_alleles(prefix + ".tped")
    _, ref_fc, _ = tc.host_arrays(alleles)
    live = codes != vc.MISS
    assert np.array_equal(fc_tped[live], ref_fc[live])


def test_half_missing_and_third_alleles_by_hand():
    def row(text, missing="0"):
        return tc.reference_row([ord(c) for c in text.split()], ord(missing))
    # one = G comes from a half-missing genotype; the first complete genotype is hom of the other allele
    codes, order, one, nalleles, total, data, fc = row("0 G A A G A A G 0 0 A 0")
    assert chr(one) == "G" and list(codes) == [1, 3, 2, 2, 1, 1] and list(order) == [0, 1, 0, 1, 0, 0]
    assert (nalleles, total) == (3, 8) and list(data) == [-9, 0, 1, 1, -9, -9]
    # the image rule would count from the first complete genotype: another allele, other counts
    counts, counted = vc.census(codes[None, :], order[None, :])
    assert counted[0] == 1 and tuple(counts[0]) != (3, 8)
    # three and four letters: everything that is not `one` is the other allele
    codes, order, one, nalleles, total, _, _ = row("C C C G T A A C G T")
    assert chr(one) == "C" and list(codes) == [0, 2, 3, 2, 3] and list(order) == [0, 0, 1, 1, 1] and (nalleles, total) == (4, 10)
    codes, order, one, nalleles, total, _, fc = row("N N N N", missing="N")
    assert chr(one) == "N" and list(codes) == [1, 1] and (nalleles, total) == (0, 0) and fc.all()
    codes, _, one, nalleles, total, _, _ = row("- 0 0 0", missing="-")
    assert chr(one) == "0" and list(codes) == [1, 0] and (nalleles, total) == (3, 3)
    codes, _, one, _, _, _, _ = tc.reference_row([0x80, 0xFF, 0xFF, 0xFF, 0x30, 0x80])
    assert one == 0x80 and list(codes) == [2, 3, 1]


def test_restatement_on_its_own_grammar_and_offences():
    al = [ord(c) for c in "AGGG00AA"]
    clean = tc.parse_line(tc.make_line(al), 4)
    assert clean[4] == (0, 0) and list(clean[0]) == [2, 3, 1, 0] and clean[3] == (3, 6)
    for kw in (dict(sep=b"\t"), dict(sep=b"  "), dict(sep=b" \t "), dict(lead_blank=b"  "), dict(tail=b" \t"), dict(newline=b"\r\n"),
               dict(newline=b""), dict(sep=lambda k: b" " * (1 + k % 3))):
        got = tc.parse_line(tc.make_line(al, **kw), 4)
        assert got[4] == (0, 0) and np.array_equal(got[0], clean[0]) and np.array_equal(got[1], clean[1]), kw
    line = tc.make_line(al)
    lead = len(b"1 rs1 0 1000 ")
    assert tc.parse_line(line[:lead] + b"AA" + line[lead + 1:], 4)[4] == (tc.LONG_ALLELE, 0)
    assert tc.parse_line(line[:-2] + b"AA\n", 4)[4] == (tc.LONG_ALLELE, 3)
    assert tc.parse_line(line, 5)[4] == (tc.FEW_COLUMNS, 4)
    assert tc.parse_line(line[:-3] + b"\n", 4)[4] == (tc.FEW_COLUMNS, 3)
    assert tc.parse_line(line[:-5] + b"\n", 4)[4] == (tc.FEW_COLUMNS, 3)
    assert tc.parse_line(line, 3)[4] == (tc.MANY_COLUMNS, 3)
    assert tc.parse_line(b"1 rs1 0\n", 4)[4] == (tc.FEW_COLUMNS, 0)
    assert tc.parse_line(line[:lead + 4] + b"\v" + line[lead + 5:], 4)[4] == (tc.BAD_BYTE, 1)
    assert tc.parse_line(line[:3] + b"\f" + line[4:], 4)[4] == (tc.BAD_BYTE, 0)


def test_tped_lines_unit_under_sanitizers(tmp_path):
    """tests/host_unit/tped_lines_unit.cpp, compiled here with ASan + UBSan and run over files the case writer wrote: a
    stand-alone program, nothing loaded into python.  Slabs of 700 bytes cut every line of the file somewhere."""
    exe = str(tmp_path / "tped_lines_unit")
    src = os.path.join(ROOT, "tests", "host_unit", "tped_lines_unit.cpp")
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                         "-o", exe, src, "-lz"], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    rng = np.random.default_rng(3)
    nind = 90
    alleles = tc.random_alleles(rng, 12, nind, third=0.1)
    leads = [(b"1", b"rs1", b"0", b"1000"), (b"chr2", b"a.very.long.name/with:things", b"0.25", b"1e6"), (b"X", b"n", b"x", b"12"),
             (b"3", b"rs3", b"1.5e-3", b"2147483647")]
    want, lines = [], []
    for r in range(12):
        lead = leads[r % 4]
        kw = [dict(), dict(sep=b"\t"), dict(sep=b"  ", lead_blank=b" "), dict(newline=b"\r\n", tail=b" ")][r % 4]
        lines.append(tc.make_line(alleles[r], lead=lead, **kw))
        if r in (4, 9):
            lines.append(b"\n" if r == 4 else b"\r\n")          # empty lines are passed over, and counted
        number = len(lines) - (1 if r in (4, 9) else 0)

        def num(tok):
            try:
                return float(tok)
            except ValueError:
                return None
        g, p = num(lead[2]), num(lead[3])
        if g is None:                                       # the stream fails at gpos: gpos = 0, and ppos is not read
            g, p = 0.0, 0.0
        want.append((number, lead[0].decode(), lead[1].decode(), g, p, nind))
    lines[-1] = lines[-1].rstrip(b"\r\n")                   # the file's last line needs no newline
    plain = str(tmp_path / "case.tped")
    open(plain, "wb").write(b"".join(lines))
    with gzip.open(plain + ".gz", "wb") as f:
        f.write(b"".join(lines))
    for path in (plain, plain + ".gz"):
        r = subprocess.run([exe, path, "700"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "tped_lines_unit ok 12" in r.stdout, (r.stdout + r.stderr)[-3000:]
        got = [ln.split("\t") for ln in r.stdout.splitlines()[:-1]]
        assert len(got) == 12
        for g, w in zip(got, want):
            assert (int(g[0]), g[1], g[2], float(g[3]), float(g[4]), int(g[5])) == w, (g, w)
    # a line longer than the slab is reported, not read past
    r = subprocess.run([exe, plain, "100"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "longer than the slab" in r.stderr
