"""CPU: the yardstick of the PLINK .bed door (tests/bed_cases.py) against the reference's TPED rule on the twin TPED text, and
the .bim / .fam / .bed reader through a stand-alone program built with ASan + UBSan."""
import os
import subprocess

import numpy as np
import pytest

import bed_cases as cases
from garlic_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n", cases.CENSUS_N)
def test_restatement_agrees_with_the_tped_rule_on_the_twin_text(tmp_path, n):
    """census() / recode() of bed_cases -- what the GPU tests compare the device against -- equal the reference's loop
    (garlic-data.cpp:107-141, transcribed in tped_census) run over the TPED lines synth.write_bed_and_tped writes for the
    same genotypes: hom A1 "A1 A1", het "A1 A2", hom A2 "A2 A2", missing "0 0".  Also: the .bed it writes holds pack_rows' bytes"""
    rng = np.random.default_rng(100 + n)
    codes = cases.case_codes(n, rng)
    nrows = codes.shape[0]
    prefix = str(tmp_path / "twin")
    synth.write_bed_and_tped(prefix, codes, ["1"] * nrows, np.arange(1, nrows + 1) * 100, a1="C", a2="T")
    counts, counted = cases.census(codes)
    data = cases.recode(codes, counted)
    assert set(counted.tolist()) == {0, 1, 2}
    with open(prefix + ".tped") as f:
        lines = f.read().splitlines()
    assert len(lines) == nrows
    for r, line in enumerate(lines):
        one, want, nalleles, total = cases.tped_census(line)
        assert one == ("C", "T", "0")[counted[r]], r
        assert (nalleles, total) == tuple(counts[r]), r
        assert np.array_equal(want, data[r]), r
    raw = open(prefix + ".bed", "rb").read()
    assert raw[:3] == bytes([0x6C, 0x1B, 0x01])
    assert np.array_equal(np.frombuffer(raw[3:], dtype=np.uint8).reshape(nrows, -1), cases.pack_rows(codes, garbage=False))


def test_dest_maps_cover_what_the_score_test_promises():
    nloci = sum(cases.SCORE_CHR)
    codes = cases.score_file(np.random.default_rng(1))
    maps = cases.dest_maps(codes.shape[0], nloci)
    s = maps["scattered"][0]
    assert s[0] == -1 and s[-1] == -1 and (s[25:45] == -1).all() and np.count_nonzero(s >= 0) == nloci
    for name, calls in maps.items():
        for m in calls:
            kept = m[m >= 0]
            assert (np.diff(kept) > 0).all(), name
        assert np.array_equal(np.sort(np.concatenate([m[m >= 0] for m in calls])), np.arange(nloci)), name
    a, b = maps["two_calls"]
    assert np.array_equal(cases.final_map(maps["two_calls"]), cases.final_map(maps["scattered"]))
    assert cases.keep_all_file(np.random.default_rng(1)).shape[0] == nloci      # the keep-all variant: a row per locus
    assert set((a[a >= 0] // 16).tolist()) & set((b[b >= 0] // 16).tolist())     # words written by both calls


def test_reader_refuses_what_it_must_and_the_filter_edits_only_the_row_map(tmp_path):
    """tests/host_unit/bed_unit.cpp (compiled here, ASan + UBSan; a stand-alone program): openBedFile on a bad magic, a
    truncated and an overlong file, an individual-major header, multi-character alleles and a short .bim line; a chr change
    and ppos given as 1e6 in the good one; genotypeAt, filterMonomorphicSites and writeGenotypeCache on a bed panel"""
    d = tmp_path
    codes = (np.arange(6)[:, None] + np.arange(5)[None, :]) % 4
    rows = cases.pack_rows(codes, garbage=True).tobytes()
    magic = bytes([0x6C, 0x1B, 0x01])
    (d / "good.bed").write_bytes(magic + rows)
    (d / "badmagic.bed").write_bytes(bytes([0x6C, 0x1C, 0x01]) + rows)
    (d / "indmajor.bed").write_bytes(bytes([0x6C, 0x1B, 0x00]) + rows)
    (d / "truncated.bed").write_bytes(magic + rows[:-1])
    (d / "toolong.bed").write_bytes(magic + rows + b"\0")
    (d / "good.fam").write_text("".join("POP i%d 0 0 0 -9\n" % i for i in range(5)))
    bim = ["1 rs0 0 100 A G", "1 rs1 0.5 1e6 A G", "1 rs2 0.7 1000100 C T", "2 rs3 0 50 A G", "2 rs4 0 60 A G", "chrX rs5 0 70 A G"]
    (d / "good.bim").write_text("\n".join(bim) + "\n")
    (d / "multichar.bim").write_text("\n".join(bim[:2] + ["1 rs2 0.7 1000100 C TTA"] + bim[3:]) + "\n")
    (d / "fivecols.bim").write_text("\n".join(bim[:4] + ["2 rs4 0 60 A"] + bim[5:]) + "\n")
    exe = str(d / "bed_unit")
    libdir = os.path.join(ROOT, "garlic_amd")
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                         "-o", exe, os.path.join(ROOT, "tests", "host_unit", "bed_unit.cpp"),
                         os.path.join(libdir, "host", "garlic_host.cpp"), "-L" + libdir, "-lgarlic_hip", "-lz",
                         "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    r = subprocess.run([exe, str(d)], capture_output=True, text=True)
    assert r.returncode == 0 and "bed_unit ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
    for word in ("magic", "truncated", "individual-major", "single character", "6 columns"):
        assert word in r.stderr, word
