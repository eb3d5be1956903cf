"""GPU: garlic-lod --vcf X --vcf-gl-field KEY --gl-type T against garlic-lod --vcf X --tgls X.tgls --gl-type T and against the
--tped twin with that .tgls, on the fixture panel of tests/test_gpu_host_tool_vcf.py (6,000 SNPs x 24 individuals): the same
files byte for byte.  The VCF carries GQ as its third subfield under a FORMAT that changes from line to line, and a custom
scalar key XL of three decimals; X.tgls holds the same tokens, `0` where a missing genotype has none.  The --tgls path is
pinned to the reference's binary by tests/golden/e2e.

--keep is not among the modes: --vcf with --keep is a usage error of the tool (tests/test_gpu_host_tool_vcf.py holds it to that)."""
import gzip
import os
import shutil

import numpy as np
import pytest

import test_gpu_host_tool_vcf as hv

pytestmark = pytest.mark.gpu
twin = hv.twin
E2E = hv.E2E
CALLS = ["--lod-cutoff", "-11", "--size-bounds", "50000", "200000"]
MODES = {
    "unweighted": ["--raw-lod", *CALLS],
    "weighted": ["--raw-lod", "--weighted", "--map", os.path.join(E2E, "tiny.map"), "--ld-subsample", "11", "--ld-seed", "5",
                 "--lod-cutoff", "-4", "--size-bounds", "50000", "200000"],
}
FORMATS = ["GT:DP:GQ", "GT:AD:GQ:XL:PL", "GT:X:GQ:XL"]
XL_FORMATS = ["GT:DP:XL", "GT:AD:GQ:XL:PL", "GT:X:XL:GQ"]


def with_likelihoods(prefix, out, drop_alt=(), formats=FORMATS, xl_decimals=3):
    """out.vcf: the lines of prefix.vcf with FORMAT and the subfields rewritten; out.GQ.tgls / out.XL.tgls: the twins.
    drop_alt: data lines whose ALT becomes a list (no biallelic SNP); the twins leave them out"""
    rng = np.random.default_rng(9)
    vcf, gq_lines, xl_lines, k = [], [], [], 0
    for line in open(prefix + ".vcf").read().split("\n"):
        if not line or line.startswith("#"):
            vcf.append(line)
            continue
        t = line.split("\t")
        fmt = formats[k % 3].split(":")
        gq_tok, xl_tok = [], []
        for j in range(9, len(t)):
            gt = t[j].split(":")[0]
            gq = "%d" % rng.integers(0, 100)
            xl = "-%d.%0*d" % (rng.integers(0, 9), xl_decimals, rng.integers(0, 10 ** xl_decimals))
            sub = {"DP": "%d" % rng.integers(1, 60), "AD": "3,4", "X": "%d,0.%d" % (k % 50, j), "GQ": gq, "XL": xl,
                   "PL": ",".join("%d" % v for v in rng.integers(0, 10 ** 8, size=9))}
            fields = [gt] + [sub[name] for name in fmt[1:]]
            if gt[0] == ".":                      # a missing genotype: its trailing subfields dropped, '.', or nothing
                how = (k + j) % 4
                gone = fmt[2:] if how == 0 else fmt[2:3] if how in (1, 2) else []
                if how == 0:
                    fields = fields[:2]
                elif how in (1, 2):
                    fields[2] = "." if how == 1 else ""
                gq = "0" if "GQ" in gone else gq
                xl = "0" if "XL" in gone else xl
            if "XL" not in fmt:
                xl = "0"
            gq_tok.append(gq)
            xl_tok.append(xl)
            t[j] = ":".join(fields)
        t[8] = ":".join(fmt)
        if k in drop_alt:
            t[4] = "G,T"
        else:
            head = "%s %s 0 %s " % (t[0], t[2], t[1])
            gq_lines.append(head + " ".join(gq_tok))
            xl_lines.append(head + " ".join(xl_tok))
        vcf.append("\t".join(t))
        k += 1
    open(out + ".vcf", "w").write("\n".join(vcf))
    open(out + ".GQ.tgls", "w").write("".join(ln + "\n" for ln in gq_lines))
    open(out + ".XL.tgls", "w").write("".join(ln + "\n" for ln in xl_lines))
    return out


@pytest.fixture(scope="module")
def gl_twin(twin, tmp_path_factory):
    return with_likelihoods(twin, str(tmp_path_factory.mktemp("vcfgl") / "G"))


def field(key, gl_type):
    return ["--vcf-gl-field", key, "--gl-type", gl_type]


@pytest.mark.parametrize("mode", sorted(MODES))
def test_field_equals_the_tgls_twin_and_the_tped_twin(tmp_path, twin, gl_twin, mode):
    tgls = ["--tgls", gl_twin + ".GQ.tgls", "--gl-type", "GQ"]
    a = hv.run(tmp_path / "field", ["--vcf", gl_twin + ".vcf"], *MODES[mode], *field("GQ", "GQ"))
    b = hv.run(tmp_path / "tgls", ["--vcf", gl_twin + ".vcf"], *MODES[mode], *tgls)
    c = hv.run(tmp_path / "tped", hv.tped_of(twin), *MODES[mode], *tgls)
    hv.same_files(a, b)
    hv.same_files(a, c)


def test_long_info_in_front_of_format(tmp_path, gl_twin):
    """INFO of a third of the data lines grown to 1 to 9 KB (colons and the key's letters in it): FORMAT then stands in the
    first, the second and the third 4 KB pass of the likelihood parse, and the genotype parse reads the same lines.  The same
    files as from the unpadded file"""
    rng = np.random.default_rng(31)
    lines = open(gl_twin + ".vcf").read().split("\n")
    k, passes = 0, set()
    for i, ln in enumerate(lines):
        if not ln or ln.startswith("#"):
            continue
        if k % 3 == 0:
            t = ln.split("\t")
            n = int(rng.integers(1024, 9 * 1024 + 1))
            t[7] = ("DP=14;GQ:AF=0.5,GQ;Q=:GQ:;" * (n // 26 + 1))[:n]
            lines[i] = "\t".join(t)
            passes.add(lines[i].index("\tGT:") // 4096)
        k += 1
    assert passes == {0, 1, 2}
    path = str(tmp_path / "I.vcf")
    open(path, "w").write("\n".join(lines))
    a = hv.run(tmp_path / "padded", ["--vcf", path], *MODES["unweighted"], *field("GQ", "GQ"))
    b = hv.run(tmp_path / "plain", ["--vcf", gl_twin + ".vcf"], *MODES["unweighted"], *field("GQ", "GQ"))
    hv.same_files(a, b)


def test_gz_phased_and_two_shards(tmp_path, twin, gl_twin):
    with open(gl_twin + ".vcf", "rb") as f, gzip.open(str(tmp_path / "G.vcf.gz"), "wb") as g:
        shutil.copyfileobj(f, g)
    mode = MODES["weighted"] + ["--phased"]
    a = hv.run(tmp_path / "gz", ["--vcf", str(tmp_path / "G.vcf.gz")], *mode, *field("GQ", "GQ"), "--devices", "0,0")
    b = hv.run(tmp_path / "tped", hv.tped_of(twin), *mode, "--tgls", gl_twin + ".GQ.tgls", "--gl-type", "GQ")
    hv.same_files(a, b)


def test_a_custom_scalar_key_enters_the_16_bit_form(tmp_path, twin, gl_twin):
    """XL: three decimals, thousands of distinct values.  A file whose first line does not name it is refused there"""
    lines = open(gl_twin + ".vcf").read().split("\n")
    first = next(k for k, ln in enumerate(lines) if ln and not ln.startswith("#"))
    assert "XL" not in lines[first].split("\t")[8]
    r = hv.run(tmp_path / "refused", ["--vcf", gl_twin + ".vcf"], *MODES["unweighted"], *field("XL", "GL"), ok=False)
    assert r.returncode != 0 and "line %d of" % (first + 1) in r.stderr and "FORMAT does not name XL" in r.stderr, r.stderr[-500:]
    g = with_likelihoods(twin, str(tmp_path / "X"), formats=XL_FORMATS)
    tgls = ["--tgls", g + ".XL.tgls", "--gl-type", "GL"]
    r = hv.run(tmp_path / "field", ["--vcf", g + ".vcf"], *MODES["unweighted"], *field("XL", "GL"), ok=False)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "FORMAT field XL" in r.stderr and "16-bit codes" in r.stderr, r.stderr[-800:]
    b = hv.run(tmp_path / "tgls", ["--vcf", g + ".vcf"], *MODES["unweighted"], *tgls)
    c = hv.run(tmp_path / "tped", hv.tped_of(twin), *MODES["unweighted"], *tgls)
    hv.same_files(str(tmp_path / "field" / "mine"), b)
    hv.same_files(b, c)


def test_more_than_65536_distinct_values_fall_back_to_the_host_reader(tmp_path, twin):
    """XL with five decimals: about 130,000 distinct raw values among the 144,000 genotypes.  The device object refuses the
    65,537th, the tool says so and reads the field on the host (vcf::parseGlValues per line) into the forms of readTGLSData,
    to which --tgls falls back by itself: the same files"""
    g = with_likelihoods(twin, str(tmp_path / "W"), formats=XL_FORMATS, xl_decimals=5)
    values = set(tok for ln in open(g + ".XL.tgls") for tok in ln.split()[4:])
    assert len(values) > 65536
    r = hv.run(tmp_path / "field", ["--vcf", g + ".vcf"], *MODES["unweighted"], *field("XL", "GL"), ok=False)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "XL holds more than 65,536 distinct values: read by the host reader instead" in r.stderr, r.stderr[:1500]
    b = hv.run(tmp_path / "tgls", ["--vcf", g + ".vcf"], *MODES["unweighted"], "--tgls", g + ".XL.tgls", "--gl-type", "GL")
    hv.same_files(str(tmp_path / "field" / "mine"), b)


def test_lines_left_out_stay_out_of_both_parses(tmp_path, twin):
    drop = (10, 20, 30)
    g = with_likelihoods(twin, str(tmp_path / "L"), drop_alt=drop)
    a = hv.run(tmp_path / "field", ["--vcf", g + ".vcf", "--vcf-biallelic-snps-only"], *MODES["unweighted"], *field("GQ", "GQ"), ok=False)
    assert a.returncode == 0 and "Left out 3 lines" in a.stderr, a.stderr[-500:]
    tped = [ln for k, ln in enumerate(open(twin + ".tped").read().splitlines()) if k not in drop]
    open(str(tmp_path / "less.tped"), "w").write("".join(ln + "\n" for ln in tped))
    b = hv.run(tmp_path / "tped", ["--tped", str(tmp_path / "less.tped"), "--tfam", twin + ".tfam"], *MODES["unweighted"],
               "--tgls", g + ".GQ.tgls", "--gl-type", "GQ")
    hv.same_files(str(tmp_path / "field" / "mine"), b)


def test_a_called_genotype_without_the_field(tmp_path, gl_twin):
    lines = open(gl_twin + ".vcf").read().split("\n")
    first = next(k for k, ln in enumerate(lines) if ln and not ln.startswith("#"))
    k = next(k for k in range(first + 40, len(lines)) if lines[k].split("\t")[9 + 6][0] != ".")
    t = lines[k].split("\t")
    t[9 + 6] = ":".join(t[9 + 6].split(":")[:2])
    lines[k] = "\t".join(t)
    path = str(tmp_path / "nogq.vcf")
    open(path, "w").write("\n".join(lines))
    r = hv.run(tmp_path / "bad", ["--vcf", path], *MODES["unweighted"], *field("GQ", "GQ"), ok=False)
    assert r.returncode != 0 and "line %d of %s" % (k + 1, path) in r.stderr and "sample 7 (ind6)" in r.stderr and "without GQ" in r.stderr, r.stderr[-500:]
    r = hv.run(tmp_path / "ok", ["--vcf", path], *MODES["unweighted"], *field("GQ", "GQ"), "--vcf-gl-missing", "0", ok=False)
    assert r.returncode == 0, r.stderr[-1000:]
    # a list is refused on the host with the same coordinates
    t[9 + 6] = t[9 + 6] + ":0,12,40"
    lines[k] = "\t".join(t)
    open(path, "w").write("\n".join(lines))
    r = hv.run(tmp_path / "list", ["--vcf", path], *MODES["unweighted"], *field("GQ", "GQ"), ok=False)
    assert r.returncode != 0 and "line %d of" % (k + 1) in r.stderr and "ind6" in r.stderr and "list" in r.stderr, r.stderr[-500:]


def test_usage_errors(tmp_path, gl_twin, twin):
    vcf = ["--vcf", gl_twin + ".vcf"]
    r = hv.run(tmp_path, vcf, *MODES["unweighted"], *field("GQ", "GQ"), "--tgls", gl_twin + ".GQ.tgls", ok=False)
    assert r.returncode != 0 and "--vcf-gl-field and --tgls" in r.stderr
    r = hv.run(tmp_path, hv.tped_of(twin), *MODES["unweighted"], *field("GQ", "GQ"), ok=False)
    assert r.returncode != 0 and "needs --vcf" in r.stderr
    r = hv.run(tmp_path, vcf, *MODES["unweighted"], *field("GT", "GQ"), ok=False)
    assert r.returncode != 0 and "--vcf-gl-field" in r.stderr
    r = hv.run(tmp_path, vcf, *MODES["unweighted"], "--vcf-gl-field", "GQ", ok=False)
    assert r.returncode != 0 and "GQ/GL/PL" in r.stderr
