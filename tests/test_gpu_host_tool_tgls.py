"""GPU: garlic-lod --tgls through the device reader (loadTGLSFile: the text parsed and dictionary-coded on the device, the
panels filled device to device) against the same run under GARLIC_TGLS_HOST_READER=1 (readTGLSData, which
tests/test_oracle_vs_ref.py pins to the reference's reader): every output file byte for byte, and the same "Genotype
likelihoods" line.  600 loci x 24 individuals, W = 30; GQ integers (one-byte codes), GL decimals (16-bit codes) and GL values
in every spelling of the grammar (exponents, +, .5, 5., signed zeros), one row of each file with a token the device defers to
the host's stream parse."""
import filecmp
import glob
import gzip
import os
import shutil
import subprocess

import numpy as np
import pytest

import tgls_cases as tc
from garlic_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E2E = os.path.join(ROOT, "tests", "golden", "e2e")
TOOL = os.path.join(ROOT, "garlic_amd", "host", "garlic-lod")
COMMON = ["--centromere", os.path.join(E2E, "tiny.centromeres.txt"), "--kde-subsample", "0", "--winsize", "30", "--raw-lod",
          "--lod-cutoff", "-11", "--size-bounds", "50000", "200000"]
NIND = 24
KEPT = [1, 2, 5, 8, 13, 14, 20, 21, 23]


def make_set(d, n, seed):
    """n SNPs x 24 individuals at the first n positions of the e2e fixture as VCF, TPED / TFAM and PLINK twins, a keep file,
    and likelihood files: GQ (two-digit integers), GL (3 decimals, more than 256 distinct values), each plain and .gz"""
    chrs, pos = [], []
    with gzip.open(os.path.join(E2E, "tiny.tped.gz"), "rt") as f:
        for line in f:
            t = line.split(None, 4)
            chrs.append(t[0])
            pos.append(int(float(t[3])))
            if len(chrs) == n:
                break
    assert len(chrs) == n
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.05, 0.95, size=(n, 1))
    u = rng.random((n, NIND))
    codes = np.where(u < (1 - p) ** 2, 3, np.where(u < (1 - p) ** 2 + 2 * p * (1 - p), 2, 0)).astype(np.uint8)
    codes[rng.random(codes.shape) < 0.03] = 1
    codes[5::97] = 0                          # monomorphic rows: the site filter edits the row map
    order = np.zeros_like(codes)
    order[codes == 3] = 1
    prefix = str(d / "X")
    synth.write_vcf_and_tped(prefix, codes, order, chrs, pos)
    plink = str(d / "B")
    synth.write_bed_and_tped(plink, codes, chrs, pos)
    with open(plink + ".fam") as f:
        fam = [line.split()[:2] for line in f]
    with open(plink + ".keep", "w") as f:
        f.write("".join("%s %s\n" % tuple(fam[i]) for i in KEPT))
    files = {}
    gq = rng.integers(0, 100, size=(n, NIND))
    gl = -rng.integers(0, 12000, size=(n, NIND)) / 1000.0
    for name, rows in (("GQ", [["%d" % v for v in r] for r in gq]), ("GL", [["%.3f" % v for v in r] for r in gl])):
        rows[7][3] = "30.000000000000000000" if name == "GQ" else "-0.12345678901234567"       # deferred: more digits than 2^53 holds
        path = str(d / (name + ".tgls"))
        with open(path, "w") as f:
            for l, r in enumerate(rows):
                f.write("%s rs%d 0 %d %s\n" % (chrs[l], l, pos[l], (" " if l % 2 else "\t").join(r)))
        with open(path, "rb") as f, gzip.open(path + ".gz", "wb") as g:
            shutil.copyfileobj(f, g)
        files[name] = path
    files["GLX"] = spellings_file(str(d / "GLX.tgls"), rng, chrs, pos)
    return {"vcf": prefix + ".vcf", "tped": ["--tped", prefix + ".tped", "--tfam", prefix + ".tfam"], "plink": plink, "tgls": files}


def spellings_file(path, rng, chrs, pos):
    """GL values -12 .. 0 to three decimals, each in a spelling spelled() draws, and in every row five valued members of
    grammar_tokens(): an exponent, a +, a .5, a 5. and a signed zero; one token deferred for its exponent"""
    valued = [t for t, _ in tc.grammar_tokens() if not tc.defers(t)]
    picks = [[t for t in valued if b"e" in t.lower() and float(t) != 0], [b"+5", b"+5.e0", b"+0.000"], [b".5", b"-.5"], [b"5.", b"0."],
             [b"0", b"-0", b"-0.0", b"+0.000", b"-.0", b"0e99999999999", b"-0e-99999999999"]]
    assert all(len(p) >= 2 and set(p) <= set(valued) for p in picks)
    with open(path, "wb") as f:
        for l in range(len(chrs)):
            row = [tc.spelled(rng, int(m), -3, sign=b"-") for m in rng.integers(1, 12000, size=NIND)]
            for p, c in zip(picks, rng.permutation(NIND)):
                row[c] = p[int(rng.integers(0, len(p)))]
            if l == 7:
                row[3] = b"1e-23"                      # deferred: the exponent is past the fast path
            f.write(b"%s rs%d 0 %d " % (chrs[l].encode(), l, pos[l]) + (b" " if l % 2 else b"\t").join(row) + b"\n")
    return path


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    return make_set(tmp_path_factory.mktemp("tgls_tool"), 600, 7)


def run(tmp, inputs, host_reader, *extra):
    os.makedirs(str(tmp), exist_ok=True)
    out = os.path.join(str(tmp), "mine")
    env = dict(os.environ)
    env.pop("GARLIC_TGLS_HOST_READER", None)
    if host_reader:
        env["GARLIC_TGLS_HOST_READER"] = "1"
    r = subprocess.run([TOOL, *inputs, "--out", out, *COMMON, *extra], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    return out, r.stderr


def both(tmp_path, inputs, tgls, gl_type, want_form):
    """the device reader against the host reader: -> the device run's stderr"""
    args = ["--tgls", tgls, "--gl-type", gl_type]
    a, err_a = run(tmp_path / "device", inputs, False, *args)
    b, err_b = run(tmp_path / "host", inputs, True, *args)
    names = sorted(p[len(a):] for p in glob.glob(a + "*"))
    assert names == sorted(p[len(b):] for p in glob.glob(b + "*"))
    assert ".freq.gz" in names and any(n.endswith(".raw.lod.windows.gz") for n in names) and len(names) >= 3, names
    for n in names:
        assert os.path.getsize(a + n) > 0 and filecmp.cmp(a + n, b + n, shallow=False), n
    line_a = [l for l in err_a.splitlines() if l.startswith("Genotype likelihoods")]
    line_b = [l for l in err_b.splitlines() if l.startswith("Genotype likelihoods")]
    assert len(line_a) == 1 and line_a == line_b and want_form in line_a[0], (line_a, line_b)
    return err_a


@pytest.mark.parametrize("gl_type,form", [("GQ", "one-byte codes"), ("GL", "16-bit codes")])
def test_tped_run_equals_the_host_readers(tmp_path, small, gl_type, form):
    err = both(tmp_path, small["tped"], small["tgls"][gl_type], gl_type, form)
    assert "host reader" not in err


def test_every_spelling_of_the_grammar_equals_the_host_readers(tmp_path, small):
    err = both(tmp_path, small["tped"], small["tgls"]["GLX"], "GL", "16-bit codes")
    assert "host reader" not in err


@pytest.mark.parametrize("gl_type,form", [("GQ", "one-byte codes"), ("GL", "16-bit codes")])
def test_gz_file(tmp_path, small, gl_type, form):
    both(tmp_path, small["tped"], small["tgls"][gl_type] + ".gz", gl_type, form)


def test_vcf_with_tgls(tmp_path, small):
    both(tmp_path, ["--vcf", small["vcf"]], small["tgls"]["GQ"], "GQ", "one-byte codes")


@pytest.mark.parametrize("gl_type,form", [("GQ", "one-byte codes"), ("GL", "16-bit codes")])
def test_keep_takes_a_column_subset(tmp_path, small, gl_type, form):
    both(tmp_path, ["--bfile", small["plink"], "--keep", small["plink"] + ".keep"], small["tgls"][gl_type], gl_type, form)


def test_three_shards_on_one_device(tmp_path, small):
    a, _ = run(tmp_path / "one", small["tped"], False, "--tgls", small["tgls"]["GL"], "--gl-type", "GL")
    b, _ = run(tmp_path / "three", small["tped"], False, "--tgls", small["tgls"]["GL"], "--gl-type", "GL", "--devices", "0,0,0")
    for p in glob.glob(a + "*"):
        assert filecmp.cmp(p, b + p[len(a):], shallow=False), p


def test_a_file_of_more_than_65536_values_falls_back_by_itself(tmp_path, tmp_path_factory):
    """3,000 loci x 24 individuals of distinct values: the device refuses, one line on stderr, the host reader takes over"""
    big = make_set(tmp_path_factory.mktemp("tgls_big"), 3000, 9)
    path = str(tmp_path / "distinct.tgls")
    with open(big["tgls"]["GQ"]) as f, open(path, "w") as g:
        for l, line in enumerate(f):
            t = line.split()
            g.write(" ".join(t[:4] + ["%d.%05d" % (l % 90, 24 * l + i) for i in range(NIND)]) + "\n")
    a, err_a = run(tmp_path / "device", big["tped"], False, "--tgls", path, "--gl-type", "GQ")
    b, err_b = run(tmp_path / "host", big["tped"], True, "--tgls", path, "--gl-type", "GQ")
    assert err_a.count("read by the host reader instead") == 1 and "read by the host reader" not in err_b
    for p in glob.glob(a + "*"):
        assert filecmp.cmp(p, b + p[len(a):], shallow=False), p
