"""Feature counts from a PLINK .bed (garlic_feature_set_rows_bed, garlic-lod --bfile-counting): the hom rows restated in
numpy, the file_row lists of the GPU test, and the golden TPED lines as a .bed file set.  Importable without a GPU.

The rule: output row k is image row file_row[k] under selector allele[k]; bit i is set iff individual i has PLINK code 0 (hom
A1) for selector 0, code 3 (hom A2) for selector 1; selector 2 sets nothing.  Codes: 0 hom A1, 1 missing, 2 het, 3 hom A2."""
import numpy as np

NINDS = [1, 3, 4, 5, 63, 64, 65, 130, 257, 513]
ROW_COUNTS = [0, 1, 63, 64, 65, 300]
IMAGE_ROWS = 70
PADS = [0x00, 0xFF]


def hom_rows(codes, file_row, allele):
    """bool [len(file_row), nind]"""
    codes = np.asarray(codes)
    file_row, allele = np.asarray(file_row, dtype=np.int64), np.asarray(allele, dtype=np.uint8)
    src = codes[file_row] if file_row.shape[0] else np.zeros((0, codes.shape[1]), dtype=codes.dtype)
    want = np.where(allele == 0, 0, np.where(allele == 1, 3, 255))[:, None]
    return src == want


def image_codes(nind, rng, nrows=IMAGE_ROWS):
    """PLINK codes [nrows, nind]: random rows, and rows of one code each (all hom A1, all missing, all het, all hom A2) at the
    image's two ends, so that rows 0 and nrows - 1 tell a selector from the other"""
    codes = rng.integers(0, 4, size=(nrows, nind)).astype(np.uint8)
    codes[0], codes[1], codes[2], codes[3] = 0, 3, 1, 2
    codes[nrows - 1], codes[nrows - 2] = 3, 0
    return codes


def plans(n_out, nrows, rng):
    """name -> (file_row, allele) of n_out entries: the identity (cycled over the image), descending, and repeats -- both
    selectors of one image row next to each other; every list of more than one entry holds rows 0 and nrows - 1; the
    selectors run through 0, 1 and 2"""
    k = np.arange(n_out, dtype=np.int64)
    sel = rng.integers(0, 3, size=n_out).astype(np.uint8)
    ident = k % nrows
    desc = (nrows - 1 - k) % nrows
    rep = (k // 2) % nrows
    rep_sel = (k % 2).astype(np.uint8)
    if n_out > 1:
        ident[-1] = nrows - 1
        desc[-1] = 0
        rep[-2:] = nrows - 1
    if n_out == 1:
        ident[0], desc[0], rep[0] = nrows - 1, nrows - 1, 0
    if n_out > 4:
        rep_sel[4] = 2
    return {"identity": (ident, sel), "descending": (desc, sel.copy()), "repeats": (rep, rep_sel)}


# The one line of the golden cases with three alleles (case1, chr22:100: `G G T T A G 0 0 G G`).  A .bed row holds two: the
# two that occur homozygous are kept, and the genotype with the third (a heterozygote, which counts for nothing) is coded
# missing.  Every other line must have at most two distinct non-missing alleles.
THREE_ALLELES = {("22", "100"): ("G", "T")}


def tped_lines_to_bed(lines, prefix, iids, fid="POP", three_alleles=None):
    """TPED lines (chromosome, id, genetic position, position, allele pairs) as prefix.bed / .bim / .fam.  A1 / A2 of a line: its
    distinct non-missing alleles in order of appearance (`0` for one that does not occur); at most two, asserted, but for
    the lines of `three_alleles` {(chromosome, position): (A1, A2)}, whose homozygotes must all be A1 or A2.  A pair of A1
    and A2 is a het in either order; a pair with a missing allele, or with a third one, is missing."""
    three_alleles = three_alleles or {}
    rows, bim = [], []
    for line in lines:
        f = line.split()
        g = f[4:]
        assert len(g) == 2 * len(iids), line
        seen = []
        for a in g:
            if a != "0" and a not in seen:
                seen.append(a)
        if (f[0], f[3]) in three_alleles:
            assert len(seen) == 3, line
            seen = list(three_alleles[(f[0], f[3])])
            assert all(g[2 * i] in seen + ["0"] for i in range(len(iids)) if g[2 * i] == g[2 * i + 1]), ("a third allele is homozygous", line)
        assert len(seen) <= 2, ("more than two alleles on a line", line)
        a1, a2 = (seen + ["0", "0"])[:2]
        codes = np.empty(len(iids), dtype=np.uint8)
        for i in range(len(iids)):
            x, y = g[2 * i], g[2 * i + 1]
            codes[i] = 1 if "0" in (x, y) or x not in seen or y not in seen else 2 if x != y else 0 if x == a1 else 3
        rows.append(codes)
        bim.append("%s\t%s\t%s\t%s\t%s\t%s\n" % (f[0], f[1], f[2], f[3], a1, a2))
    from garlic_amd import synth
    with open(prefix + ".bed", "wb") as out:
        out.write(bytes([0x6C, 0x1B, 0x01]))
        out.write(synth.bed_rows(np.array(rows, dtype=np.uint8)).tobytes())
    with open(prefix + ".bim", "w") as out:
        out.write("".join(bim))
    with open(prefix + ".fam", "w") as out:
        out.write("".join("%s %s 0 0 0 -9\n" % (fid, i) for i in iids))
    return prefix
