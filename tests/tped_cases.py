"""What garlic_bed_set_rows_tped must give, restated in Python: the reference's TPED loop (src/garlic-data.cpp:103-141) from
the alleles of a line to (codes, order, one, nalleles, total), the grammar of a line byte by byte (tokens, blanks, offences),
and writers of TPED text with control over blank runs, leading-field widths and line ends."""
import numpy as np

import vcf_cases as vc

MISS = 1                       # PLINK's code of a missing genotype
LONG_ALLELE, BAD_BYTE, FEW_COLUMNS, MANY_COLUMNS = 1, 2, 3, 4
BLANKS = b" \t\r"
BAD = b"\v\f\0"
PASS_BYTES = 4096              # tped_parse_kernel: 256 pieces of 16 bytes
NINDS = [1, 3, 4, 5, 7, 8, 9, 63, 64, 65]

pack_image, pack_plane = vc.pack_image, vc.pack_plane


def reference_row(alleles, missing=ord("0")):
    """the loop of src/garlic-data.cpp:109-130 and :141 over the 2 * nind alleles (byte values) of one line ->
    (codes uint8 [nind] in PLINK's codes with A1 := one, order uint8 [nind], one, nalleles, total, data int16 [nind],
    firstCopy bool [nind]); firstCopy is the reference's own (`a1 == oneAllele` as it stands at that genotype)"""
    al = [int(a) for a in alleles]
    nind = len(al) // 2
    one = missing
    nalleles = total = 0
    data = np.zeros(nind, dtype=np.int16)
    fc = np.zeros(nind, dtype=bool)
    for i in range(nind):
        x, y = al[2 * i], al[2 * i + 1]
        if one == missing and x != missing:
            one = x
        if one == missing and y != missing:
            one = y
        v = 0
        for a in (x, y):
            if a == missing:
                v += -9
            elif a == one:
                v += 1
                nalleles += 1
                total += 1
            else:
                total += 1
        data[i] = -9 if v < 0 else v
        fc[i] = x == one
    codes = np.array([{2: 0, 1: 2, 0: 3, -9: 1}[int(v)] for v in data], dtype=np.uint8)
    first = np.array(al[0::2], dtype=np.int64)
    order = ((codes != MISS) & (first != one)).astype(np.uint8)
    return codes, order, one, nalleles, total, data, fc


def parse_line(line, nind, missing=ord("0")):
    """one line byte by byte -> (codes, order, one, (nalleles, total), (code, column)); an offending line gives zeros.
    Tokens are runs of non-blank bytes; token 4 + a is allele a, of individual a >> 1.  Offences, each with the individual it
    is charged to, the smallest (individual, code) wins:
      a token start past the last allele -> MANY_COLUMNS at nind;  a second byte of an allele token -> LONG_ALLELE;
      \\v \\f NUL -> BAD_BYTE (individual 0 inside the leading tokens; capped at nind);  fewer tokens -> FEW_COLUMNS at
      allele tokens found // 2."""
    line = bytes(line)
    nl = line.find(b"\n")
    if nl >= 0:
        line = line[:nl]
    keys, alleles = [], []
    tok, prev_blank = -1, True
    for c in line:
        blank = c in BLANKS
        if not blank:
            start = prev_blank
            if start:
                tok += 1
            col = 0 if tok < 4 else min((tok - 4) >> 1, nind)
            if start and tok >= 4 + 2 * nind:
                keys.append((nind, MANY_COLUMNS))
            if start and 4 <= tok < 4 + 2 * nind:
                alleles.append(c)
            if not start and tok >= 4:
                keys.append((col, LONG_ALLELE))
            if c in BAD:
                keys.append((col, BAD_BYTE))
        prev_blank = blank
    if tok + 1 < 4 + 2 * nind:
        keys.append((max(tok + 1 - 4, 0) >> 1, FEW_COLUMNS))
    if keys:
        col, code = min(keys)
        return np.zeros(nind, np.uint8), np.zeros(nind, np.uint8), 0, (0, 0), (code, col)
    codes, order, one, nalleles, total, _, _ = reference_row(alleles, missing)
    return codes, order, one, (nalleles, total), (0, 0)


def parse_slab(text, line_begin, nind, missing=ord("0")):
    """-> dict(image, plane, status int32 [rows][2], codes, order, allele uint8 [rows], counts int32 [rows][2], counted uint8
    [rows]) of the lines line_begin names in the slab `text`"""
    text = bytes(text)
    rows = len(line_begin) - 1
    codes = np.zeros((rows, nind), dtype=np.uint8)
    order = np.zeros((rows, nind), dtype=np.uint8)
    status = np.zeros((rows, 2), dtype=np.int32)
    allele = np.zeros(rows, dtype=np.uint8)
    counts = np.zeros((rows, 2), dtype=np.int32)
    for r in range(rows):
        limit = min(int(line_begin[r + 1]), len(text))
        codes[r], order[r], allele[r], counts[r], status[r] = parse_line(text[int(line_begin[r]):limit], nind, missing)
    counted = np.where(allele == missing, 2, 0).astype(np.uint8)
    return dict(image=pack_image(codes), plane=pack_plane(order), status=status, codes=codes, order=order, allele=allele,
                counts=counts, counted=counted)


def host_arrays(alleles, missing=ord("0")):
    """what the host reader (parseTpedLine) holds of rows of alleles [rows][2 * nind]: (data int16, firstCopy bool, freq)"""
    rows = [reference_row(a, missing) for a in alleles]
    freq = np.array([r[3] / r[4] if r[4] else 0.0 for r in rows])
    return np.stack([r[5] for r in rows]), np.stack([r[6] for r in rows]), freq


# ---- generators
def random_alleles(rng, rows, nind, letters=b"ACGT", miss=0.08, half=0.05, third=0.0, missing=ord("0")):
    """uint8 [rows][2 * nind]: per row two letters at a random frequency, `third` of the alleles any letter, `miss` of the
    genotypes missing and `half` of them half-missing (either side)"""
    out = np.zeros((rows, 2 * nind), dtype=np.uint8)
    pool = np.frombuffer(bytes(letters), dtype=np.uint8)
    for r in range(rows):
        a, b = rng.choice(len(pool), size=2, replace=False)
        p = rng.uniform(0.1, 0.9)
        al = np.where(rng.random(2 * nind) < p, pool[a], pool[b])
        anyl = rng.random(2 * nind) < third
        al[anyl] = pool[rng.integers(0, len(pool), size=int(anyl.sum()))]
        m = rng.random(nind) < miss
        al[0::2][m] = missing
        al[1::2][m] = missing
        h = rng.random(nind) < half
        side = rng.integers(0, 2, size=nind)
        al[0::2][h & (side == 0)] = missing
        al[1::2][h & (side == 1)] = missing
        out[r] = al
    return out


def make_line(alleles, lead=(b"1", b"rs1", b"0", b"1000"), sep=b" ", lead_blank=b"", tail=b"", newline=b"\n"):
    """one TPED line.  sep: one blank run, or f(k) -> the run in front of token k (k >= 1)"""
    toks = list(lead) + [bytes([int(a)]) for a in alleles]
    run = sep if callable(sep) else (lambda k: sep)
    out = [lead_blank, toks[0]]
    for k in range(1, len(toks)):
        out += [run(k), toks[k]]
    return b"".join(out) + tail + newline


def lead_of_width(width, row=0):
    """four leading tokens that fill exactly `width` bytes with single blanks behind each (width >= 13)"""
    name = b"rs" + (b"%d" % row).rjust(width - 12, b"0")
    lead = (b"1", name, b"0", b"1000")
    assert sum(len(t) + 1 for t in lead) == width, (width, lead)
    return lead


def slab_of(lines, keep=None, header=b""):
    """-> (text, line_begin int64 [kept + 1]); lines not in `keep` stay in the text, line_begin passes over them"""
    at, begins = len(header), []
    for ln in lines:
        begins.append(at)
        at += len(ln)
    keep = range(len(lines)) if keep is None else keep
    lb = [begins[k] for k in keep]
    last = keep[-1] if len(keep) else 0
    lb.append(begins[last] + len(lines[last]))
    return header + b"".join(lines), np.array(lb, dtype=np.int64)


def tped_alleles(path, missing="0"):
    """the alleles of a TPED file written with one-letter tokens: (uint8 [rows][2 * nind], the four leading tokens per row)"""
    rows, leads = [], []
    for line in open(path, "rb").read().splitlines():
        t = line.split()
        if not t:
            continue
        leads.append(t[:4])
        rows.append([x[0] for x in t[4:]])
    return np.array(rows, dtype=np.uint8), leads
