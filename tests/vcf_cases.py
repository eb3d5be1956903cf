"""Cases and a plain numpy restatement of the VCF door (garlic_bed_set_rows_vcf, the order plane, garlic_panel_set_phase_bed);
importable without a GPU.

  grammar      of a data line: nine tab-separated columns, then one column per sample whose leading GT is `a sep b`, a and b
               one of 0 1 . , sep / or | , followed by : tab \\r \\n or the line's end
  codes        0?0 -> 0, .?. -> 1, 0?1 / 1?0 -> 2, 1?1 -> 3 (PLINK's, A1 = REF, A2 = ALT); order bit = (a == '1')
  status       (code, sample column) of the line's first offence in file order, (0, 0) for a clean line
  census       counted = A2 when the first non-missing genotype has its order bit set, else A1, none (2) when all are missing;
               counts = (2 * #hom(counted) + #het, 2 * #non-missing)
  first_copy   non-missing and (order bit == (counted == A2)); all ones on a row without a counted allele
"""
import numpy as np

BAD_BYTE, HALF_MISSING, HAPLOID, ALLELE_INDEX, FEW_COLUMNS, MANY_COLUMNS = 1, 2, 3, 4, 5, 6
MISS = 1
NINDS = [1, 3, 4, 5, 7, 8, 9, 63, 64, 65, 257, 1250]
END = b":\t\r\n"


def decode_gt(field):
    """(status code, PLINK code, order bit) of one sample column (bytes without its tab)"""
    f = field + b"\n"
    a, s = f[0:1], f[1:2]
    if a not in (b"0", b"1", b"."):
        return (ALLELE_INDEX if a.isdigit() else BAD_BYTE), 0, 0
    if s not in (b"/", b"|"):
        return (HAPLOID if s in (b":", b"\t", b"\r", b"\n") else ALLELE_INDEX if s.isdigit() and a != b"." else BAD_BYTE), 0, 0
    b = f[2:3]
    if b not in (b"0", b"1", b"."):
        return (ALLELE_INDEX if b.isdigit() else BAD_BYTE), 0, 0
    e = f[3:4]
    if e not in (b":", b"\t", b"\r", b"\n"):
        return (ALLELE_INDEX if e.isdigit() and b != b"." else BAD_BYTE), 0, 0
    if (a == b".") != (b == b"."):
        return HALF_MISSING, 0, 0
    code = 1 if a == b"." else 2 if a != b else 3 if a == b"1" else 0
    return 0, code, int(a == b"1")


def parse_line(line, nind):
    """line: bytes from the line's first byte (anything behind its first \\n is ignored).
    -> (codes uint8 [nind], order uint8 [nind], (status code, column)); codes / order are meaningful for a clean line only"""
    line = line.split(b"\n", 1)[0]
    cols = line.split(b"\t")
    fields = cols[9:]
    codes = np.zeros(nind, dtype=np.uint8)
    order = np.zeros(nind, dtype=np.uint8)
    status = (0, 0)
    for j, f in enumerate(fields[:nind]):
        st, codes[j], order[j] = decode_gt(f)
        if st and not status[0]:
            status = (st, j)
    if not status[0] and len(fields) < nind:
        status = (FEW_COLUMNS, len(fields))
    if not status[0] and len(fields) > nind:
        status = (MANY_COLUMNS, nind)
    return codes, order, status


def pack_image(codes):
    """.bed rows [rows][(nind + 3) // 4] with zero pad bits"""
    codes = np.asarray(codes, dtype=np.uint8)
    nrows, n = codes.shape
    rb = (n + 3) // 4
    padded = np.zeros((nrows, 4 * rb), dtype=np.uint8)
    padded[:, :n] = codes
    q = padded.reshape(nrows, rb, 4)
    return (q[:, :, 0] | (q[:, :, 1] << 2) | (q[:, :, 2] << 4) | (q[:, :, 3] << 6)).astype(np.uint8)


def pack_plane(bits):
    """one bit per genotype, bit i & 7 of byte i >> 3, zero pad bits: rows [rows][(nind + 7) // 8]"""
    return np.packbits(np.asarray(bits, dtype=np.uint8), axis=1, bitorder="little")


def parse_slab(text, line_begin, nind):
    """-> (image rows, plane rows, status int32 [rows][2], codes, order) of the lines line_begin names in the slab `text`"""
    text = bytes(text)
    rows = len(line_begin) - 1
    codes = np.zeros((rows, nind), dtype=np.uint8)
    order = np.zeros((rows, nind), dtype=np.uint8)
    status = np.zeros((rows, 2), dtype=np.int32)
    for r in range(rows):
        limit = min(int(line_begin[r + 1]), len(text))
        codes[r], order[r], status[r] = parse_line(text[int(line_begin[r]):limit], nind)
    return pack_image(codes), pack_plane(order), status, codes, order


def census(codes, order=None):
    """(counts int32 [rows][2], counted uint8 [rows]); order None: the .bed rule (a het's first allele is A1)"""
    codes = np.asarray(codes)
    order = (codes == 3).astype(np.uint8) if order is None else np.asarray(order)
    nrows = codes.shape[0]
    counts = np.zeros((nrows, 2), dtype=np.int32)
    counted = np.full(nrows, 2, dtype=np.uint8)
    for r in range(nrows):
        nm = np.flatnonzero(codes[r] != MISS)
        if nm.size == 0:
            continue
        c = int(order[r, nm[0]])
        counted[r] = c
        counts[r, 0] = 2 * int(np.count_nonzero(codes[r] == (3 if c else 0))) + int(np.count_nonzero(codes[r] == 2))
        counts[r, 1] = 2 * nm.size
    return counts, counted


def first_copy(codes, order, counted):
    codes, order, counted = np.asarray(codes), np.asarray(order), np.asarray(counted)
    fc = (codes != MISS) & (order == (counted[:, None] == 1))
    fc[counted == 2] = True
    return fc


def tped_read(line, missing="0"):
    """src/garlic-data.cpp:103-130 on one TPED line: (oneAllele, data int16 [nind], firstCopy bool [nind], nalleles, total)"""
    al = line.split()[4:]
    nind = len(al) // 2
    one = missing
    nalleles = total = 0
    data, fc = [], []
    for i in range(nind):
        v = 0
        x, y = al[2 * i], al[2 * i + 1]
        if one == missing and x != missing:
            one = x
        if one == missing and y != missing:
            one = y
        for a in (x, y):
            if a == missing:
                v += -9
            elif a == one:
                v += 1
                nalleles += 1
                total += 1
            else:
                total += 1
        data.append(-9 if v < 0 else v)
        fc.append(x == one)
    return one, np.array(data, dtype=np.int16), np.array(fc, dtype=bool), nalleles, total


def recode(codes, counted):
    """copies of the counted allele per genotype, -9 = missing; a row without a counted allele is all -9"""
    table = np.array([[2, -9, 1, 0], [0, -9, 1, 2], [-9, -9, -9, -9]], dtype=np.int16)
    return table[np.asarray(counted, dtype=np.int64)[:, None], np.asarray(codes, dtype=np.int64)]


# ---- generators
def random_genotypes(rng, rows, nind, miss=0.1):
    """(codes, order): random codes; a het's order bit is random, a hom A2's is 1.  Row 0 begins with a 1|0 het, row 1 with
    ./. and then a 1|0 het, row 2 with a 0|1 het, row 3 is all missing, row 4 all hom A1, row 5 all hom A2 (as far as rows and
    nind go)"""
    codes = rng.integers(0, 4, size=(rows, nind)).astype(np.uint8)
    codes[rng.random(codes.shape) < miss] = MISS
    order = rng.integers(0, 2, size=(rows, nind)).astype(np.uint8)

    def put(r, j, c, o):
        if r < rows and j < nind:
            codes[r, j], order[r, j] = c, o
    put(0, 0, 2, 1)
    put(1, 0, MISS, 0)
    put(1, 1, 2, 1)
    put(2, 0, 2, 0)
    if rows > 3:
        codes[3] = MISS
    if rows > 4:
        codes[4] = 0
    if rows > 5:
        codes[5] = 3
    order[codes == 3] = 1
    order[codes == 0] = 0
    order[codes == MISS] = 0
    return codes, order


FIXED = b"1\t%d\trs%d\tA\tG\t.\tPASS\t.\tGT"


def gt_bytes(code, order, sep):
    a, b = ((b"0", b"0"), (b".", b"."), (b"1", b"0") if order else (b"0", b"1"), (b"1", b"1"))[int(code)]
    return a + sep + b


def field_tail(rng, style):
    """what follows a GT inside its column"""
    if style == "bare":
        return b""
    if style == "short":
        return b":35:0.1,0.9"
    if style == "long":            # several 16-byte pieces
        return b":" + b"7" * int(rng.integers(20, 90))
    if style == "wave":            # more than the 1024 bytes of a wave's 64 pieces
        return b":" + b"8" * 1100
    raise ValueError(style)


def make_lines(rng, codes, order, styles=("bare", "short", "long"), newline=b"\n", wave_at=None):
    """the data lines of a genotype matrix, each with its newline: every column draws its separator and its tail from `styles`;
    wave_at = (row, column) gets the "wave" tail"""
    lines = []
    for r in range(codes.shape[0]):
        cols = [FIXED % (100 + r, r)]
        for j in range(codes.shape[1]):
            style = "wave" if wave_at == (r, j) else styles[int(rng.integers(0, len(styles)))]
            cols.append(gt_bytes(codes[r, j], order[r, j], b"|" if rng.integers(0, 2) else b"/") + field_tail(rng, style))
        lines.append(b"\t".join(cols) + newline)
    return lines


def slab_of(lines, keep=None, header=b"##fileformat=VCFv4.2\n#CHROM\tPOS\n"):
    """(text, line_begin) of the lines joined behind a header; keep: the indices of the lines line_begin names (the others
    stay in the text, left out)"""
    keep = list(range(len(lines))) if keep is None else list(keep)
    at, begins = len(header), []
    for ln in lines:
        begins.append(at)
        at += len(ln)
    text = header + b"".join(lines)
    lb = [begins[k] for k in keep]
    last = keep[-1]
    lb.append(begins[last] + len(lines[last]))
    return text, np.array(lb, dtype=np.int64)


# each offence kind as (name, the column's text, code); the column replaces sample `col` of a clean line
OFFENCES = [
    ("half_missing_a", b"./1", HALF_MISSING),
    ("half_missing_b", b"0|.:5", HALF_MISSING),
    ("haploid", b"1", HAPLOID),
    ("haploid_subfield", b"0:12", HAPLOID),
    ("haploid_missing", b".", HAPLOID),
    ("allele_2", b"0/2", ALLELE_INDEX),
    ("allele_2_first", b"2|0", ALLELE_INDEX),
    ("allele_10", b"0|10", ALLELE_INDEX),
    ("allele_12_first", b"12/0", ALLELE_INDEX),
    ("bad_sep", b"0-1", BAD_BYTE),
    ("bad_letter", b"A|0", BAD_BYTE),
    ("bad_end", b"0|1;7", BAD_BYTE),
    ("empty", b"", BAD_BYTE),
    ("nul", b"0|\x001", BAD_BYTE),
]
