"""Cases and plain numpy restatements for the PLINK .bed door (garlic_bed_*, garlic_panel_set_genotypes_bed); importable
without a GPU.

  PLINK codes    0 hom A1, 1 missing, 2 het, 3 hom A2 (the two bits of a .bed genotype, read as a number)
  census         per row: counted (0 = A1, 1 = A2, 2 = none) from the first non-missing genotype in file order -- A2 when it is
                 hom A2, else A1 -- and counts = (nalleles, total) = (2 * #hom(counted) + #het, 2 * #non-missing)
  recode         int16 [rows][nind]: copies of the row's counted allele, -9 = missing (what garlic_panel_set_genotypes takes)
  tped_census    the reference's loop over the character pairs of a TPED line (src/garlic-data.cpp:107-130), transcribed
  case_codes     the rows every N of the census test gets
  pack_rows      .bed rows from codes, with a chosen row pitch and garbage in the bits past the last individual
"""
import numpy as np

CENSUS_N = [1, 3, 4, 5, 63, 64, 65, 127, 130, 257, 1025, 4100]
MISS = 1


def census(codes):
    codes = np.asarray(codes)
    nrows = codes.shape[0]
    counts = np.zeros((nrows, 2), dtype=np.int32)
    counted = np.full(nrows, 2, dtype=np.uint8)
    for r in range(nrows):
        row = codes[r]
        nm = np.flatnonzero(row != MISS)
        if nm.size == 0:
            continue
        c = 1 if row[nm[0]] == 3 else 0
        counted[r] = c
        hom = int(np.count_nonzero(row == (3 if c else 0)))
        counts[r, 0] = 2 * hom + int(np.count_nonzero(row == 2))
        counts[r, 1] = 2 * nm.size
    return counts, counted


def recode(codes, counted):
    """copies of the counted allele per genotype, -9 = missing; a row without a counted allele is all -9"""
    table = np.array([[2, -9, 1, 0], [0, -9, 1, 2], [-9, -9, -9, -9]], dtype=np.int16)
    return table[np.asarray(counted, dtype=np.int64)[:, None], np.asarray(codes, dtype=np.int64)]


def tped_census(line, missing="0"):
    """garlic-data.cpp:103-141 on one TPED line: (oneAllele, data[], nalleles, total)"""
    t = line.split()
    al = t[4:]
    nind = len(al) // 2
    one = missing
    nalleles = total = 0
    data = []
    for i in range(nind):
        v = 0
        a1, a2 = al[2 * i], al[2 * i + 1]
        if one == missing and a1 != missing:
            one = a1
        if one == missing and a2 != missing:
            one = a2
        for a in (a1, a2):
            if a == missing:
                v += -9
            elif a == one:
                v += 1
                nalleles += 1
                total += 1
            else:
                total += 1
        data.append(-9 if v < 0 else v)
    return one, np.array(data, dtype=np.int16), nalleles, total


def case_codes(n, rng, random_rows=12):
    """PLINK codes [rows][n]: rows of all missing; rows whose first non-missing genotype is hom A1, het, hom A2 -- at
    individual 0, at the LAST individual (everything before it missing), and at the first individual of the row's last
    16-byte piece (64 genotypes: the last lane's tail) with the rest behind it mixed; and random rows, some half missing"""
    rows = [np.full(n, MISS)]
    for g in (0, 2, 3):
        r = rng.integers(0, 4, size=n)
        r[0] = g
        rows.append(r)
        r = np.full(n, MISS)
        r[n - 1] = g
        rows.append(r)
        r = rng.integers(0, 4, size=n)
        tail = 64 * ((n - 1) // 64)
        r[:tail] = MISS
        r[tail] = g
        rows.append(r)
        r = rng.integers(0, 4, size=n)           # the first genotypes missing, then g: the hit inside a word
        k = min(n - 1, int(rng.integers(1, 40)))
        r[:k] = MISS
        r[k] = g
        rows.append(r)
    for k in range(random_rows):
        r = rng.integers(0, 4, size=n)
        if k % 3 == 0:
            r[rng.random(n) < 0.5] = MISS
        rows.append(r)
    rows.append(np.full(n, MISS))
    return np.array(rows, dtype=np.uint8)


def pack_rows(codes, pitch=None, garbage=True):
    """uint8 [rows][pitch]: the .bed rows (individual j at bits 2 * (j % 4) of byte j // 4).  With garbage, the bits past
    the last individual cycle through 00 / 01 / 10 / 11 patterns by row and the bytes past the row are 0xA7"""
    codes = np.asarray(codes, dtype=np.uint8)
    nrows, n = codes.shape
    rb = (n + 3) // 4
    pitch = rb if pitch is None else pitch
    padded = np.zeros((nrows, 4 * rb), dtype=np.uint8)
    padded[:, :n] = codes
    if garbage:
        padded[:, n:] = (np.arange(nrows)[:, None] + np.arange(4 * rb - n)[None, :]) % 4
    q = padded.reshape(nrows, rb, 4)
    out = np.full((nrows, pitch), 0xA7 if garbage else 0, dtype=np.uint8)
    out[:, :rb] = q[:, :, 0] | (q[:, :, 1] << 2) | (q[:, :, 2] << 4) | (q[:, :, 3] << 6)
    return out


# ---- the panel of the score tests: 3 chromosomes whose starts fall inside 16-locus words, cut from a 257-individual file
SCORE_CHR = [40, 17, 4]
SCORE_NIND_FILE = 257
SCORE_W = 5
SCORE_OFFSETS = [0, 1, 2, 3, 64, 67]
SCORE_NINDS = [1, 63, 64, 65, 130]


def score_file(rng, extra_rows=30):
    """PLINK codes [sum(SCORE_CHR) + extra_rows][257]: more file rows than the panel has loci, so that maps can drop rows"""
    n = sum(SCORE_CHR) + extra_rows
    codes = rng.integers(0, 4, size=(n, SCORE_NIND_FILE)).astype(np.uint8)
    codes[rng.random(codes.shape) < 0.05] = MISS
    codes[3] = MISS                     # a row without a counted allele
    codes[7, :70] = MISS                # first non-missing genotype behind the first block
    codes[7, 70] = 3
    return codes


def keep_all_file(rng):
    """a file of exactly as many rows as the panel has loci: dest_locus = arange keeps every row, the image's last included"""
    return score_file(rng, extra_rows=0)


def dest_maps(nrows, nloci):
    """name -> list of dest_locus arrays applied in order (each int64 [nrows], -1 = dropped).  (The variant that keeps every
    row of its file is keep_all_file with arange; "prefix" here keeps the first nloci rows of the longer file.)"""
    assert nrows - nloci >= 22
    # scattered drops: the first row, the last row, 20 consecutive rows, and the rest spread out
    drop = {0, nrows - 1} | set(range(25, 45))
    k = 50
    while len(drop) < nrows - nloci:
        drop.add(k)
        k += 5
    keep = [r for r in range(nrows) if r not in drop]
    scattered = np.full(nrows, -1, dtype=np.int64)
    scattered[keep] = np.arange(nloci)
    all_kept = np.full(nrows, -1, dtype=np.int64)          # the first nloci rows, none dropped between them
    all_kept[:nloci] = np.arange(nloci)
    # two calls that each cover a part: odd loci first, then the even ones -- every word is written twice, half each time
    first = np.where((scattered >= 0) & (scattered % 2 == 1), scattered, -1)
    second = np.where((scattered >= 0) & (scattered % 2 == 0), scattered, -1)
    return {"scattered": [scattered], "prefix": [all_kept], "two_calls": [first, second]}


def final_map(maps):
    """the file row behind every locus after the calls of one dest_maps entry"""
    out = {}
    for m in maps:
        for r in np.flatnonzero(m >= 0):
            out[int(m[r])] = int(r)
    return np.array([out[l] for l in range(len(out))], dtype=np.int64)
