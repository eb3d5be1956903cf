"""Feature counts per ROH class (garlic_feature_counts, garlic-lod --features): the semantics of the reference's
src/count_features_in_roh.pl restated in numpy, the golden cases of tests/golden/features/ and generators for random cases.
Importable without a GPU.

The rule: a hom row (chromosome, position, effect, one bit per individual) counts for every individual whose bit is set, into
the class of that individual's interval with chr == the row's and start <= position < stop (stop is the `end` column of a
.roh.bed line; the script tests position <= end - 1), else into NONE, the class with index n_classes."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "features")
GOLDEN_CASES = ["case1", "case2"]
CHUNK = 4096        # FEAT_CHUNK_ROWS
GROUP = 32          # effects per launch
CAP = 256           # GARLIC_FEATURE_MAX_EFFECTS
INTERVAL = np.dtype([("ind", "<i4"), ("chr", "<i4"), ("start", "<i4"), ("stop", "<i4"), ("cls", "<i4")])


def unpack(bits, nind):
    """[nrows, nind] bool of LSB-first bit rows"""
    return np.unpackbits(np.ascontiguousarray(bits, dtype=np.uint8), axis=1, bitorder="little")[:, :nind].astype(bool)


def pack(hom):
    """LSB-first bit rows of [nrows, nind] bool"""
    if hom.shape[0] == 0:
        return np.zeros((0, (hom.shape[1] + 7) // 8), dtype=np.uint8)
    return np.packbits(hom, axis=1, bitorder="little")


def expected_counts(hom, chr_, pos, effect, intervals, nind, n_classes, n_effects):
    """int64 [nind, n_classes + 1, n_effects]: searchsorted over each individual's intervals.  intervals: INTERVAL array in
    (ind, chr, start) order, not overlapping within an individual."""
    out = np.zeros((nind, n_classes + 1, n_effects), dtype=np.int64)
    chr_, pos, effect = (np.asarray(v, dtype=np.int64) for v in (chr_, pos, effect))
    key = chr_ * (1 << 32) + pos
    for i in range(nind):
        rows = np.nonzero(hom[:, i])[0]
        if rows.shape[0] == 0:
            continue
        iv = intervals[intervals["ind"] == i]
        cls = np.full(rows.shape[0], n_classes, dtype=np.int64)
        if iv.shape[0]:
            starts = iv["chr"].astype(np.int64) * (1 << 32) + iv["start"]
            stops = iv["chr"].astype(np.int64) * (1 << 32) + iv["stop"]
            at = np.searchsorted(starts, key[rows], side="right") - 1        # the last interval that starts at or before the row
            ok = at >= 0
            inside = ok & (key[rows] < stops[np.maximum(at, 0)]) & (iv["chr"][np.maximum(at, 0)] == chr_[rows])
            cls[inside] = iv["cls"][at[inside]]
        np.add.at(out[i], (cls, effect[rows]), 1)
    return out


# ---- the golden cases: the script's inputs read with plain Python, as the script reads them

def golden_path(case, what):
    return os.path.join(GOLDEN, "%s.%s" % (case, what))


def golden_tped_lines(case):
    """the lines of the per-chromosome files in the script's order (22, 23) with the chromosome the file NAME gives"""
    lines = []
    for c in (22, 23):
        for line in open(golden_path(case, "chr%d.tped" % c)).read().splitlines():
            lines.append(("chr%d" % c, line))
    return lines


def golden_table(case):
    """the table of a golden case from the restatement, as the script prints it (three classes)"""
    effect_of, effects = {}, set()
    for line in open(golden_path(case, "features.txt")).read().splitlines():
        chrpos, _ref, allele, effect = line.split()
        c, p = chrpos.split(":")
        effect_of[(c, int(p), allele)] = effect
        effects.add(effect)
    effects = sorted(effects)
    iid = [line.split()[1] for line in open(golden_path(case, "chr22.tfam")).read().splitlines()]
    chr_id = {"chr22": 0, "chr23": 1}
    rows = []
    for c, line in golden_tped_lines(case):
        f = line.split()
        p, g = int(f[3]), f[4:]
        for (kc, kp, allele), effect in sorted(effect_of.items()):
            if (kc, kp) != (c, p):
                continue
            hom = [g[2 * i] != "0" and g[2 * i] == allele and g[2 * i + 1] == allele for i in range(len(iid))]
            rows.append((chr_id[c], p, effects.index(effect), hom))
    rows.sort(key=lambda r: (r[0], r[1]))
    iv, ind = [], None
    for line in open(golden_path(case, "roh.bed")).read().splitlines():
        m = re.match(r"^track .+Ind: (.+) Pop:(.+) ROH.+", line)
        if m:
            ind = iid.index(m.group(1)) if m.group(1) in iid else None
            continue
        f = line.split()
        if ind is not None:
            iv.append((ind, chr_id[f[0]], int(f[1]), int(f[2]), "ABC".index(f[3])))
    iv = np.array(sorted(iv), dtype=INTERVAL)
    hom = np.array([r[3] for r in rows], dtype=bool).reshape(len(rows), len(iid))
    counts = expected_counts(hom, [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], iv, len(iid), 3, len(effects))
    return table_text(effects, iid, counts, 3)


def table_text(effects, iid, counts, n_classes):
    head = "".join("%s%s " % (e, k) for e in effects for k in [chr(ord("A") + c) for c in range(n_classes)] + ["NONE"])
    lines = [head]
    for i, name in enumerate(iid):
        lines.append(name + "".join(" %d" % counts[i, c, e] for e in range(len(effects)) for c in range(n_classes + 1)))
    return "\n".join(lines) + "\n"


def read_table(path):
    """(column names, {iid: counts}) of a feature.counts file"""
    lines = open(path).read().split("\n")
    assert lines[-1] == "" and lines[0].endswith(" ")
    return lines[0].split(), {f[0]: [int(v) for v in f[1:]] for f in (line.split() for line in lines[1:-1])}


# ---- random cases

def random_case(seed, nind, nrows, n_classes, n_effects, nchr=3, density=0.05, many=40, straddle=None):
    """(hom [nrows, nind] bool, chr, pos, effect, intervals).  Rows: sorted by (chr, pos), some positions twice with different
    effects, one chromosome (1 or 2) of 0 .. nchr without intervals, chromosome nchr + 1 with intervals and no rows, the first and the
    last row all ones and all zeros.  Intervals: individual 0 none, 1 one, the others up to `many`, with empty ones
    (start == stop), adjacent ones of different classes, and edges on row positions.  straddle: a row index; individual 1's
    interval then runs from three rows before it to three rows behind it."""
    rng = np.random.default_rng(seed)
    chr_ = np.sort(rng.integers(0, nchr + 1, nrows)).astype(np.int32)
    pos = np.zeros(nrows, dtype=np.int32)
    for c in range(nchr + 1):
        m = chr_ == c
        pos[m] = np.sort(rng.integers(1, 200000, int(m.sum())))
    if nrows > 3:          # two rows at one position
        twin = rng.integers(1, nrows, max(1, nrows // 50))
        twin = twin[chr_[twin] == chr_[twin - 1]]
        pos[twin] = pos[twin - 1]
    effect = rng.integers(0, n_effects, nrows).astype(np.int32)
    if nrows > 3 and n_effects > 1:
        effect[twin] = (effect[twin - 1] + 1) % n_effects
    if nrows:
        effect[rng.integers(0, nrows)] = n_effects - 1             # the last effect occurs
    hom = rng.random((nrows, nind)) < density
    if nrows > 1:
        hom[0], hom[-1] = True, False
    iv = []
    one_chr = int(chr_[straddle if straddle is not None else 0]) if nrows else 0     # where individual 1's interval lies
    bare = 1 if one_chr != 1 else 2                                                  # rows and no intervals
    for i in range(1, nind):
        n = 1 if i == 1 else int(rng.integers(0, many + 1))
        for c in [k for k in range(nchr + 2) if k != bare]:
            if i == 1 and c != one_chr:
                continue
            cuts = np.sort(rng.integers(0, 200000, 2 * n))
            rows_c = pos[chr_ == c]
            if rows_c.shape[0] and n:          # edges on row positions: start == p, stop == p, stop == p + 1
                cuts[rng.integers(0, 2 * n, min(4, 2 * n))] = rows_c[rng.integers(0, rows_c.shape[0], min(4, 2 * n))] + rng.integers(0, 2, min(4, 2 * n))
                cuts = np.sort(cuts)
            for k in range(n):
                a, b = int(cuts[2 * k]), int(cuts[2 * k + 1])
                if k and rng.random() < 0.3:
                    a = int(cuts[2 * k - 1])           # adjacent to the one before
                if rng.random() < 0.1:
                    b = a                              # empty
                iv.append((i, c, a, max(a, b), int(rng.integers(0, n_classes))))
    iv = np.array(sorted(iv, key=lambda v: v[:3]), dtype=INTERVAL)
    if straddle is not None and nrows and nind > 1:
        lo, hi = max(straddle - 3, 0), min(straddle + 3, nrows - 1)
        while chr_[lo] != chr_[straddle]:
            lo += 1
        while chr_[hi] != chr_[straddle]:
            hi -= 1
        iv = iv[iv["ind"] != 1]
        one = np.array([(1, chr_[straddle], pos[lo], pos[hi] + 1, n_classes - 1)], dtype=INTERVAL)
        iv = np.concatenate([iv, one])
        iv = iv[np.lexsort((iv["start"], iv["chr"], iv["ind"]))]
    iv = drop_overlaps(iv)
    # adjacent intervals of one individual get different classes where there are two
    if n_classes > 1:
        for k in range(1, iv.shape[0]):
            a, b = iv[k - 1], iv[k]
            if a["ind"] == b["ind"] and a["chr"] == b["chr"] and a["stop"] == b["start"] and a["cls"] == b["cls"]:
                iv["cls"][k] = (a["cls"] + 1) % n_classes
    return hom, chr_, pos, effect, iv


def drop_overlaps(iv):
    keep, last = [], None
    for k in range(iv.shape[0]):
        v = iv[k]
        if last is not None and last["ind"] == v["ind"] and last["chr"] == v["chr"] and v["start"] < last["stop"]:
            continue
        keep.append(k)
        last = v
    return iv[keep]
