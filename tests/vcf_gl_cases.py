"""The rule of garlic_tgls_set_rows_vcf restated in plain Python, its line builders, and the writer of the twin .tgls text;
importable without a GPU.

  line      ends at its first \\r or \\n (or where the caller's next offset or the slab ends); columns are separated by tabs;
            column 8 is FORMAT, keys joined by ':', and k = the index of the first key that equals `key` bytewise
  value     of sample j (column 9 + j): the column split at ':' -- subfield k.  MISSING when the column has no subfield k,
            when it is empty and when it is exactly "."; any other subfield is float(token) unless tgls_number defers it
  missing   on a column that starts with '.': missing_raw, or 0.0 when there is none; on any other column: missing_raw, or the
            offence NO_VALUE when there is none
  status    the lowest (column << 3 | code) of the line: DEFERRED / NO_VALUE at their sample column (kept columns only),
            MANY at ncols, FEW at the number of sample columns found, NO_KEY at column 0
"""
import numpy as np

import tgls_cases as tc

OK, DEFERRED, FEW, MANY, NO_KEY, NO_VALUE = 0, 1, 2, 3, 4, 5

FIXED = b"1\t%d\trs%d\tA\tG\t.\tPASS\t.\t"


def cut_line(line):
    """the bytes of the line in front of its first \\r or \\n"""
    for k, c in enumerate(line):
        if c in (0x0A, 0x0D):
            return line[:k]
    return line


def parse_line(line, ncols, key, missing_raw=None, kept=None):
    """-> (values float64 [ncols] with NaN where the rule gives none, (code, column))"""
    cols = cut_line(bytes(line)).split(b"\t")
    samples = cols[9:]
    vals = np.full(ncols, np.nan)
    offences = []
    k = None
    if len(cols) > 8:
        keys = cols[8].split(b":")
        k = keys.index(key) if key in keys else None
    if k is None:
        offences.append((0, NO_KEY))
    if len(samples) < ncols:
        offences.append((len(samples), FEW))
    if len(samples) > ncols:
        offences.append((ncols, MANY))
    for j, col in enumerate(samples[:ncols]):
        if k is None or (kept is not None and j not in kept):
            continue
        sub = col.split(b":")
        tok = sub[k] if k < len(sub) else b""
        if tok in (b"", b"."):
            if missing_raw is not None:
                vals[j] = missing_raw
            elif col.startswith(b"."):
                vals[j] = 0.0
            else:
                offences.append((j, NO_VALUE))
        elif tc.defers(tok):
            offences.append((j, DEFERRED))
        else:
            vals[j] = float(tok)
    status = (0, 0)
    if offences:
        column, code = min(offences)
        status = (code, column)
    return vals, status


def parse_slab(text, lb, ncols, key, missing_raw=None, col_idx=None):
    """-> (raw float64 [rows][n_kept], NaN where the rule gives no value; status int32 [rows][2])"""
    text = bytes(text)
    idx = np.arange(ncols) if col_idx is None else np.asarray(col_idx)
    kept = set(int(c) for c in idx)
    rows = len(lb) - 1
    raw = np.full((rows, len(idx)), np.nan)
    status = np.zeros((rows, 2), dtype=np.int32)
    for r in range(rows):
        vals, status[r] = parse_line(text[int(lb[r]):min(int(lb[r + 1]), len(text))], ncols, key, missing_raw, kept)
        raw[r] = vals[idx]
    return raw, status


def twin_tgls(text, lb, ncols, key, missing_raw=None):
    """the .tgls lines that hold the same tokens: the subfield as it stands, or `0` / the missing value where the rule
    substitutes one.  Every line must be clean under the rule but for deferred tokens, which are copied too."""
    text = bytes(text)
    lines = []
    for r in range(len(lb) - 1):
        cols = cut_line(text[int(lb[r]):min(int(lb[r + 1]), len(text))]).split(b"\t")
        k = cols[8].split(b":").index(key)
        toks = []
        for col in cols[9:9 + ncols]:
            sub = col.split(b":")
            tok = sub[k] if k < len(sub) else b""
            if tok in (b"", b"."):
                assert missing_raw is not None or col.startswith(b"."), (r, col)
                tok = repr(float(missing_raw)).encode() if missing_raw is not None else b"0"
            toks.append(tok)
        lines.append(tc.plain_line(r, toks))
    return lines


# ---- builders
def sample_column(gt, subs):
    """a sample column: the genotype and the subfields behind it; None in `subs` from some index on = dropped from there"""
    out = [gt]
    for s in subs:
        if s is None:
            break
        out.append(s)
    return b":".join(out)


def data_line(r, fmt_keys, columns, eol=b"\n"):
    return FIXED % (100 + r, r) + b":".join(fmt_keys) + b"\t" + b"\t".join(columns) + eol


def pl_list(rng):
    """a neighbouring subfield of more than 48 bytes"""
    return b",".join(b"%d" % v for v in rng.integers(0, 10 ** 9, size=int(rng.integers(6, 12))))


FORMATS = [                                 # (keys, position of GQ)
    ([b"GT", b"GQ"], 1),
    ([b"GT", b"DP", b"GQ"], 2),
    ([b"GT", b"GQ", b"PL"], 1),
    ([b"GT", b"AD", b"DP", b"PL", b"GQ"], 4),
    ([b"GT", b"GQX", b"GQ", b"QG"], 2),     # keys that contain the key, or are contained in it
]


def random_lines(rng, rows, nind, tokens, key=b"GQ", eols=(b"\n",), drop=0.1, last_eol=b""):
    """`rows` data lines of nind samples whose key value is tokens[r][j]; FORMAT changes from line to line; the other
    subfields are short numbers or long lists; with probability `drop` a sample with a missing genotype drops its trailing
    subfields, writes '.' or nothing.  -> lines"""
    lines = []
    for r in range(rows):
        keys, pos = FORMATS[r % len(FORMATS)]
        keys = [key if x == b"GQ" else x for x in keys]
        cols = []
        for j in range(nind):
            called = rng.random() >= drop
            gt = (b"0/0", b"0|1", b"1|0", b"1/1")[int(rng.integers(0, 4))] if called else b"./."
            subs = []
            for i, name in enumerate(keys[1:], start=1):
                if i == pos:
                    subs.append(tokens[r][j])
                elif name == b"PL" or name == b"AD":
                    subs.append(pl_list(rng) if rng.random() < 0.3 else b"0,1")
                else:
                    subs.append(b"%d" % rng.integers(0, 500))
            if not called:
                how = int(rng.integers(0, 4))
                if how == 0:
                    subs[pos - 1:] = [None]                   # the key's subfield and what follows are dropped
                elif how == 1:
                    subs[pos - 1] = b"."
                elif how == 2:
                    subs[pos - 1] = b""
            cols.append(sample_column(gt, subs))
        eol = last_eol if r == rows - 1 else eols[r % len(eols)]
        lines.append(data_line(r, keys, cols, eol))
    return lines


# ---- device text (the GPU tests only: torch and the binding are imported where they are used)
class DeviceSlab:
    """the text at `offset` bytes past a 16-byte aligned device address, with 64 bytes of `poison` on each side"""

    def __init__(self, text, offset, poison):
        import torch
        self.buf = torch.full((len(text) + 160,), poison, dtype=torch.uint8, device="cuda")
        base = self.buf.data_ptr()
        self.at = (-base) % 16 + 64 + offset
        self.buf[self.at:self.at + len(text)] = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
        torch.cuda.synchronize()
        self.ptr = base + self.at
        assert self.ptr % 16 == offset


def feed(obj, text, lb, where="host", row_begin=0, key=b"GQ", missing_raw=None, poison=0x3A):
    """-> (status, err); where: "host", or "devN" = device text N bytes past an aligned address, with `poison` (':') around"""
    from garlic_amd import abi
    if where == "host":
        return obj.set_rows_vcf(text, lb, key, missing_raw=missing_raw, row_begin=row_begin)
    slab = DeviceSlab(text, int(where[3:]), poison)
    return obj.set_rows_vcf(slab.ptr, lb, key, missing_raw=missing_raw, row_begin=row_begin, text_bytes=len(text), where=abi.DEVICE)
