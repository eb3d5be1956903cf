"""Lines for garlic_tgls_set_rows_vcf whose events -- FORMAT and its key, a sample column's first byte, its k-th colon, its
closing tab, the line's end -- stand on chosen bytes of tgls_vcf_parse_kernel's passes; importable without a GPU.

A pass is PIECES pieces of PIECE bytes and begins at the piece that holds the line's first byte, so the offset of a byte in
its pass is (offset of the line's first byte in its piece) + (index in the line) modulo P.  place() pads one field in front
of a named byte until the byte stands on `target`; the pad is always longer than the look-ahead of LOOK bytes, so nothing in
front of it can be seen from the byte.  Every builder returns the slab with one mark per row: what was planted where, for
tests/test_vcf_gl_borders_cpu.py to check against the bytes."""
import numpy as np

import tgls_cases as tc
import vcf_gl_cases as vg

P = tc.PASS_BYTES
PIECES = 256                        # pieces of a pass, one per lane of the workgroup
PIECE = P // PIECES                 # bytes of a piece: one 16-byte load
LOOK = 3 * PIECE                    # the three slots behind its own that a value may reach: what a pass carries to the next
BORDER = list(range(P - 50, P + 18)) + [2 * P - 1, 2 * P, 2 * P + 1]
ALIGNS = list(range(PIECE))
HEAD = b"1\t%d\trs%d\tA\tG\t.\tPASS\t"
INFO_FILL = b"DP=14;GQ:AF=0.5,GQ;Q=:GQ:;"          # colons and the key's letters outside column 8 decide nothing
SUB_FILL = b"0,12,345,"
EOLS = (b"\n", b"\r\n", b"")
KEY = b"GQ"
VALUES = [b"7", b"0" * 15 + b"17", b"0" * 28 + b"12.5", b"0" * 29 + b"12.5"]      # 1, 17, 32 and 33 bytes; 33 defer
assert [len(v) for v in VALUES] == [1, 17, 32, tc.TOKEN_MAX + 1] and LOOK == 48 and PIECE == 16


def fill(pattern, n, lead=b""):
    n -= len(lead)
    assert n >= 0
    return lead + (pattern * (n // len(pattern) + 1))[:n]


class Line:
    """a data line: INFO, FORMAT's keys, the sample columns as lists of subfields, the EOL"""

    def __init__(self, r, keys, columns, info=b".", eol=b"\n"):
        self.r, self.keys, self.columns, self.info, self.eol = r, list(keys), [list(c) for c in columns], info, eol

    def _parts(self):
        return HEAD % (100 + self.r, self.r), b":".join(self.keys), [b":".join(c) for c in self.columns]

    def text(self):
        head, fmt, cols = self._parts()
        return head + self.info + b"\t" + fmt + b"\t" + b"\t".join(cols) + self.eol

    def at(self, name):
        """the index in the line of a named byte:
        ("format",) FORMAT's first byte; ("key", i, "first" | "last") of FORMAT's key i; ("format_tab",) the tab behind FORMAT;
        ("column", j) sample j's first byte; ("colon", j, n) its n-th colon, n >= 1; ("value", j, i) the first byte of its
        subfield i; ("column_tab", j) the byte behind it: its tab or the line's end; ("eol",) the first byte of the EOL = the
        line's length without it; ("end",) one past the line's last byte, EOL included = the line's length"""
        head, fmt, cols = self._parts()
        f0 = len(head) + len(self.info) + 1
        kind = name[0]
        if kind == "format":
            return f0
        if kind == "key":
            b = f0 + sum(len(x) + 1 for x in self.keys[:name[1]])
            return b if name[2] == "first" else b + len(self.keys[name[1]]) - 1
        if kind == "format_tab":
            return f0 + len(fmt)
        if kind == "eol":
            return len(self.text()) - len(self.eol)
        if kind == "end":
            return len(self.text())
        j = name[1]
        b = f0 + len(fmt) + 1 + sum(len(x) + 1 for x in cols[:j])
        if kind == "column":
            return b
        if kind == "column_tab":
            return b + len(cols[j])
        if kind == "colon":
            return b + sum(len(x) + 1 for x in self.columns[j][:name[2]]) - 1
        assert kind == "value"
        return b + sum(len(x) + 1 for x in self.columns[j][:name[2]])

    def set_pad(self, where, n, lead=b""):
        if where == "info":
            self.info = fill(INFO_FILL, n, lead)
        else:
            self.columns[where[0]][where[1]] = fill(SUB_FILL, n, lead)


def place(line, name, target, first, where="info", lead=b""):
    """pads INFO (where="info") or subfield i of sample j (where=(j, i); never the key's) so that the named byte stands
    `target` bytes into the pass that holds the line's first byte at offset `first` (< PIECE).  lead: the pad's first bytes"""
    assert 0 <= first < PIECE
    line.set_pad(where, LOOK + 1, lead)
    before = line.at(name)
    need = target - first - before
    assert need >= 0, (name, target, first, before)
    line.set_pad(where, LOOK + 1 + need, lead)
    assert first + line.at(name) == target and line.at(name) == before + need, (name, target)      # the pad stood in front
    return line


class Slab:
    """lines back to back, as they will stand `align` bytes behind a 16-byte aligned address"""

    def __init__(self, align):
        self.align, self.text, self.lb, self.marks = align, bytearray(), [], []

    def first(self):
        """where the next line's first byte will stand in its first pass"""
        return (len(self.text) + self.align) % PIECE

    def add(self, line, **mark):
        """line: a Line or bytes; mark: what the CPU test checks.  name + target: the named byte of a Line stands on target"""
        data = line.text() if isinstance(line, Line) else bytes(line)
        mark["first"] = self.first()
        if "name" in mark and "index" not in mark:
            mark["index"] = line.at(mark["name"])
        self.lb.append(len(self.text))
        self.text += data
        self.marks.append(mark)

    def done(self):
        return bytes(self.text), np.array(self.lb + [len(self.text)], dtype=np.int64), self.marks


def number(r, j, i):
    """a short value that differs between the subfields of a column, the columns of a line and neighbouring lines"""
    return b"%d" % (100 + (37 * r + 11 * j + 3 * i) % 9000)


# ------------------------------------------------------------------------------------------------ a. FORMAT anywhere
KEYS = [b"Q", b"GQ", b"GL_0123456789.ab"]
assert [len(k) for k in KEYS] == [1, 2, 16]
POSITIONS = ("first", "middle", "last")
FORMAT_BYTES = (("format",), ("key", "first"), ("key", "last"), ("format_tab",))


def decoys(key):
    """keys that contain the key or are contained in it: GQX, G, QG and GY for GQ"""
    out = [key + b"X", key[:1] if len(key) > 1 else b"G", key[::-1] if key[::-1] != key else b"QG", key[:-1] + b"Y"]
    assert key not in out and b"GT" not in out
    return out


def format_keys(key, position, r):
    d = decoys(key)
    d1, d2 = d[r % 4], d[(r + 1 + r // 4 % 3) % 4]
    return {"first": [key, d1, d2, b"GT"], "middle": [b"GT", d1, key, d2], "last": [b"GT", d1, d2, key]}[position]


def format_columns(r, keys, nind=3):
    return [[b"0/1" if name == b"GT" else number(r, j, i) for i, name in enumerate(keys)] for j in range(nind)]


def fmt_spans(line, first):
    """(key, first byte, last byte) of every FORMAT key as offsets in the pass"""
    return [(k, first + line.at(("key", i, "first")), first + line.at(("key", i, "last"))) for i, k in enumerate(line.keys)]


def format_slab(key, align):
    """FORMAT's first byte, the key's first and last byte and the tab behind FORMAT on every offset of BORDER, the key first,
    in the middle and last among decoys; one FORMAT wholly in the third pass; one that names the key twice around the
    border.  Clean throughout.  -> (text, lb, marks, nind)"""
    s, r = Slab(align), 0
    for what in FORMAT_BYTES:
        for position in POSITIONS:
            for target in BORDER:
                keys = format_keys(key, position, r)
                name = ("key", keys.index(key), what[1]) if what[0] == "key" else what
                line = place(Line(r, keys, format_columns(r, keys)), name, target, s.first())
                s.add(line, name=name, target=target, position=position, spans=fmt_spans(line, s.first()))
                r += 1
    keys = format_keys(key, "middle", r)
    line = place(Line(r, keys, format_columns(r, keys)), ("format",), 2 * P + 100, s.first())
    s.add(line, name=("format",), target=2 * P + 100, spans=fmt_spans(line, s.first()))
    r += 1
    for target in (P - 1, P, P + 1):                      # the key twice, the second one's first byte on the target
        keys = [b"GT", key, decoys(key)[0], key]
        line = place(Line(r, keys, format_columns(r, keys)), ("key", 3, "first"), target, s.first())
        s.add(line, name=("key", 3, "first"), target=target, twice=True, spans=fmt_spans(line, s.first()))
        r += 1
    return s.done() + (3,)


def no_key_slab(key, align):
    """a FORMAT of decoys only whose every byte in turn straddles the border, between clean lines: NO_KEY at column 0"""
    s, r = Slab(align), 0
    d = decoys(key)
    for target in range(P - 2, P + LOOK):
        keys = [b"GT", d[r % 4], d[(r + 1) % 4], d[(r + 2) % 4]] if r % 2 else format_keys(key, "last", r)
        line = place(Line(r, keys, format_columns(r, keys)), ("format_tab",), target, s.first())
        s.add(line, name=("format_tab",), target=target, no_key=bool(r % 2), spans=fmt_spans(line, s.first()))
        r += 1
    return s.done() + (3,)


# ------------------------------------------------------------------------------------------------ b. the key first: k == 0
FIRST_KEYS = [KEY, b"GT", b"DP"]
FIRST_FORMS = [[v, b"0/1", b"5"] for v in VALUES] + [
    [b"."], [b""], [b".", b"3"], [b"", b"3"], [b"8"], [b".", b"./.", b"4"], [b"", b"./."]]
# the status of a line whose sample 1 is the form, without a missing value; with one only the 33 bytes still offend
FIRST_STATUS = [[0, 0], [0, 0], [0, 0], [vg.DEFERRED, 1], [0, 0], [vg.NO_VALUE, 1], [0, 0], [vg.NO_VALUE, 1], [0, 0], [0, 0],
                [vg.NO_VALUE, 1]]
FIRST_VALUE = [7.0, 17.0, 12.5, None, 0.0, None, 0.0, None, 8.0, 0.0, None]       # of sample 1, without a missing value


def key_first_slab(align, forms=FIRST_FORMS):
    """FORMAT GQ:GT:DP; sample 1 is each form in turn with its first byte on every offset of BORDER; the pad is sample 0's DP.
    -> (text, lb, marks, nind)"""
    s, r = Slab(align), 0
    for target in BORDER:
        for f, form in enumerate(forms):
            cols = [[number(r, 0, 0), b"0/1", b""], form, [number(r, 2, 0), b"1/1", b"9"]]
            line = place(Line(r, FIRST_KEYS, cols), ("column", 1), target, s.first(), where=(0, 2))
            s.add(line, name=("column", 1), target=target, form=f)
            r += 1
    return s.done() + (3,)


UNKEPT_FORMS = [[b"1,2,3", b"0/1", b"5"], [b""], [b"0" * 40], [b":"]]


# ------------------------------------------------------------------------------------------------ c. state carried over passes
CARRY_KS = (1, 2, 4)
FILLERS = [b"AD", b"DP", b"PL"]
COLON_TARGETS = [P - 1, P, P + 100, 2 * P - 1, 2 * P + 100]          # the pass behind the column's and the one after that
START = P - 200                                                       # where the carried column begins: in the first pass


def carry_keys(k):
    return [b"GT"] + FILLERS[:k - 1] + [KEY, b"PP", b"XX"]


def carried_slab(k, align):
    """the key at index k.  Sample 1 begins at START in the first pass; what decides its value stands in a later pass.
    -> (text, lb, marks, nind); every mark names its case"""
    s, r = Slab(align), 0
    keys = carry_keys(k)

    def others(r):
        col0 = [b"0/1"] + [number(r, 0, i) for i in range(1, k + 1)] + [b""]        # its PP is the pad that sets START
        col2 = [b"1/1"] + [number(r, 2, i) for i in range(1, k + 1)]
        return col0, col2

    def front(dot):
        """sample 1 up to the subfield in front of the key's, which is the pad -> (subfields, the pad's lead)"""
        if k == 1:
            return [b""], b"." if dot else b"0/1"
        return [b"./." if dot else b"0|1"] + [number(r, 1, i) for i in range(1, k - 1)] + [b""], b""

    def add(col1, name, target, case, **more):
        nonlocal r
        col0, col2 = others(r)
        line = Line(r, keys, [col0, col1, col2])
        line.set_pad((1, k - 1), LOOK + 1, more.get("lead", b""))
        place(line, ("column", 1), START, s.first(), where=(0, k + 1))
        place(line, name, target, s.first(), where=(1, k - 1), lead=more.get("lead", b""))
        assert s.first() + line.at(("column", 1)) == START
        s.add(line, name=name, target=target, case=case, dot=more.get("dot", False))
        r += 1

    for target in COLON_TARGETS:
        for dot in (False, True):
            sub, lead = front(dot)
            add(sub + [number(r, 1, k)], ("colon", 1, k), target, "value", lead=lead, dot=dot)
            add(sub + [b"."], ("colon", 1, k), target, "dot", lead=lead, dot=dot)
            add(sub + [b""], ("colon", 1, k), target, "empty", lead=lead, dot=dot)
            add(sub, ("column_tab", 1), target, "dropped", lead=lead, dot=dot)
        # more than k colons: the value and two colons behind it in the first pass, one more colon in the later pass
        sub, lead = front(False)
        col0, col2 = others(r)
        col1 = (sub[:-1] + [b"3"] if k > 1 else [b"0/1"]) + [number(r, 1, k), b"", b"77"]
        line = Line(r, keys, [col0, col1, col2])
        line.set_pad((1, k + 1), LOOK + 1)
        place(line, ("column", 1), START, s.first(), where=(0, k + 1))
        place(line, ("colon", 1, k + 2), target, s.first(), where=(1, k + 1))
        s.add(line, name=("colon", 1, k + 2), target=target, case="once", dot=False)
        r += 1
    # fewer than k colons, the closing tab on every offset of BORDER; then the same as the line's last column with each EOL
    for target in BORDER:
        for dot in (False, True):
            sub, lead = front(dot)
            col0, col2 = others(r)
            line = Line(r, keys, [col0[:-1], sub, col2])
            place(line, ("column_tab", 1), target, s.first(), where=(1, k - 1), lead=lead)
            s.add(line, name=("column_tab", 1), target=target, case="short", dot=dot)
            r += 1
            for eol in EOLS:
                col0, col2 = others(r)
                line = Line(r, keys, [col0[:-1], col2, sub], eol=eol)
                place(line, ("column_tab", 2), target, s.first(), where=(2, k - 1), lead=lead)
                s.add(line, name=("column_tab", 2), target=target, case="short last", dot=dot, eol=eol)
                r += 1
    return s.done() + (3,)


# ------------------------------------------------------------------------------------------------ d. line ends
END_LENGTHS = [P - 1, P, P + 1, 2 * P] + [P + PIECE * k - 1 for k in (1, 2, 3)]
END_KEYS = [b"GT", b"DP", KEY]
REST = b"9\t0/1:1:2\n"              # what stands behind a cut: read, it would change the last value and add a column
# (variant, status without a missing value, status with one)
END_VARIANTS = [("value", [0, 0], [0, 0]), ("short", [vg.NO_VALUE, 2], [0, 0]), ("short dot", [0, 0], [0, 0]),
                ("tab full", [vg.MANY, 3], [vg.MANY, 3]), ("tab less", [vg.NO_VALUE, 2], [0, 0]), ("cut", [0, 0], [0, 0])]


def end_line(r, variant, eol):
    full = [[b"0/1", b"", number(r, 0, 2)], [b"0|1", b"3", number(r, 1, 2)], [b"1/1", b"4", number(r, 2, 2)]]
    cols = {"value": full, "cut": full, "short": full[:2] + [[b"0/1"]], "short dot": full[:2] + [[b"./."]],
            "tab full": full + [[b""]], "tab less": full[:2] + [[b""]]}[variant]
    return Line(r, END_KEYS, cols, eol=eol)


def end_cases():
    """every variant with every EOL ("cut": none; its row ends in front of REST) at every length of END_LENGTHS.  in_pass: the
    length is not the line's but the offset in its pass of the byte behind it, which differs where the line does not begin
    a piece"""
    for variant, st, st_missing in END_VARIANTS:
        for eol in (EOLS if variant != "cut" else (b"",)):
            for length in END_LENGTHS:
                for in_pass in (False, True):
                    yield dict(variant=variant, eol=eol, length=length, in_pass=in_pass, status=st, status_missing=st_missing)


def end_rows(first_of):
    """first_of(bytes so far) -> where the next line's first byte will stand in its piece.
    -> [(the row's bytes, the bytes behind it that are not the row's, mark)]"""
    out, size = [], 0
    for r, case in enumerate(end_cases()):
        first = first_of(size)
        target = case["length"] if case["in_pass"] else first + case["length"]
        line = place(end_line(r, case["variant"], case["eol"]), ("end",), target, first, where=(0, 1))
        rest = REST if case["variant"] == "cut" else b""
        out.append((line.text(), rest, dict(case, name=("end",), target=target, first=first, index=line.at(("end",)))))
        size += len(line.text()) + len(rest)
    return out


def line_end_slab(align):
    """end_rows() back to back, each followed by another line; REST behind a cut is a row of its own (FEW at 0) and a clean
    line closes the slab.  -> (text, lb, marks, nind)"""
    s = Slab(align)
    for data, rest, mark in end_rows(lambda size: (size + align) % PIECE):
        assert s.first() == mark["first"]
        s.add(data, **{k: v for k, v in mark.items() if k != "first"})
        if rest:
            s.add(rest, rest=True)
    s.add(end_line(9999, "value", b"\n").text(), closing=True)
    return s.done() + (3,)


# ------------------------------------------------------------------------------------------------ e. offences decided late
D33 = VALUES[3]
# (name, the three sample columns or fewer or more, (named byte, its target, the pad), status without a missing value)
LATE = [
    ("a column too many that starts in the third pass",
     [[b"0/1", b"3", b"41"], [b"0/1", b"3", b"42"], [b"1/1", b"", b"43"], [b"0/0", b"1", b"44"]], (("column", 3), 2 * P + 10, (2, 1)),
     [vg.MANY, 3]),
    ("a column too few on a line of three passes",
     [[b"0/1", b"3", b"41"], [b"0/1", b"", b"42"]], (("end",), 2 * P + 300, (1, 1)), [vg.FEW, 2]),
    ("deferred in the first pass, too few found in the third",
     [[b"0/1", b"3", D33], [b"0/1", b"", b"42"]], (("end",), 2 * P + 300, (1, 1)), [vg.DEFERRED, 0]),
    ("deferred at column 1 in the first pass, a column too many in the third",
     [[b"0/1", b"3", b"41"], [b"0/1", b"3", D33], [b"1/1", b"", b"43"], [b"0/0", b"1", b"44"]], (("column", 3), 2 * P + 10, (2, 1)),
     [vg.DEFERRED, 1]),
    ("DEFERRED at column 0 in the first pass, NO_VALUE at column 2 in the third",
     [[b"0/1", b"3", D33], [b"0/1", b"", b"42"], [b"1/1", b"4"]], (("column", 2), 2 * P + 10, (1, 1)), [vg.DEFERRED, 0]),
    ("NO_VALUE at column 0 in the first pass, DEFERRED at column 2 in the third",
     [[b"0/1", b"3"], [b"0/1", b"", b"42"], [b"1/1", b"4", D33]], (("column", 2), 2 * P + 10, (1, 1)), [vg.NO_VALUE, 0]),
    ("NO_VALUE at column 2, closed by the line's end in the third pass",
     [[b"0/1", b"3", b"41"], [b"0/1", b"", b"42"], [b"1/1", b"4"]], (("end",), 2 * P + 300, (1, 1)), [vg.NO_VALUE, 2]),
    ("clean over three passes",
     [[b"0/1", b"3", b"41"], [b"0/1", b"", b"42"], [b"1/1", b"4", b"43"]], (("end",), 2 * P + 300, (1, 1)), [0, 0]),
]
LATE_WITH_MISSING = [[vg.MANY, 3], [vg.FEW, 2], [vg.DEFERRED, 0], [vg.DEFERRED, 1], [vg.DEFERRED, 0], [vg.DEFERRED, 2], [0, 0], [0, 0]]


def late_slab(align):
    """-> (text, lb, marks, nind)"""
    s = Slab(align)
    for r, (what, cols, (name, target, where), status) in enumerate(LATE):
        line = place(Line(r, END_KEYS, cols), name, target, s.first(), where=where)
        s.add(line, name=name, target=target, what=what, status=status)
    return s.done() + (3,)
