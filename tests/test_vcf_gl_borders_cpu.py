"""No GPU: the lines of tests/vcf_gl_border_cases.py.  Geometry: the named byte of every line stands on its target in the
pass, whatever the alignment and the lines in front.  Rule: what vg.parse_slab answers for them, spelled out here, so that
tests/test_gpu_vcf_gl_borders.py compares the kernel with answers a reader can see and a change of the rule cannot move both
sides unseen."""
import numpy as np
import pytest

import vcf_gl_border_cases as bc
import vcf_gl_cases as vg

P = bc.P


def check_geometry(slab, align):
    """every mark with a name: the line's first byte stands at `first` in its piece and the named byte on `target`"""
    text, lb, marks, nind = slab
    assert len(marks) == len(lb) - 1
    for r, mark in enumerate(marks):
        assert (int(lb[r]) + align) % bc.PIECE == mark["first"]
        if "name" not in mark:
            continue
        row = text[int(lb[r]):int(lb[r + 1])]
        i, kind = mark["index"], mark["name"][0]
        assert mark["first"] + i == mark["target"], mark
        at, front = row[i:i + 1], row[i - 1:i]
        if kind == "format":
            assert front == b"\t" and row[:i].count(b"\t") == 8 and at not in b"\t:", mark
        elif kind == "key":
            assert row[:i].count(b"\t") == 8, mark
            assert front in (b"\t", b":") if mark["name"][2] == "first" else row[i + 1:i + 2] in (b"\t", b":"), mark
        elif kind == "format_tab":
            assert at == b"\t" and row[:i].count(b"\t") == 8, mark
        elif kind == "column":
            assert front == b"\t" and row[:i].count(b"\t") == 9 + mark["name"][1], mark
        elif kind == "column_tab":
            assert row[:i].count(b"\t") == 9 + mark["name"][1] and at in (b"\t", b"\r", b"\n", b""), mark
        elif kind == "colon":
            assert at == b":", mark
        else:
            assert kind == "end" and i == len(row), mark
        # one field of the line is the pad, longer than the look-ahead
        assert max(len(f) for f in row.split(b"\t")) > bc.LOOK


def test_the_constants_are_the_kernels():
    assert (bc.P, bc.PIECE, bc.LOOK) == (4096, 16, 48)
    assert bc.BORDER == list(range(4046, 4114)) + [8191, 8192, 8193]
    assert bc.END_LENGTHS == [4095, 4096, 4097, 8192, 4111, 4127, 4143]
    assert bc.decoys(b"GQ") == [b"GQX", b"G", b"QG", b"GY"] and bc.decoys(b"Q") == [b"QX", b"G", b"QG", b"Y"]


@pytest.mark.parametrize("align", [0, 5])
@pytest.mark.parametrize("key", bc.KEYS)
def test_format_anywhere(key, align):
    slab = bc.format_slab(key, align)
    check_geometry(slab, align)
    text, lb, marks, nind = slab
    want, status = vg.parse_slab(text, lb, nind, key)
    assert not status.any() and not np.isnan(want).any()
    seen = set()
    decoy_then_key = key_then_decoy = third = 0
    for r, mark in enumerate(marks):
        seen.add((mark["name"][0], mark["name"][-1], mark.get("position"), mark["target"]))
        keys = [k for k, a, b in mark["spans"]]
        k = keys.index(key)
        # the value is the one that stands at the key's index, which no other subfield of the column equals
        assert want[r].tolist() == [float(bc.number(r, j, k)) for j in range(nind)]
        assert mark.get("twice") is None or (keys.count(key) == 2 and k == 1)
        for name, a, b in mark["spans"]:
            for border in (P, 2 * P):
                if a < border <= b and name != key and mark["spans"][k][1] >= border:
                    decoy_then_key += 1
                if a < border <= b and name == key and k + 1 < len(keys):
                    key_then_decoy += 1
        third += all(a >= 2 * P for _, a, _ in mark["spans"])
    for what in bc.FORMAT_BYTES:
        for position in bc.POSITIONS:
            for target in bc.BORDER:
                assert (what[0], what[-1], position, target) in seen
    assert third >= 1 and decoy_then_key >= 1 and (key_then_decoy >= 1 or len(key) == 1)
    # INFO carries colons and the key outside column 8
    assert all(b":" in row.split(b"\t")[7] and b"Q" in row.split(b"\t")[7] for row in text.split(b"\n")[:-1])


@pytest.mark.parametrize("key", bc.KEYS)
def test_a_format_of_decoys_only(key):
    slab = bc.no_key_slab(key, 3)
    check_geometry(slab, 3)
    text, lb, marks, nind = slab
    status = vg.parse_slab(text, lb, nind, key)[1]
    assert status[1::2].tolist() == [[vg.NO_KEY, 0]] * 25 and not status[0::2].any()
    straddles = [m for m in marks if m["no_key"] and m["spans"][0][1] < P <= m["spans"][-1][2]]
    assert len(straddles) >= 3 and min(m["target"] for m in marks) < P


def test_the_key_first_in_format():
    for align in (0, 11):
        slab = bc.key_first_slab(align)
        check_geometry(slab, align)
        text, lb, marks, nind = slab
        assert len(marks) == 11 * len(bc.BORDER) and [m["target"] for m in marks[::11]] == bc.BORDER
        assert text[int(lb[4]):].split(b"\t")[8:11][0] == b"GQ:GT:DP" and text[int(lb[4]):].split(b"\t")[10] == b"."
        for missing in (None, 0.0, 99.0):
            want, status = vg.parse_slab(text, lb, nind, bc.KEY, missing)
            # spelled out: the forms are values of 1, 17, 32, 33 bytes, `.`, ``, `.:3`, `:3`, `8`, `.:./.:4`, `:./.`
            per_form = [[0, 0], [0, 0], [0, 0], [1, 1], [0, 0], [5, 1], [0, 0], [5, 1], [0, 0], [0, 0], [5, 1]]
            assert per_form == bc.FIRST_STATUS and (vg.DEFERRED, vg.NO_VALUE) == (1, 5)
            if missing is not None:
                per_form = [[0, 0], [0, 0], [0, 0], [1, 1]] + [[0, 0]] * 7
            assert status.tolist() == per_form * len(bc.BORDER)
            m = 0.0 if missing is None else missing
            value = [7.0, 17.0, 12.5, None, m, None if missing is None else m, m, None if missing is None else m, 8.0, m,
                     None if missing is None else m]
            assert missing is not None or value == bc.FIRST_VALUE
            for r in range(len(marks)):
                v = value[r % 11]
                assert np.isnan(want[r, 1]) if v is None else want[r, 1] == v, (r, want[r])
                assert v is None and status[r, 0] or want[r].tolist() == [float(bc.number(r, 0, 0)), want[r, 1], float(bc.number(r, 2, 0))]
    slab = bc.key_first_slab(5, forms=bc.UNKEPT_FORMS)
    check_geometry(slab, 5)
    text, lb, marks, nind = slab
    assert vg.parse_slab(text, lb, nind, bc.KEY)[1][:4].tolist() == [[1, 1], [5, 1], [1, 1], [5, 1]]
    want, status = vg.parse_slab(text, lb, nind, bc.KEY, None, [2, 0])
    assert not status.any() and not np.isnan(want).any()


@pytest.mark.parametrize("k", bc.CARRY_KS)
def test_column_state_carried_over_passes(k):
    for align in (0, 5):
        slab = bc.carried_slab(k, align)
        check_geometry(slab, align)
        text, lb, marks, nind = slab
        assert bc.carry_keys(k).index(bc.KEY) == k
        for missing in (None, 99.0):
            want, status = vg.parse_slab(text, lb, nind, bc.KEY, missing)
            for r, mark in enumerate(marks):
                row = text[int(lb[r]):int(lb[r + 1])]
                j = 2 if mark["case"] == "short last" else 1
                col = vg.cut_line(row).split(b"\t")[9 + j]
                assert col.startswith(b".") == mark["dot"]
                start = mark["first"] + row.index(b"\t" + col) + 1
                if mark["case"] in ("value", "dot", "empty", "dropped", "once"):
                    # the column begins in the first pass, the named byte stands in a later one
                    assert start == bc.START and mark["target"] >= P - 1 and mark["target"] // P >= 1 or mark["target"] == P - 1
                if mark["case"] in ("value", "once"):
                    assert status[r].tolist() == [0, 0] and want[r, 1] == float(bc.number(r, 1, k))
                    assert col.count(b":") == (k if mark["case"] == "value" else k + 2)
                elif mark["dot"] or missing is not None:
                    assert status[r].tolist() == [0, 0] and want[r, j] == (0.0 if missing is None else 99.0)
                else:
                    assert status[r].tolist() == [vg.NO_VALUE, j]
                if mark["case"] in ("dropped", "short", "short last"):
                    assert col.count(b":") == k - 1
            targets = set((m["case"], m["dot"], m.get("eol"), m["target"]) for m in marks)
            for target in bc.BORDER:
                for dot in (False, True):
                    assert ("short", dot, None, target) in targets
                    assert all(("short last", dot, eol, target) in targets for eol in bc.EOLS)
        # a pass without events: the pad in front of a colon two passes on is longer than a pass
        far = [m for m in marks if m["target"] == 2 * P + 100]
        assert far and all(m["index"] - (bc.START - m["first"]) > P for m in far)


def test_line_ends():
    for align in bc.ALIGNS:
        slab = bc.line_end_slab(align)
        check_geometry(slab, align)
        text, lb, marks, nind = slab
        status = vg.parse_slab(text, lb, nind, bc.KEY)[1]
        status_missing = vg.parse_slab(text, lb, nind, bc.KEY, 99.0)[1]
        want = vg.parse_slab(text, lb, nind, bc.KEY)[0]
        literal = {"value": ([0, 0], [0, 0]), "short": ([5, 2], [0, 0]), "short dot": ([0, 0], [0, 0]), "tab full": ([3, 3], [3, 3]),
                   "tab less": ([5, 2], [0, 0]), "cut": ([0, 0], [0, 0])}
        seen = set()
        for r, mark in enumerate(marks):
            row = text[int(lb[r]):int(lb[r + 1])]
            if mark.get("rest"):
                assert row == bc.REST and status[r].tolist() == [vg.FEW, 0]
                continue
            if mark.get("closing"):
                continue
            assert (status[r].tolist(), status_missing[r].tolist()) == literal[mark["variant"]] == (mark["status"], mark["status_missing"])
            assert row.endswith(mark["eol"]) and vg.cut_line(row) == row[:len(row) - len(mark["eol"])]
            if mark["variant"].startswith("tab"):
                assert vg.cut_line(row).endswith(b"\t") and vg.cut_line(row).count(b"\t") == (12 if mark["variant"] == "tab full" else 11)
            if mark["variant"] in ("value", "cut"):
                assert want[r].tolist() == [float(bc.number(mark_r(row), j, 2)) for j in range(3)]
            if mark["variant"] == "cut":
                assert text[int(lb[r + 1]):].startswith(bc.REST)
            assert len(row) == mark["length"] or (mark["in_pass"] and mark["first"] + len(row) == mark["length"])
            seen.add((mark["variant"], mark["eol"], mark["first"] + len(row)))
            if mark["eol"] == b"\r\n" and mark["first"] + len(row) == P + 1:
                assert (mark["first"] + row.index(b"\r"), mark["first"] + row.index(b"\n")) == (P - 1, P)
        # where the line does not begin a piece it still ends on every one of the in-pass offsets
        for variant, _, _ in bc.END_VARIANTS:
            for eol in (bc.EOLS if variant != "cut" else (b"",)):
                assert all((variant, eol, length) in seen for length in bc.END_LENGTHS), (align, variant, eol)
        # the case that the kernel of the parent commit missed: a tab as the pass's last byte and the line's, ended by the offset
        assert ("tab full", b"", P) in seen and ("tab less", b"", P) in seen and ("tab full", b"", 2 * P) in seen
    rows = bc.end_rows(lambda size: 7)
    assert all(mark["first"] == 7 and len(data) == mark["index"] for data, rest, mark in rows) and len(rows) == 2 * 7 * 16


def mark_r(row):
    """the line's number, as number() took it: from the ID column"""
    return int(row.split(b"\t")[2][2:])


def test_offences_decided_late():
    for align in (0, 5, 15):
        slab = bc.late_slab(align)
        check_geometry(slab, align)
        text, lb, marks, nind = slab
        want, status = vg.parse_slab(text, lb, nind, bc.KEY)
        assert status.tolist() == [[3, 3], [2, 2], [1, 0], [1, 1], [1, 0], [5, 0], [5, 2], [0, 0]] == [x[3] for x in bc.LATE]
        assert vg.parse_slab(text, lb, nind, bc.KEY, 99.0)[1].tolist() == \
            [[3, 3], [2, 2], [1, 0], [1, 1], [1, 0], [1, 2], [0, 0], [0, 0]] == bc.LATE_WITH_MISSING
        assert want[7].tolist() == [41.0, 42.0, 43.0] and want[6, :2].tolist() == [41.0, 42.0]
        assert all(2 * P < int(n) < 3 * P for n in np.diff(lb))                       # lines of three passes
        for r, mark in enumerate(marks):
            row = text[int(lb[r]):int(lb[r + 1])]
            if bc.D33 in row:                                                         # the deferred value: first or third pass
                at = mark["first"] + row.index(bc.D33)
                assert at < P - 100 or at > 2 * P, mark
