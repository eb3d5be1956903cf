"""No GPU: the rule of garlic_tgls_set_rows_vcf as tests/vcf_gl_cases.py states it, on hand-written lines, and the host's parser
of the same rule (vcf::parseGlValues, garlic_amd/host/vcf_lines.hpp) over those lines, the deferred forms and the refusals."""
import os
import subprocess

import numpy as np

import vcf_gl_border_cases as bc
import vcf_gl_cases as vg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = b"1\t100\trs0\tA\tG\t.\tPASS\t.\t"

# (line, nsamples, missing_raw, values or None, status)
HAND = [
    (F + b"GT:GQ\t0/1:35\t1|1:7\n", 2, None, [35.0, 7.0], (0, 0)),
    (F + b"GT:DP:GQ\t0/1:9:35\t1|1:9:7.5\r\n", 2, None, [35.0, 7.5], (0, 0)),
    (F + b"GT:AD:DP:PL:GQ\t0/1:1,2:9:0,1,2:35\t1|1:3,4:9:5,5,5:1e1", 2, None, [35.0, 10.0], (0, 0)),
    (F + b"GT:GQX:GQ:QG\t0/1:1:2:3\t1|1:4:5:6\n", 2, None, [2.0, 5.0], (0, 0)),
    (F + b"GT:DP:GQ\t./.\t.|.:3:.\t./.:3:\t.:3\t0/0:1:-0\n", 5, None, [0.0, 0.0, 0.0, 0.0, -0.0], (0, 0)),
    (F + b"GT:DP:GQ\t./.\t.|.:3:.\t./.:3:\t0/0:1\n", 4, 42.0, [42.0, 42.0, 42.0, 42.0], (0, 0)),
    (F + b"GT:DP:GQ\t0/0:1:5\t0/1:3\n", 2, None, None, (vg.NO_VALUE, 1)),
    (F + b"GT:DP:GQ\t0/0:1:.\t0/1:3:4\n", 2, None, None, (vg.NO_VALUE, 0)),
    (F + b"GT:DP:GQ\t0/0:1:5\t0/1:3:\n", 2, None, None, (vg.NO_VALUE, 1)),
    (F + b"GT:DP:GQ\t0/0:1:5\t\n", 2, None, None, (vg.NO_VALUE, 1)),
    (F + b"GT:DP\t0/0:1\t0/1:3\n", 2, None, None, (vg.NO_KEY, 0)),
    (F + b"GT:GQX\t0/0:1\t0/1:3\n", 2, None, None, (vg.NO_KEY, 0)),
    (F + b"GT:DP:GQ\t0/0:1:5\n", 2, None, None, (vg.FEW, 1)),
    (F + b"GT:DP:GQ\t0/0:1:5\t0/0:1:5\t0/0:1:5\n", 2, None, None, (vg.MANY, 2)),
    (b"1\t5\n", 2, None, None, (vg.FEW, 0)),
    # the key first in FORMAT: the value stands on the column's own first byte
    (F + b"GQ:GT\t5:0/1\t:0/1\n", 2, 3.0, [5.0, 3.0], (0, 0)),
    (F + b"GQ:GT:DP\t.\t.:3\t8\t.:./.:4\n", 4, None, [0.0, 0.0, 8.0, 0.0], (0, 0)),
    (F + b"GQ:GT\t\t5:0/1\n", 2, None, None, (vg.NO_VALUE, 0)),
    (F + b"GQ:GT\t5:0/1\t:0/1\n", 2, None, None, (vg.NO_VALUE, 1)),
    # a tab as the line's last byte: an empty column behind it
    (F + b"GT:DP:GQ\t0/0:1:5\t0/0:1:6\t\n", 2, None, None, (vg.MANY, 2)),
    (F + b"GT:DP:GQ\t0/0:1:5\t0/0:1:6\t", 2, 42.0, None, (vg.MANY, 2)),
    (F + b"GT:DP:GQ\t0/0:1:5\t", 2, 42.0, [5.0, 42.0], (0, 0)),
    (F + b"GT:DP:GQ\t0/0:1:5\t\r\n", 2, None, None, (vg.NO_VALUE, 1)),
]
# what the device defers and the host completes, or refuses
DEFERRED = [
    (F + b"GT:GQ\t0/1:" + b"0" * 31 + b"12\t1|1:7\n", [12.0, 7.0]),
    (F + b"GT:GQ\t0/1:%d\t1|1:7\n" % (2 ** 53 + 1), [float(2 ** 53 + 1), 7.0]),
    (F + b"GT:GQ\t0/1:nan\t1|1:7\n", None),
    (F + b"GT:GQ\t0/1:7\t1|1:-inf\n", None),
    (F + b"GT:GQ\t0/1:0x1p3\t1|1:7\n", [8.0, 7.0]),
    (F + b"GT:GQ\t0/1:1e23\t1|1:7\n", [1e23, 7.0]),
    (F + b"GT:GQ\t0/1:1,2\t1|1:7\n", None),
    (F + b"GT:GQ\t0/1:7\t1|1:7x\n", None),
]


def test_the_rule_on_hand_written_lines():
    for line, n, missing, values, status in HAND:
        got, st = vg.parse_line(line, n, b"GQ", missing)
        assert st == status, (line, st)
        if values is not None:
            assert np.array_equal(got.view(np.uint64), np.array(values).view(np.uint64)), (line, got)
    for line, values in DEFERRED:
        got, st = vg.parse_line(line, 2, b"GQ")
        assert st[0] == vg.DEFERRED and st[1] == (1 if b"7x" in line or b"inf" in line else 0), (line, st)
    # a column that is not kept is not looked at; the lowest column wins; a key at position 0
    assert vg.parse_line(HAND[6][0], 2, b"GQ", None, kept={0})[1] == (0, 0)
    assert vg.parse_line(F + b"GT:GQ\t0/1:1,2\t0/1\n", 2, b"GQ")[1] == (vg.DEFERRED, 0)
    assert vg.parse_line(F + b"GT:GQ\t0/1\t0/1:1,2\n", 2, b"GQ")[1] == (vg.NO_VALUE, 0)
    assert vg.parse_line(F + b"GQ:GT\t5:0/1\t:0/1\n", 2, b"GQ", 3.0)[0].tolist() == [5.0, 3.0]
    # the twin's text holds the same tokens
    text = b"".join(h[0] for h in HAND[:5] if h[0].endswith(b"\n"))
    lb = np.cumsum([0] + [len(h[0]) for h in HAND[:2]])
    assert vg.twin_tgls(text, lb, 2, b"GQ") == [b"1 rs0 0.0 100 35 7\n", b"1 rs1 0.1 101 35 7.5\n"]


def test_vcf_gl_lines_unit_under_sanitizers(tmp_path):
    """tests/host_unit/vcf_gl_lines_unit.cpp, compiled here with ASan + UBSan: a stand-alone program, nothing loaded into python"""
    exe = str(tmp_path / "vcf_gl_lines_unit")
    src = os.path.join(ROOT, "tests", "host_unit", "vcf_gl_lines_unit.cpp")
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                         "-o", exe, src, "-lz"], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]

    def run(lines, n, missing, cols=()):
        path = str(tmp_path / "lines.vcf")
        with open(path, "wb") as f:
            f.write(b"".join(ln if ln.endswith(b"\n") else ln + b"\n" for ln in lines))
        r = subprocess.run([exe, "GQ", str(n), "none" if missing is None else repr(missing), path, *[str(c) for c in cols]],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "vcf_gl_lines_unit ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
        return r.stdout.splitlines()[:-1]

    for line, n, missing, values, status in HAND:
        out = run([line], n, missing)[0].split(" ", 2)
        if values is not None:
            got = np.array([float(v) for v in " ".join(out[1:]).split()])
            assert out[0] == "ok" and np.array_equal(got.view(np.uint64), np.array(values).view(np.uint64)), (line, out)
        else:
            assert out[0] == "bad" and int(out[1]) == (status[1] if status[0] == vg.NO_VALUE else -1), (line, out)
            word = {vg.NO_VALUE: "without GQ", vg.NO_KEY: "does not name GQ", vg.FEW: "too few", vg.MANY: "too many"}[status[0]]
            assert word in out[2], (line, out)
    for line, values in DEFERRED:
        out = run([line], 2, None)[0].split(" ", 2)
        if values is None:
            why = "no finite number" if b"nan" in line or b"inf" in line else "no single number"
            assert out[0] == "bad" and why in out[2] and ("list" in out[2]) == (b"1,2" in line), (line, out)
            assert int(out[1]) == (1 if b"7x" in line or b"inf" in line else 0)
        else:
            got = np.array([float(v) for v in " ".join(out[1:]).split()])
            assert out[0] == "ok" and np.array_equal(got, np.array(values), equal_nan=True), (line, out)
    # kept columns in any order and with repeats; several lines in one file
    lines = [h[0] for h in HAND[:4]]
    out = run(lines, 2, None, cols=(1, 0, 1))
    assert [o.split()[1:] for o in out] == [["7", "35", "7"], ["7.5", "35", "7.5"], ["10", "35", "10"], ["5", "2", "5"]]
    # the lines of tests/vcf_gl_border_cases.py, the key first and trailing tabs among them: the host gives the rule's values
    # wherever the rule gives values (and completes what the device defers), and refuses what the rule refuses
    # (in late_slab every deferred value stands in a line with a second offence, which the host names instead)
    for slab, missing, completes in ((bc.key_first_slab(0), None, True), (bc.key_first_slab(3), 99.0, True),
                                     (bc.carried_slab(2, 0), None, True), (bc.line_end_slab(0), None, True),
                                     (bc.line_end_slab(1), 99.0, True), (bc.late_slab(0), None, False)):
        text, lb, marks, nind = slab
        rows = [text[int(lb[r]):int(lb[r + 1])] for r in range(len(marks))]
        want, status = vg.parse_slab(text, lb, nind, b"GQ", missing)
        out = run(rows, nind, missing)
        assert len(out) == len(rows)
        for r, o in enumerate(out):
            o = o.split(" ", 2)
            if status[r, 0] == vg.OK or (status[r, 0] == vg.DEFERRED and completes):
                got = np.array([float(v) for v in " ".join(o[1:]).split()])
                full = np.where(np.isnan(want[r]), 12.5, want[r])           # the one deferred value of these lines
                assert o[0] == "ok" and np.array_equal(got.view(np.uint64), full.view(np.uint64)), (marks[r], o)
            else:
                assert o[0] == "bad", (marks[r], o)
                assert status[r, 0] == vg.DEFERRED or int(o[1]) == (status[r, 1] if status[r, 0] == vg.NO_VALUE else -1), (marks[r], o)
