"""GPU: one scalar FORMAT subfield per sample parsed from VCF text and dictionary-coded on the device
(garlic_tgls_set_rows_vcf, csrc/vcf_gl_kernels.hpp), bit for bit against the rule of tests/vcf_gl_cases.py, and code for code
against garlic_tgls_set_rows_text on the twin .tgls text.

tgls_vcf_parse_kernel has no switch point: every line takes the same passes of 256 sixteen-byte pieces.  What changes with the
shape is covered by shape: sample counts around the piece, the wave and the pass (1250 samples make lines of several passes),
FORMAT changing from line to line with the key at position 1, 2 and last, neighbouring subfields longer than the look-ahead,
values planted on the last byte of a pass and around it, slabs at every alignment."""
import numpy as np
import pytest

import tgls_cases as tc
import vcf_cases as vc
import vcf_gl_cases as vg
from garlic_amd import abi
from vcf_gl_cases import feed

pytestmark = pytest.mark.gpu

ROWS = 40
KEY = b"GQ"


def random_tokens(rng, rows, nind):
    """GQ integers, GL decimals and PL integers by row: every one inside tgls_number's fast grammar"""
    kinds = [tc.gq_tokens(rng, rows, nind), tc.gl_tokens(rng, rows, nind), tc.pl_tokens(rng, rows, nind)]
    toks = [kinds[r % 3][r] for r in range(rows)]
    assert not any(tc.defers(t) for row in toks for t in row)       # tests/test_tgls_cpu.py pins defers() to the host build
    return toks


def random_slab(nind, seed, rows=ROWS, edit=None):
    """lines that end in \\n and \\r\\n, the last one at the slab's end without either; two lines stand in the text and are
    left out of line_begin.  edit(lines): changes the data lines before they are joined"""
    rng = np.random.default_rng(seed)
    lines = vg.random_lines(rng, rows, nind, random_tokens(rng, rows, nind), eols=(b"\n", b"\n", b"\r\n"), last_eol=b"")
    if edit:
        edit(lines)
    extra = [vg.data_line(900, [b"GT"], [b"0/0"] * nind), vg.data_line(901, [b"GT", b"GQ"], [b"0/0:1,2"] * nind)]
    mid = rows // 2
    lines = lines[:3] + extra[:1] + lines[3:mid] + extra[1:] + lines[mid:]
    keep = [k for k in range(len(lines)) if k not in (3, mid + 1)]
    return vc.slab_of(lines, keep=keep)


def check_against_rule_and_twin(gpu_ctx, text, lb, nind, where, col_idx=None, missing_raw=None):
    rows = len(lb) - 1
    want, want_status = vg.parse_slab(text, lb, nind, KEY, missing_raw, col_idx)
    assert not want_status.any() and not np.isnan(want).any()
    twin_text, twin_lb = tc.slab_of(vg.twin_tgls(text, lb, nind, KEY, missing_raw))
    with abi.Tgls(gpu_ctx, rows, nind, col_idx) as obj, abi.Tgls(gpu_ctx, rows, nind, col_idx) as twin:
        status, err = feed(obj, text, lb, where, missing_raw=missing_raw)
        assert err is None and not status.any(), (nind, where, err, np.argwhere(status[:, 0] != 0)[:3].tolist(), status[status[:, 0] != 0][:3])
        got = obj.get_rows()
        assert np.array_equal(tc.bits(got), tc.bits(want)), (nind, where, np.argwhere(tc.bits(got) != tc.bits(want))[:5])
        assert obj.info() == (np.unique(tc.bits(want)).shape[0], rows, 0)
        status, err = twin.set_rows_text(twin_text, twin_lb)
        assert err is None and not status.any()
        # the same dictionary in the same order and the same values row by row: the same codes
        assert np.array_equal(tc.bits(obj.values()), tc.bits(twin.values()))
        assert np.array_equal(tc.bits(twin.get_rows()), tc.bits(got))
    return want


@pytest.mark.parametrize("where", ["host", "dev1", "dev15"])
@pytest.mark.parametrize("nind", vc.NINDS)
def test_raw_values_are_the_rules_and_the_codes_the_twins(gpu_ctx, nind, where):
    text, lb = random_slab(nind, 100 + nind)
    assert not text.endswith(b"\n") and b"\r\n" in text
    assert sorted(set(pos for _, pos in vg.FORMATS)) == [1, 2, 4] and vg.FORMATS[3][0][-1] == KEY     # position 1, 2 and last
    if nind == 1250:
        assert min(np.diff(lb)) > tc.PASS_BYTES and max(np.diff(lb)) > 3 * tc.PASS_BYTES
    check_against_rule_and_twin(gpu_ctx, text, lb, nind, where)


def test_text_at_every_alignment(gpu_ctx):
    text, lb = random_slab(9, 7, rows=12)
    for offset in range(16):
        check_against_rule_and_twin(gpu_ctx, text, lb, 9, "dev%d" % offset)


@pytest.mark.parametrize("missing_raw", [None, 0.0, 99.0])
def test_missing_value_on_and_off(gpu_ctx, missing_raw):
    """on missing genotypes the value is 0 without a missing value and the missing value with one"""
    text, lb = random_slab(65, 3)
    want = check_against_rule_and_twin(gpu_ctx, text, lb, 65, "host", missing_raw=missing_raw)
    plain, _ = vg.parse_slab(text, lb, 65, KEY, None)
    differs = tc.bits(want) != tc.bits(plain)
    assert differs.any() == (missing_raw == 99.0)


def planted_line(r, offset_in_pass, target, value, nind=3):
    """a line whose sample 0 carries `value` as its GQ, the value's first byte `target` bytes into the pass that holds it:
    the DP in front is a run of digits sized for that (far longer than the look-ahead).  offset_in_pass: where the line's
    first byte stands in its first pass"""
    head = vg.FIXED % (100 + r, r) + b"GT:DP:GQ:PL\t0/1:"
    pad = target - offset_in_pass - len(head) - 1
    assert pad > 48
    cols = [b"0/1:" + b"7" * pad + b":" + value + b":0,5,9"] + [b"1/1:3:%d:0,0,0" % (j + 1) for j in range(1, nind)]
    line = vg.data_line(r, [b"GT", b"DP", b"GQ", b"PL"], cols)
    assert line.index(b":" + value + b":") + 1 + offset_in_pass == target
    return line


@pytest.mark.parametrize("where", ["dev0", "dev5"])
def test_values_planted_around_the_borders_of_pieces_and_passes(gpu_ctx, where):
    """a value that starts on the last byte of a pass (and of a piece), on the first of the next pass (its colon is the last
    byte), two in front, and in the last three slots of a pass, with 1, 17 and 32 bytes; 33 bytes defer"""
    offset = int(where[3:])
    values = [b"7", b"0" * 15 + b"17", b"0" * 28 + b"12.5", b"0" * 29 + b"12.5"]
    assert [len(v) for v in values] == [1, 17, 32, 33]
    targets = [tc.PASS_BYTES - 1, tc.PASS_BYTES, tc.PASS_BYTES - 2, tc.PASS_BYTES - 17, tc.PASS_BYTES - 33, tc.PASS_BYTES - 48,
               2 * tc.PASS_BYTES - 1, tc.PASS_BYTES + 15]
    lines, at = [], 0
    for target in targets:
        for value in values:
            lines.append(planted_line(len(lines), (at + offset) & 15, target, value))
            at += len(lines[-1])
    text, lb = tc.slab_of(lines)
    want, want_status = vg.parse_slab(text, lb, 3, KEY)
    deferred = np.array([len(values[r % 4]) > 32 for r in range(len(lines))])
    assert np.array_equal(want_status[:, 0] == vg.DEFERRED, deferred) and not want_status[~deferred].any()
    with abi.Tgls(gpu_ctx, len(lines), 3) as obj:
        status, err = feed(obj, text, lb, where)
        assert err is None and np.array_equal(status, want_status), status.tolist()
        for r in np.flatnonzero(~deferred):
            got = obj.get_rows(row_begin=int(r), row_count=1)
            assert np.array_equal(tc.bits(got), tc.bits(want[r:r + 1])), (int(r), got, want[r])


def statuses_slab():
    nind = 70
    rng = np.random.default_rng(5)
    toks = random_tokens(rng, 20, nind)
    fmt = [b"GT", b"DP", b"GQ"]

    def cols_of(r, change=None):
        cols = [b"0/1:%d:" % (r + j) + toks[r][j] for j in range(nind)]
        for j, col in (change or {}).items():
            cols[j] = col
        return cols
    big = b"%d" % (2 ** 53 + 1)
    lines = [
        vg.data_line(0, fmt, cols_of(0)),
        vg.data_line(1, [b"GT", b"DP", b"GQX", b"QG"], cols_of(1)),                     # NO_KEY
        vg.data_line(2, [b"GT"], [b"0/1"] * nind),                                        # NO_KEY
        vg.data_line(3, fmt, cols_of(3, {5: b"0/1:3"})),                                  # NO_VALUE: dropped
        vg.data_line(4, fmt, cols_of(4, {0: b"1|1:3:."})),                                # NO_VALUE: '.'
        vg.data_line(5, fmt, cols_of(5, {69: b"1|1:3:"})),                                # NO_VALUE: empty, the line's last column
        vg.data_line(6, fmt, cols_of(6, {7: b"./.", 8: b".|.:3:.", 9: b"./.:3:", 10: b".:3"})),      # clean: missing genotypes
        vg.data_line(7, fmt, cols_of(7, {33: b"0/0:1:" + b"0" * 31 + b"12"})),           # DEFERRED: 33 bytes
        vg.data_line(8, fmt, cols_of(8, {1: b"0/0:1:" + big})),                           # DEFERRED: 2^53 + 1
        vg.data_line(9, fmt, cols_of(9, {2: b"0/0:1:nan"})),
        vg.data_line(10, fmt, cols_of(10, {64: b"0/0:1:1,2"})),
        vg.data_line(11, fmt, cols_of(11, {63: b"0/0:1:0x1p3"})),
        vg.data_line(12, fmt, cols_of(12)[:50]),                                          # FEW
        vg.data_line(13, fmt, cols_of(13) + [b"0/0:1:1", b"0/0:1:2"]),                    # MANY
        vg.data_line(14, fmt, cols_of(14, {20: b"0/0:1:1,2", 11: b"0/1"})),               # two offences: the lowest column
        vg.data_line(15, fmt, cols_of(15, {20: b"0/0:1:1,2"}) + [b"0/0"]),                # deferred, then too many
        vg.data_line(16, fmt, cols_of(16), eol=b"\r\n"),
        b"1\t5\n",                                                                        # FEW, 0
        vg.data_line(18, fmt, cols_of(18, {4: b"0/1:2:2e0"})),
        vg.data_line(19, fmt, cols_of(19), eol=b""),
    ]
    return nind, lines


def test_statuses_and_the_completion_of_deferred_rows(gpu_ctx):
    nind, lines = statuses_slab()
    text, lb = tc.slab_of(lines)
    want, want_status = vg.parse_slab(text, lb, nind, KEY)
    assert want_status.tolist() == [[0, 0], [vg.NO_KEY, 0], [vg.NO_KEY, 0], [vg.NO_VALUE, 5], [vg.NO_VALUE, 0], [vg.NO_VALUE, 69], [0, 0],
                                    [1, 33], [1, 1], [1, 2], [1, 64], [1, 63], [vg.FEW, 50], [vg.MANY, nind], [vg.NO_VALUE, 11], [1, 20],
                                    [0, 0], [vg.FEW, 0], [0, 0], [0, 0]]
    assert (vg.NO_KEY, vg.NO_VALUE) == (abi.TGLS_VCF_NO_KEY, abi.TGLS_VCF_NO_VALUE)
    clean = [0, 6, 16, 18, 19]
    with abi.Tgls(gpu_ctx, 20, nind) as obj:
        status, err = feed(obj, text, lb, "dev3")
        assert np.array_equal(status, want_status), status.tolist()
        assert err is not None and err.code == abi.ERR_INVALID and "row 1 " in str(err) and "FORMAT" in str(err), err
        assert obj.info()[1:] == (len(clean), 6)
        for r in clean:
            assert np.array_equal(tc.bits(obj.get_rows(row_begin=r, row_count=1)), tc.bits(want[r:r + 1])), r
        assert want[6, 7:11].tolist() == [0.0, 0.0, 0.0, 0.0]
        with pytest.raises(abi.GarlicError) as e:
            obj.get_rows(row_begin=7, row_count=1)
        assert e.value.code == abi.ERR_STATE and "deferred" in str(e.value)
        for r in (7, 8, 9, 10, 11, 15):
            vals = np.where(np.isnan(want[r]), 0.5, want[r])[None, :]
            obj.set_rows_values(vals, row_begin=r)
            assert np.array_equal(tc.bits(obj.get_rows(row_begin=r, row_count=1)), tc.bits(vals)), r
        assert obj.info()[1:] == (len(clean) + 6, 0)
    # with a missing value the called genotypes without one are clean, and only they change
    with abi.Tgls(gpu_ctx, 20, nind) as obj:
        status, err = feed(obj, text, lb, missing_raw=0.0)
        w2, s2 = vg.parse_slab(text, lb, nind, KEY, 0.0)
        assert np.array_equal(status, s2) and s2[[3, 4, 5]].tolist() == [[0, 0]] * 3 and s2[14].tolist() == [1, 20]
        assert err is not None and "row 1 " in str(err)
        for r in clean + [3, 4, 5]:
            assert np.array_equal(tc.bits(obj.get_rows(row_begin=r, row_count=1)), tc.bits(w2[r:r + 1])), r
    # the lowest offending row is the one named
    with abi.Tgls(gpu_ctx, 20, nind) as obj:
        status, err = feed(obj, text[lb[3]:], lb[3:] - lb[3], row_begin=3)
        assert err is not None and "row 3 " in str(err) and "sample column" in str(err) and "(5)" in str(err), err


@pytest.mark.parametrize("name", ["one", "every third", "reversed", "repeat"])
def test_kept_columns(gpu_ctx, name):
    nind = 65
    col_idx = {"one": [17], "every third": list(range(0, nind, 3)), "reversed": list(range(nind - 1, -1, -1)),
               "repeat": [3, 9, 3, 0, 64, 9, 9]}[name]
    def edit(lines):      # offences in columns that are not kept are not looked for: a list, and a called genotype without a value
        if name != "reversed":
            cols = lines[0].split(b"\t")
            cols[9 + 1] = b"0/1:1:1,2:4:5:6"
            cols[9 + 2] = b"0/1"
            lines[0] = b"\t".join(cols)
    text, lb = random_slab(nind, 11, edit=edit)
    want, want_status = vg.parse_slab(text, lb, nind, KEY, None, col_idx)
    assert not want_status.any() and not np.isnan(want).any()
    with abi.Tgls(gpu_ctx, ROWS, nind, col_idx) as obj:
        status, err = feed(obj, text, lb)
        assert err is None and not status.any(), status[status[:, 0] != 0][:3]
        assert np.array_equal(tc.bits(obj.get_rows()), tc.bits(want))


def test_several_slabs_and_both_doors_fill_one_object(gpu_ctx):
    """rows 0..14 and 30..39 from VCF slabs, rows 15..29 from the twin's text: values and dictionary equal those of an object
    fed the twin's text with the same rows per call"""
    nind = 64
    rng = np.random.default_rng(21)
    toks = [[b"-%d.%03d" % (v // 1000, v % 1000) for v in rng.integers(0, 12000, size=nind)] for _ in range(ROWS)]
    lines = vg.random_lines(rng, ROWS, nind, toks)
    text, lb = vc.slab_of(lines)
    want, want_status = vg.parse_slab(text, lb, nind, KEY)
    assert not want_status.any()
    twin_lines = vg.twin_tgls(text, lb, nind, KEY)
    parts = [(0, 15, "vcf"), (15, 30, "text"), (30, ROWS, "vcf")]
    with abi.Tgls(gpu_ctx, ROWS, nind) as obj, abi.Tgls(gpu_ctx, ROWS, nind) as twin:
        for a, b, door in parts:
            t2, l2 = tc.slab_of(twin_lines[a:b])
            status, err = twin.set_rows_text(t2, l2, row_begin=a)
            assert err is None and not status.any()
            if door == "vcf":
                t1, l1 = vc.slab_of(lines[a:b], header=b"#x\n")
                status, err = feed(obj, t1, l1, row_begin=a)
            else:
                status, err = obj.set_rows_text(t2, l2, row_begin=a)
            assert err is None and not status.any()
        assert obj.info() == twin.info() and obj.info()[1:] == (ROWS, 0)
        assert np.array_equal(tc.bits(obj.values()), tc.bits(twin.values()))
        assert np.array_equal(tc.bits(obj.get_rows()), tc.bits(want))
        assert np.array_equal(tc.bits(obj.get_rows(tc.GL)), tc.bits(twin.get_rows(tc.GL)))


@pytest.mark.parametrize("key", [b"", b"GT", b"G Q", b"G:Q", b"GQ\t", b"A" * 17, b"G-Q"])
def test_bad_keys_are_refused(gpu_ctx, key):
    text, lb = tc.slab_of([vg.data_line(0, [b"GT", b"GQ"], [b"0/0:5"])])
    with abi.Tgls(gpu_ctx, 1, 1) as obj:
        with pytest.raises(abi.GarlicError) as e:
            feed(obj, text, lb, key=key)
        assert e.value.code == abi.ERR_INVALID and "key" in str(e.value)
        assert obj.info() == (0, 0, 0)


@pytest.mark.parametrize("key", [b"GQ", b"G", b"X.y_0", b"A" * 16])
def test_keys_of_every_length(gpu_ctx, key):
    lines = [vg.data_line(0, [b"GT", key + b"X", key, b"Z"], [b"0/0:1:5:2", b"0/1:1:6:2"]),
             vg.data_line(1, [b"GT", b"A" * 15, key[:-1] + b"Y", key], [b"0/0:1:2:7", b"0/1:1:2:8"])]
    text, lb = tc.slab_of(lines)
    with abi.Tgls(gpu_ctx, 2, 2) as obj:
        status, err = feed(obj, text, lb, key=key)
        assert err is None and not status.any()
        assert obj.get_rows().tolist() == [[5.0, 6.0], [7.0, 8.0]]
