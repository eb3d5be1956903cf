"""GPU: --tgls text parsed and dictionary-coded on the device (garlic_tgls), bit for bit against the pure-Python model of
tests/tgls_cases.py (float(token), bytes.split(), the conversion restated with math.pow), against the reference's reader,
and as a panel's likelihoods against the oracle's scores.

tgls_parse_kernel has no switch point: every line takes the same passes of 256 sixteen-byte pieces.  What changes with the
shape is covered by shape: one-byte tokens (a 300-column line is one pass), tokens padded to 12..24 bytes behind separator
runs of 1..5 spaces and tabs (a 300-column line is two passes: tokens astride pieces and the pass boundary, one that begins
in the last slot of a pass), column counts around the wave and the piece, slabs that start 1 and 15 bytes past an aligned
address."""
import numpy as np
import pytest

import oracle_lib as ol
import tgls_cases as tc
from garlic_amd import abi

pytestmark = pytest.mark.gpu

NCOLS = [1, 7, 8, 9, 63, 64, 65, 300]
ROWS = 40


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


def feed(obj, text, lb, where="host", row_begin=0):
    """-> (status, err); where: "host", or "devN" = device text N bytes past an aligned address, poisoned with digits around"""
    if where == "host":
        return obj.set_rows_text(text, lb, row_begin=row_begin)
    slab = DeviceSlab(text, int(where[3:]), 0x37)
    return obj.set_rows_text(slab.ptr, lb, row_begin=row_begin, text_bytes=len(text), where=abi.DEVICE)


def padded_slab(ncols, where, seed=0):
    """40 lines of padded tokens with every variation of the slab: leading and trailing blanks, \\r\\n, lines left out between
    kept ones, the last line without a newline; at 300 columns line 0 has a token that begins in the last slot of its first
    pass (the slab's byte 0 stands `offset` bytes into its piece)"""
    rng = np.random.default_rng(1000 + ncols + seed)
    kinds = [tc.gq_tokens(rng, ROWS, ncols), tc.gl_tokens(rng, ROWS, ncols), tc.pl_tokens(rng, ROWS, ncols)]
    offset = 0 if where == "host" else int(where[3:])
    lines, placed = [], None
    for r in range(ROWS):
        toks = kinds[r % 3][r]
        lead = b" \t " if r % 4 == 1 else b""
        trail = b"\t  " if r % 4 == 2 else b""
        eol = b"" if r == ROWS - 1 else b"\r\n" if r % 5 == 3 else b"\n"
        line, col = tc.padded_line(rng, r, toks, target=tc.PASS_BYTES - 6 - offset if r == 0 and ncols == 300 else None,
                                   lead=lead, trail=trail, eol=eol)
        placed = col if r == 0 else placed
        lines.append(line)
    text, lb = tc.slab_of(lines, between={3: b"# a line the caller leaves out\n", 17: b"1 rsX 0 1 5 5 5\n\n"})
    return text, lb, placed


@pytest.mark.parametrize("where", ["host", "dev1", "dev15"])
@pytest.mark.parametrize("ncols", NCOLS)
def test_raw_values_are_float_of_the_token(gpu_ctx, ncols, where):
    rng = np.random.default_rng(ncols)
    one_byte = [tc.plain_line(r, toks) for r, toks in enumerate(tc.gq_tokens(rng, ROWS, ncols, one_byte=True))]
    text1, lb1 = tc.slab_of(one_byte)
    text2, lb2, placed = padded_slab(ncols, where)
    if ncols == 300:
        assert len(one_byte[0]) < tc.PASS_BYTES and placed is not None and lb2[1] > tc.PASS_BYTES + 100
    for tag, text, lb in (("one byte", text1, lb1), ("padded", text2, lb2)):
        want, want_status = tc.parse_slab(text, lb, ncols)
        assert not want_status.any() and not np.isnan(want).any()
        with abi.Tgls(gpu_ctx, ROWS, ncols) as obj:
            status, err = feed(obj, text, lb, where)
            assert err is None and not status.any(), (tag, ncols, where, err, status[status[:, 0] != 0][:3])
            got = obj.get_rows()
            assert np.array_equal(tc.bits(got), tc.bits(want)), (tag, ncols, where, np.argwhere(tc.bits(got) != tc.bits(want))[:5])
            assert obj.info() == (np.unique(tc.bits(want)).shape[0], ROWS, 0)


def statuses_slab(where):
    """12 lines of 300 padded columns with their offences.  Line 0 is the slab's first, so its passes are counted from the
    slab's own piece: the slab's byte 0 stands `offset` bytes into it, and the planted 16-byte token begins 11 bytes in front
    of the first pass's end.  -> (lines, text, lb, column of the planted token)"""
    ncols = 300
    offset = 0 if where == "host" else int(where[3:])
    rng = np.random.default_rng(77)
    toks = tc.gl_tokens(rng, 12, ncols)
    late = b"1e23"                                      # in the grammar, past the fast path: deferred, and float() reads it
    toks[1][0] = late
    toks[2][1] = late
    toks[3][ncols - 1] = late
    toks[5][5], toks[5][9] = b"nan", late              # two offences: the first in file order
    toks[6][200] = b"0.000000000000000000000000000000001"      # 35 bytes: longer than the look-ahead
    toks[7] = toks[7][:123]                             # FEW
    toks[8] = toks[8] + [b"1", b"2"]                    # MANY
    toks[9][7] = late
    toks[9] = toks[9] + [b"3"]                          # deferred, then too many: the first in file order
    lines, astride = [], None
    planted = b"0000000000001e23"
    for r in range(12):
        line, col = tc.padded_line(rng, r, toks[r], target=tc.PASS_BYTES - 11 - offset if r == 0 else None, planted=planted if r == 0 else None)
        astride = col if r == 0 else astride
        lines.append(line)
    text, lb = tc.slab_of(lines)
    # where the planted token stands in its pass: the pass begins at the aligned piece that holds the line's first byte
    start = lines[0].index(planted) + ((int(lb[0]) + offset) & 15)
    assert astride is not None and lb[0] == 0 and start < tc.PASS_BYTES <= start + len(planted) - 1, (start, astride)
    return lines, text, lb, astride


@pytest.mark.parametrize("where", ["host", "dev15"])
def test_statuses_and_the_completion_of_deferred_rows(gpu_ctx, where):
    """one deferred token per row astride the pass boundary and at columns 0, 1 and the last; two offences report the first in
    file order; FEW / MANY carry their columns; the clean rows of the offending call are set; deferred rows completed through
    set_rows_values equal the model"""
    ncols = 300
    lines, text, lb, astride = statuses_slab(where)
    want, want_status = tc.parse_slab(text, lb, ncols)
    assert want_status.tolist() == [[1, astride], [1, 0], [1, 1], [1, ncols - 1], [0, 0], [1, 5], [1, 200], [tc.FEW, 123], [tc.MANY, ncols],
                                    [1, 7], [0, 0], [0, 0]]
    with abi.Tgls(gpu_ctx, 12, ncols) as obj:
        status, err = feed(obj, text, lb, where)
        assert np.array_equal(status, want_status), (where, status.tolist())
        assert err is not None and err.code == abi.ERR_INVALID and "row 7" in str(err) and "too few" in str(err), err
        assert obj.info()[1:] == (3, 7)
        for r in (4, 10, 11):
            assert np.array_equal(tc.bits(obj.get_rows(row_begin=r, row_count=1)), tc.bits(want[r:r + 1])), r
        with pytest.raises(abi.GarlicError) as e:
            obj.get_rows(row_begin=1, row_count=1)
        assert e.value.code == abi.ERR_STATE and "deferred" in str(e.value)
        # what the host's stream parse reads of the deferred rows (row 5's nan excepted: the test brings a number)
        fixed = dict((r, lines[r].replace(b"nan", b"0.5") if r == 5 else lines[r]) for r in (0, 1, 2, 3, 5, 6))
        for r, line in fixed.items():
            t1, l1 = tc.slab_of([line])
            vals = tc.host_values(t1, l1, ncols)
            obj.set_rows_values(vals, row_begin=r)
            assert np.array_equal(tc.bits(obj.get_rows(row_begin=r, row_count=1)), tc.bits(vals)), r
            keep = ~np.isnan(want[r])
            assert np.array_equal(tc.bits(vals[0][keep]), tc.bits(want[r][keep]))
        assert obj.info()[1:] == (9, 1)
        with abi.Panel(gpu_ctx, [12], 4) as panel, pytest.raises(abi.GarlicError) as e:
            panel.set_gl_tgls(obj, abi.GL_GL, np.arange(12))
        assert e.value.code == abi.ERR_STATE


@pytest.mark.parametrize("name", ["all", "one", "every third", "reversed", "repeat"])
def test_kept_columns(gpu_ctx, name):
    ncols = 65
    col_idx = {"all": None, "one": [17], "every third": list(range(0, ncols, 3)), "reversed": list(range(ncols - 1, -1, -1)),
               "repeat": [3, 9, 3, 0, 64, 9, 9]}[name]
    text, lb, _ = padded_slab(ncols, "host", seed=5)
    # a token the parser defers, in a column that is not kept, is not read
    if name in ("one", "every third", "repeat"):
        import re
        tok = list(re.finditer(rb"\S+", tc.line_of(text, lb, 0)))[4 + 1]       # sample column 1 of line 0
        text = text[:tok.start()] + b"x" * (tok.end() - tok.start()) + text[tok.end():]
    want, want_status = tc.parse_slab(text, lb, ncols, col_idx)
    assert not want_status.any()
    with abi.Tgls(gpu_ctx, ROWS, ncols, col_idx) as obj:
        status, err = feed(obj, text, lb)
        assert err is None and not status.any()
        assert np.array_equal(tc.bits(obj.get_rows()), tc.bits(want))
        assert obj.get_rows(tc.PL).shape == (ROWS, len(col_idx) if col_idx else ncols)


def dictionary_file(seed=3, rows=60, ncols=50):
    rng = np.random.default_rng(seed)
    toks = tc.gl_tokens(rng, rows, ncols, decimals=3)
    lines = [tc.plain_line(r, t) for r, t in enumerate(toks)]
    return lines, tc.slab_of(lines)


def issue_order(chunks):
    """the dictionary the rule gives: each call's new values in ascending order of their bit patterns"""
    out = []
    for want in chunks:
        fresh = np.setdiff1d(np.unique(tc.bits(want)), np.array(out, dtype=np.uint64))
        out.extend(np.sort(fresh).tolist())
    return np.array(out, dtype=np.uint64)


def test_code_numbers_are_a_function_of_the_slabs_alone(gpu_ctx):
    lines, (text, lb) = dictionary_file()
    want, _ = tc.parse_slab(text, lb, 50)
    tables = []
    for _ in range(5):
        with abi.Tgls(gpu_ctx, 60, 50) as obj:
            for a, b in ((0, 25), (25, 60)):
                t, l = tc.slab_of(lines[a:b])
                status, err = feed(obj, t, l, row_begin=a)
                assert err is None and not status.any()
            assert np.array_equal(tc.bits(obj.get_rows()), tc.bits(want))
            tables.append(tc.bits(obj.values()).copy())
    for t in tables:
        assert np.array_equal(t, tables[0])
    # slab A then B holds the union, A's values first, each call's in ascending bit order; issued codes do not move
    assert np.array_equal(tables[0], issue_order([want[:25], want[25:]]))
    assert set(tables[0].tolist()) == set(np.unique(tc.bits(want)).tolist())
    # one slab and row-by-row slabs decode to the same values
    with abi.Tgls(gpu_ctx, 60, 50) as one, abi.Tgls(gpu_ctx, 60, 50) as single:
        feed(one, text, lb)
        for r in range(60):
            t, l = tc.slab_of(lines[r:r + 1])
            feed(single, t, l, row_begin=r)
        assert np.array_equal(tc.bits(one.values()), issue_order([want]))
        assert np.array_equal(tc.bits(single.values()), issue_order([want[r:r + 1] for r in range(60)]))
        for gl_type in (tc.RAW, tc.GL):
            assert np.array_equal(tc.bits(one.get_rows(gl_type)), tc.bits(single.get_rows(gl_type)))
            assert np.array_equal(tc.bits(one.get_rows(gl_type)), tc.bits(tc.convert(want, gl_type)))


def test_the_65537th_raw_value_is_refused(gpu_ctx):
    """260 rows x 256 columns of distinct 5-digit integers: 65,536 values are held, the next one is refused with
    GARLIC_ERR_RANGE, its message names the host reader, and the object is unusable from there on"""
    ncols = 256
    lines = [tc.plain_line(r, [b"%d" % (10000 + r * ncols + c) for c in range(ncols)]) for r in range(260)]
    with abi.Tgls(gpu_ctx, 260, ncols) as obj:
        text, lb = tc.slab_of(lines[:256])
        status, err = feed(obj, text, lb)
        assert err is None and not status.any() and obj.info() == (65536, 256, 0)
        assert np.array_equal(obj.get_rows(row_begin=255, row_count=1)[0], 10000.0 + 255 * ncols + np.arange(ncols))
        text, lb = tc.slab_of(lines[256:])
        with pytest.raises(abi.GarlicError) as e:
            feed(obj, text, lb, row_begin=256)
        assert e.value.code == abi.ERR_RANGE and "host reader" in str(e.value)
        with pytest.raises(abi.GarlicError) as e:
            obj.get_rows(row_begin=0, row_count=1)
        assert e.value.code == abi.ERR_STATE
    with abi.Tgls(gpu_ctx, 260, ncols) as obj:             # the same in one slab
        text, lb = tc.slab_of(lines)
        with pytest.raises(abi.GarlicError) as e:
            feed(obj, text, lb)
        assert e.value.code == abi.ERR_RANGE


def test_a_slab_of_more_distinct_values_than_the_report_set_holds_is_refused(gpu_ctx):
    """520 rows x 256 columns of distinct 6-digit integers: 133,120 unknown values in one slab, more than the 131,072 slots of
    the encode kernel's set -- refused as the 65,537th is, after bounded work (an element that sees the outcome decided
    probes no further)"""
    ncols = 256
    lines = [tc.plain_line(r, [b"%d" % (100000 + r * ncols + c) for c in range(ncols)]) for r in range(520)]
    text, lb = tc.slab_of(lines)
    with abi.Tgls(gpu_ctx, 520, ncols) as obj:
        with pytest.raises(abi.GarlicError) as e:
            feed(obj, text, lb)
        assert e.value.code == abi.ERR_RANGE and "host reader" in str(e.value)
        assert obj.info() == (0, 0, 0)
        with pytest.raises(abi.GarlicError) as e:
            feed(obj, text, lb)
        assert e.value.code == abi.ERR_STATE


def reference_files(tmp_path):
    """the value sets of test_tgls_reader_of_the_host_adapter, and a GL file of 300 distinct 3-decimal values"""
    nloci, nind = 300, 17
    out = []
    for name, gl_type, seed in (("GQ", tc.GQ, 1), ("GL", tc.GL, 2), ("PL", tc.PL, 3), ("GL", tc.GL, 4)):
        rng = np.random.default_rng(seed)
        if seed == 1:
            vals = rng.choice(np.concatenate([np.arange(0, 100), [150, 1000]]), size=(nloci, nind)).astype(float)
        elif seed == 2:
            vals = rng.choice([-0.0004, -0.004, -0.3, -1.0, -3.0, -12.0, 0.0, 0.1], size=(nloci, nind))
        elif seed == 3:
            vals = rng.choice([0.004, 0.04, 3.0, 10.0, 30.0, 120.0, 0.0, -1.0], size=(nloci, nind))
        else:
            vals = rng.permutation(np.arange(300 * 17) % 300).reshape(nloci, nind) + 1

        def spell(v):
            return str(int(v)) if seed == 1 else "-0.%03d" % v if seed == 4 else repr(float(v))
        lines = [b"1 rs%d 0 %d " % (l, l + 1) + b" ".join(spell(v).encode() for v in vals[l]) + b"\n" for l in range(nloci)]
        path = str(tmp_path / f"x{seed}.tgls")
        with open(path, "wb") as f:
            f.write(b"".join(lines))
        out.append((name, gl_type, path, lines, nloci, nind))
    return out


def test_converted_values_are_the_reference_readers(gpu_ctx, tmp_path):
    if not ol.have_ref():
        pytest.skip("oracle/_ref is not built")
    for name, gl_type, path, lines, nloci, nind in reference_files(tmp_path):
        want = np.empty((nloci, nind))
        assert ol.ref().ref_readTGLS(path.encode(), nloci, nind, name.encode(), want.ctypes.data_as(ol._dp)) == 0
        text, lb = tc.slab_of(lines)
        with abi.Tgls(gpu_ctx, nloci, nind) as obj:
            status, err = feed(obj, text, lb)
            assert err is None and not status.any(), (name, status[status[:, 0] != 0][:3])
            assert np.array_equal(tc.bits(obj.get_rows(gl_type)), tc.bits(want)), name
        assert np.array_equal(tc.bits(tc.convert(tc.parse_slab(text, lb, nind)[0], gl_type)), tc.bits(want)), (name, "the model")


W, ERROR, MG = 10, 0.001, 200000


@pytest.mark.parametrize("kind", ["GQ", "GL"])
@pytest.mark.parametrize("ind_offset", [0, 3])
def test_a_panel_filled_from_the_object(gpu_ctx, kind, ind_offset):
    """200 loci x 70 individuals, W = 10: rows dropped at the front, in the middle and at the end, columns from ind_offset on;
    the same mode as the twin the converted doubles fill (GQ: one-byte codes), DICTIONARY16 for the GL file, and scores
    bits_equal to the oracle's"""
    nloci, nind = 200, 70
    rng = np.random.default_rng(11 + ind_offset)
    g, f, pos, cs, ce = ol.random_panel(rng, nloci, nind, max_gap=MG)
    ncols = nind + ind_offset + (2 if ind_offset else 0)
    dropped = [0, 1, 100, 150, 151, 205, 206]
    rows = nloci + len(dropped)
    toks = tc.gq_tokens(rng, rows, ncols) if kind == "GQ" else tc.gl_tokens(rng, rows, ncols, decimals=3)
    gl_type = tc.GQ if kind == "GQ" else tc.GL
    text, lb = tc.slab_of([tc.plain_line(r, t) for r, t in enumerate(toks)])
    raw, _ = tc.parse_slab(text, lb, ncols)
    kept = np.array([r for r in range(rows) if r not in dropped])
    dest = np.full(rows, -1, dtype=np.int64)
    dest[kept] = np.arange(nloci)
    gl = tc.convert(raw[kept][:, ind_offset:ind_offset + nind], gl_type)
    want = ol.oracle_calc_lod(g, f, pos, cs, ce, W, ERROR, MG, gl=gl)

    def open_panel():
        panel = abi.Panel(gpu_ctx, [nloci], nind)
        panel.set_map(pos, [cs], [ce])
        panel.set_freq(f)
        panel.set_genotypes(g)
        return panel

    with abi.Tgls(gpu_ctx, rows, ncols) as obj, open_panel() as panel, open_panel() as twin:
        status, err = feed(obj, text, lb)
        assert err is None and not status.any()
        panel.set_gl_tgls(obj, gl_type, dest, ind_offset=ind_offset)
        twin.set_gl(gl)
        if kind == "GQ":
            assert panel.tgls_mode()[0] == twin.tgls_mode()[0] == abi.TGLS_DICTIONARY
        else:
            assert np.unique(tc.bits(gl)).shape[0] > 256 and panel.tgls_mode()[0] == abi.TGLS_DICTIONARY16
        got = panel.lod_windows(W, ERROR, MG, use_gl=True, pitch_align=32)
        assert ol.bits_equal(np.ascontiguousarray(got[0]), want), ol.count_mismatch(np.ascontiguousarray(got[0]), want)
        assert ol.bits_equal(np.ascontiguousarray(twin.lod_windows(W, ERROR, MG, use_gl=True, pitch_align=32)[0]), want)
        bad = dest.copy()
        bad[[5, 6]] = bad[[6, 5]]
        with pytest.raises(abi.GarlicError) as e:
            panel.set_gl_tgls(obj, gl_type, bad, ind_offset=ind_offset)
        assert e.value.code == abi.ERR_INVALID and "ascending" in str(e.value)
