"""GPU: the device build of tgls_number (csrc/tgls_number.hpp) and the token geometry of tgls_parse_kernel at the grammar's
edges, bit for bit against float(token) through the model of tests/tgls_cases.py.  tests/test_gpu_tgls_text.py covers the
slab geometry with plain integers and short negative decimals; here the tokens are the point: every form of the grammar and
every border of the fast path at every start byte of a 16-byte slot, token lengths across the 32-byte look-ahead, random
spellings of m * 10^e on both branches (m up to 2^53, |e| <= 22), the quotients and products nearest a rounding midpoint,
every isspace() byte as a separator and its neighbours inside a token, and the two zeros as two dictionary values.
tests/test_tgls_cpu.py checks without a GPU that none of the valued tokens can pass by being deferred.  No tolerance: every
comparison is on the uint64 views of the doubles."""
import numpy as np
import pytest

import oracle_lib as ol
import tgls_cases as tc
from garlic_amd import abi
from test_gpu_tgls_text import feed

pytestmark = pytest.mark.gpu

PLAIN = [b"7", b"-1.25", b"3"]
STAND_IN = 0.25            # what the test brings for a token no reader gives a number


def completed(want_row):
    """the row the host brings for a deferred one: the model's values, STAND_IN where it has none"""
    return np.where(np.isnan(want_row), STAND_IN, want_row)[None, :]


def check_slab(gpu_ctx, text, lb, ncols, where, tag):
    """feed the slab; statuses equal the model's; clean rows equal it bit for bit; deferred rows do after completion"""
    want, want_status = tc.parse_slab(text, lb, ncols)
    rows = len(lb) - 1
    with abi.Tgls(gpu_ctx, rows, ncols) as obj:
        status, err = feed(obj, text, lb, where)
        assert err is None, (tag, err)
        assert np.array_equal(status, want_status), (tag, np.argwhere(status != want_status)[:5], status[(status != want_status).any(1)][:5])
        deferred = np.flatnonzero(want_status[:, 0] == tc.DEFERRED)
        assert obj.info()[1:] == (rows - len(deferred), len(deferred))
        for r in deferred:
            obj.set_rows_values(completed(want[r]), row_begin=int(r))
        got = obj.get_rows()
        full = np.where(np.isnan(want), STAND_IN, want)
        assert np.array_equal(tc.bits(got), tc.bits(full)), (tag, np.argwhere(tc.bits(got) != tc.bits(full))[:5])
        assert obj.info() == (np.unique(tc.bits(full)).shape[0], rows, 0)
    return want, want_status


@pytest.mark.parametrize("q", range(16))
def test_every_grammar_token_at_every_start_byte(gpu_ctx, q):
    """one line per token, the token at byte q of an aligned piece (the slab itself is aligned), three plain tokens behind it
    so that a wrong length shows in the neighbours; valued and deferred lines share the slab"""
    grammar = tc.grammar_tokens()
    lines, begin = [], 0
    for r, (tok, _) in enumerate(grammar):
        lines.append(tc.placed_line(r, begin, q, tok, PLAIN))
        begin += len(lines[-1])
    text, lb = tc.slab_of(lines)
    want, want_status = check_slab(gpu_ctx, text, lb, 4, "dev0", q)
    for r, (tok, _) in enumerate(grammar):
        assert (int(lb[r]) + lines[r].index(b" " + PLAIN[0]) - len(tok)) % 16 == q
        if tc.defers(tok):
            assert want_status[r].tolist() == [tc.DEFERRED, 0] and np.isnan(want[r, 0])
        else:
            assert want_status[r].tolist() == [0, 0] and tc.bits(want[r, 0])[()] == tc.bits(float(tok))[()]
        assert want[r, 1:].tolist() == [7.0, -1.25, 3.0]
    assert (want_status[:, 0] == tc.DEFERRED).sum() == 23


LENGTHS = list(range(24, 35)) + [47, 48, 49, 100]


def long_token(L, k):
    return b"0" * (L - 3) + b"%03d" % (100 + k)


def sweep_slabs():
    """-> [(tag, text, lb, ncols, column of the long token)].  The short lines: a plain column, the L-byte token at byte q of
    a piece, two plain columns.  The long lines begin on a piece (bytes left out in front of them see to it), so that their
    first pass ends 4096 bytes in: 252 fifteen-byte columns, then the token with its first byte in that pass's last slot"""
    lines, begin, k = [], 0, 0
    for L in LENGTHS:
        for q in (0, 1, 14, 15):
            lines.append(tc.placed_line(k, begin, q, long_token(L, k), [b"42", b"-0.5"], front=[b"5"]))
            begin += len(lines[-1])
            k += 1
    short = tc.slab_of(lines)
    lines, between, begin = [], {}, 0
    for i, L in enumerate(LENGTHS):
        q = (0, 15, 1, 14)[i % 4]
        between[i] = b"#" * ((-begin) % 16)
        begin += len(between[i])
        front = [b"%015d" % (1000 * i + c) for c in range(252)]
        line = tc.placed_line(i, begin, q, long_token(L, i), [b"42", b"-0.5"], front=front, not_before=tc.PASS_BYTES - 16)
        start = line.index(b" 42") - L
        assert begin % 16 == 0 and tc.PASS_BYTES - 16 <= start < tc.PASS_BYTES and start % 16 == q, (L, start)
        lines.append(line)
        begin += len(line)
    astride = tc.slab_of(lines, between=between)
    return [("short", short[0], short[1], 4, 1), ("astride", astride[0], astride[1], 255, 252)]


def test_token_lengths_across_the_look_ahead(gpu_ctx):
    """L <= 32 has its value and L >= 33 is (DEFERRED, its column), wherever the token starts; with the long token's column
    not kept the line is clean and the tokens around it have their columns and values"""
    for tag, text, lb, ncols, col in sweep_slabs():
        assert len(text) < 400000
        want, want_status = check_slab(gpu_ctx, text, lb, ncols, "dev0", tag)
        per_line = [len(tc.line_of(text, lb, r).split()[4 + col]) for r in range(len(lb) - 1)]
        assert sorted(set(per_line)) == LENGTHS
        for r, L in enumerate(per_line):
            assert want_status[r].tolist() == ([0, 0] if L <= 32 else [tc.DEFERRED, col]), (tag, r, L)
            assert want[r, col + 1] == 42.0 and want[r, col + 2] == -0.5 and (L > 32 or want[r, col] == 100 + r)
        others = [c for c in range(ncols) if c != col]
        rest, rest_status = tc.parse_slab(text, lb, ncols, others)
        assert not rest_status.any() and not np.isnan(rest).any()
        with abi.Tgls(gpu_ctx, len(lb) - 1, ncols, others) as obj:
            status, err = feed(obj, text, lb, "dev0")
            assert err is None and not status.any(), (tag, status[status[:, 0] != 0][:5])
            assert np.array_equal(tc.bits(obj.get_rows()), tc.bits(rest)), tag


def spelled_rows(rows=40, ncols=300, seed=31):
    rng = np.random.default_rng(seed)
    pool = [int(2 ** (53 * u)) for u in rng.random(4000)]
    pool[:2] = [2 ** 53, 1]
    return [[tc.spelled(rng, pool[int(rng.integers(0, 4000))], int(rng.integers(-22, 23))) for _ in range(ncols)] for _ in range(rows)]


@pytest.mark.parametrize("where", ["host", "dev15"])
def test_random_spellings_on_both_branches(gpu_ctx, where):
    """40 x 300 spellings of m * 10^e, m log-uniform up to 2^53 from a pool of 4,000, e uniform in -22 .. 22 (spelled() fits
    every such pair into 32 bytes, so none is redrawn): no status, every value float(token)"""
    toks = spelled_rows()
    flat = [t for row in toks for t in row]
    net = np.array([tc.mantissa_exponent(t)[1] for t in flat])
    big = np.array([tc.mantissa_exponent(t)[0] for t in flat])
    assert (net > 0).sum() >= len(flat) // 4 and (net < 0).sum() >= len(flat) // 4
    assert (big > 2 ** 40).sum() >= len(flat) // 8 and not any(tc.defers(t) for t in flat)
    rng = np.random.default_rng(32)
    lines = [b"1 rs%d 0.5 %d " % (r, r) + b"".join(t + tc.sep(rng, 1, 3) for t in row) + b"\n" for r, row in enumerate(toks)]
    text, lb = tc.slab_of(lines)
    want, want_status = tc.parse_slab(text, lb, 300)
    assert not want_status.any() and np.array_equal(tc.bits(want), tc.bits(np.array([[float(t) for t in row] for row in toks])))
    distinct = np.unique(tc.bits(want)).size
    assert distinct < 65536
    with abi.Tgls(gpu_ctx, 40, 300) as obj:
        status, err = feed(obj, text, lb, where)
        assert err is None and not status.any(), (where, status[status[:, 0] != 0][:5])
        got = obj.get_rows()
        bad = np.argwhere(tc.bits(got) != tc.bits(want))
        assert bad.shape[0] == 0, [(toks[r][c], hex(tc.bits(got)[r, c]), hex(tc.bits(want)[r, c])) for r, c in bad[:5]]
        assert obj.info() == (distinct, 40, 0)


def test_quotients_and_products_nearest_a_midpoint(gpu_ctx):
    """the 256 hard_cases as m e+-k and in one spelled() form each, the columns of two rows"""
    cases = tc.hard_cases()
    rng = np.random.default_rng(9)
    rows = [[tc.plain_spelling(*c) for c in cases], [tc.spelled(rng, m, k if op == "*" else -k) for m, k, op in cases]]
    text, lb = tc.slab_of([tc.plain_line(r, row) for r, row in enumerate(rows)])
    want, want_status = tc.parse_slab(text, lb, 256)
    assert not want_status.any() and np.array_equal(tc.bits(np.abs(want[1])), tc.bits(want[0]))
    for where in ("host", "dev1"):
        with abi.Tgls(gpu_ctx, 2, 256) as obj:
            status, err = feed(obj, text, lb, where)
            assert err is None and not status.any(), (where, status)
            got = obj.get_rows()
            bad = np.argwhere(tc.bits(got) != tc.bits(want))
            assert bad.shape[0] == 0, [(rows[r][c], hex(tc.bits(got)[r, c]), hex(tc.bits(want)[r, c])) for r, c in bad[:5]]


def separator_lines():
    toks = [b"1", b"-0.5", b"2e1", b".25", b"7.", b"+3", b"-0", b"12"]
    n = len(toks)
    every = tc.BLANKS
    lines = [tc.blank_line(toks, [b""] + [bytes([c])] * n + [b""], r=r) for r, c in enumerate(b"\v\f\r")]
    lines.append(tc.blank_line(toks, [b"\v\f"] + [every[j % 5:] + every[:j % 5] for j in range(n)] + [b"\r \f\t\v"], r=3))
    lines.append(tc.blank_line(toks, [b"\r"] + [every[j % 5:j % 5 + 1] + every[(3 * j) % 5:(3 * j) % 5 + 1] for j in range(n)] + [b"\v"],
                               r=4, eol=b"\r\n"))
    lines.append(tc.blank_line(toks, [b" \t"] + [every[::-1] * 4] * n + [b"\f\f"], r=5, eol=b""))      # 20-byte runs: blank pieces
    return toks, lines


@pytest.mark.parametrize("where", ["host", "dev0", "dev15"])
def test_every_isspace_byte_separates(gpu_ctx, where):
    toks, lines = separator_lines()
    text, lb = tc.slab_of(lines)
    want, want_status = check_slab(gpu_ctx, text, lb, len(toks), where, where)
    assert not want_status.any() and all(row.tolist() == [float(t) for t in toks] for row in want)
    assert np.signbit(want[:, 6]).all()


@pytest.mark.parametrize("where", ["host", "dev15"])
def test_a_foreign_byte_stays_inside_its_token(gpu_ctx, where):
    """8, 14, NUL, 0x80 and 0xFF are no blanks: the token they stand in is one token and deferred, not two columns"""
    toks = [b"1", b"-0.5", b"2e1", b".25", b"7.", b"+3", b"-0", b"12"]
    lines, cols = [], []
    for r, c in enumerate(tc.FOREIGN):
        col = (2 * r + 1) % len(toks)
        spoilt = list(toks)
        spoilt[col] = (b"1" + bytes([c]) + b"2", bytes([c]) + b"5", b"5" + bytes([c]))[r % 3]
        lines.append(tc.blank_line(spoilt, [b""] + [tc.BLANKS[(r + j) % 5:(r + j) % 5 + 1] for j in range(len(toks))] + [b""], r=r))
        cols.append(col)
    text, lb = tc.slab_of(lines)
    want, want_status = check_slab(gpu_ctx, text, lb, len(toks), where, where)
    assert want_status.tolist() == [[tc.DEFERRED, col] for col in cols]
    for r, col in enumerate(cols):
        keep = np.arange(len(toks)) != col
        assert np.isnan(want[r, col]) and want[r, keep].tolist() == [float(t) for j, t in enumerate(toks) if j != col]


ZEROS = [b"0", b"-0", b"0.0", b"-0.000", b"0e5"]
OTHERS = [b"-0.001", b"-.5", b"-1", b"-3.25", b"-12", b"0.1", b"1e-3", b"-2.5e-1", b"+2", b"-1E1", b"30", b"-7.", b"-1.5e+1"]
W, ERROR, MG = 10, 0.001, 200000


def zeros_file(rows=60, ncols=50, seed=41):
    rng = np.random.default_rng(seed)
    toks = [[ZEROS[int(rng.integers(0, 5))] if rng.random() < 0.5 else OTHERS[int(rng.integers(0, 13))] for _ in range(ncols)]
            for _ in range(rows)]
    return toks, tc.slab_of([tc.plain_line(r, t) for r, t in enumerate(toks)])


def test_the_two_zeros_are_two_values(gpu_ctx):
    toks, (text, lb) = zeros_file()
    want, want_status = tc.parse_slab(text, lb, 50)
    assert not want_status.any()
    b = tc.bits(want)
    assert (b == 0).sum() > 300 and (b == 0x8000000000000000).sum() > 300 and np.unique(b).size == 2 + len(OTHERS)
    assert np.array_equal(np.signbit(want), np.array([[t[:1] == b"-" for t in row] for row in toks]))
    with abi.Tgls(gpu_ctx, 60, 50) as obj:
        status, err = feed(obj, text, lb)
        assert err is None and not status.any()
        assert obj.info() == (2 + len(OTHERS), 60, 0)
        assert np.array_equal(tc.bits(obj.get_rows(tc.RAW)), b)
        assert sorted(tc.bits(obj.values()).tolist()) == np.unique(b).tolist()
        for gl_type in (tc.GQ, tc.GL, tc.PL):
            conv = tc.convert(want, gl_type)
            assert np.array_equal(tc.bits(obj.get_rows(gl_type)), tc.bits(conv)), gl_type
            both = [np.unique(tc.bits(conv[b == z])) for z in (0, 0x8000000000000000)]          # one likelihood for the two zeros
            assert both[0].size == 1 and np.array_equal(both[0], both[1]), gl_type


@pytest.mark.parametrize("kind", ["GQ", "GL"])
def test_a_panel_of_both_zeros(gpu_ctx, kind):
    """50 individuals x 60 loci, W = 10: scores bits_equal to the oracle's for the converted values, and to the twin's that
    set_gl fills with them"""
    nloci, nind = 60, 50
    gl_type = tc.GQ if kind == "GQ" else tc.GL
    toks, (text, lb) = zeros_file()
    raw, _ = tc.parse_slab(text, lb, nind)
    gl = tc.convert(raw, gl_type)
    rng = np.random.default_rng(42)
    g, f, pos, cs, ce = ol.random_panel(rng, nloci, nind, max_gap=MG)
    want = ol.oracle_calc_lod(g, f, pos, cs, ce, W, ERROR, MG, gl=gl)

    def open_panel():
        panel = abi.Panel(gpu_ctx, [nloci], nind)
        panel.set_map(pos, [cs], [ce])
        panel.set_freq(f)
        panel.set_genotypes(g)
        return panel

    with abi.Tgls(gpu_ctx, nloci, nind) as obj, open_panel() as panel, open_panel() as twin:
        status, err = feed(obj, text, lb)
        assert err is None and not status.any()
        panel.set_gl_tgls(obj, gl_type, np.arange(nloci))
        twin.set_gl(gl)
        got = panel.lod_windows(W, ERROR, MG, use_gl=True, pitch_align=32)
        assert ol.bits_equal(np.ascontiguousarray(got[0]), want), ol.count_mismatch(np.ascontiguousarray(got[0]), want)
        assert ol.bits_equal(np.ascontiguousarray(twin.lod_windows(W, ERROR, MG, use_gl=True, pitch_align=32)[0]), want)


def test_both_zeros_through_the_reference_reader(gpu_ctx, tmp_path):
    if not ol.have_ref():
        pytest.skip("oracle/_ref is not built")
    toks, (text, lb) = zeros_file()
    path = str(tmp_path / "zeros.tgls")
    with open(path, "wb") as f:
        f.write(text)
    with abi.Tgls(gpu_ctx, 60, 50) as obj:
        status, err = feed(obj, text, lb)
        assert err is None and not status.any()
        for name, gl_type in (("GQ", tc.GQ), ("GL", tc.GL), ("PL", tc.PL)):
            want = np.empty((60, 50))
            assert ol.ref().ref_readTGLS(path.encode(), 60, 50, name.encode(), want.ctypes.data_as(ol._dp)) == 0
            assert np.array_equal(tc.bits(obj.get_rows(gl_type)), tc.bits(want)), name
