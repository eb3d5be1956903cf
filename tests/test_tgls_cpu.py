"""CPU: the host side of csrc/tgls_number.hpp against strtod, in a stand-alone program under -fsanitize=address,undefined
(tests/host_unit/tgls_number_unit.cpp, run as a child process), and the model of tests/tgls_cases.py against itself."""
import os
import subprocess

import numpy as np
import pytest

import tgls_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def unit(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tgls_number") / "tgls_number_unit")
    src = os.path.join(ROOT, "tests", "host_unit", "tgls_number_unit.cpp")
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=undefined", "-o", exe, src], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    return exe


def test_every_value_is_strtods_and_everything_else_defers(unit):
    """0..120, every -d.ddd of up to 4 decimals over a grid, signed zeros, the edges of the fast path (2^53, 1e22, 1e-22 in; 2^53
    + 1, 1e23, 1e-23, 16-digit significands past 2^53, inf, nan, hex floats out) and 10^6 random tokens of <= 15 digits and
    |e| <= 22, which must all get values"""
    run = subprocess.run([unit], capture_output=True, text=True)
    assert run.returncode == 0 and "tgls_number_unit ok" in run.stdout, (run.stdout + run.stderr)[-3000:]


@pytest.mark.parametrize("kind", ["GQ", "PL", "GL"])
def test_no_token_of_the_generated_files_defers(unit, tmp_path, kind):
    """the GPU parity tests read these generators' files: they must not be able to pass by deferring"""
    rng = np.random.default_rng(5)
    rows = {"GQ": tc.gq_tokens, "PL": tc.pl_tokens, "GL": tc.gl_tokens}[kind](rng, 200, 50)
    path = str(tmp_path / "x.tgls")
    tc.write_file(path, rows)
    run = subprocess.run([unit, "--file", path], capture_output=True, text=True)
    assert run.returncode == 0 and "tokens 10000 deferred 0" in run.stdout, (run.stdout + run.stderr)[-3000:]
    assert not any(tc.defers(t) for toks in rows for t in toks)
    # the padded spellings of the same tokens as well
    padded = [[tc.pad_token(t, int(rng.integers(12, 25))) for t in toks] for toks in rows]
    tc.write_file(path, padded)
    run = subprocess.run([unit, "--file", path], capture_output=True, text=True)
    assert run.returncode == 0 and "tokens 10000 deferred 0" in run.stdout, (run.stdout + run.stderr)[-3000:]


def test_the_models_defer_rule_is_the_headers(unit, tmp_path):
    """tgls_cases.defers names the tokens the program defers: checked through --file on a line of edge tokens"""
    toks = [b"9007199254740992", b"9007199254740993", b"1e22", b"1e23", b"1e-22", b"1e-23", b"inf", b"nan", b"0x1p3", b".5", b"5.",
            b"+5", b"-0", b"1e", b"0e1000000", b"1234567890123456", b"12345678901234567", b"0.000000000000000000000001",
            b"000000000000000000000000000012.5", b"0000000000000000000000000000012.5", b"1.2.3", b"--1"]
    want = sum(tc.defers(t) for t in toks)
    assert want == 12      # 2^53 + 1, 1e23, 1e-23, inf, nan, 0x1p3, 1e, 17 digits, 1e-24, 33 bytes, 1.2.3, --1
    path = str(tmp_path / "edge.tgls")
    tc.write_file(path, [toks])
    run = subprocess.run([unit, "--file", path], capture_output=True, text=True)
    assert run.returncode == 0 and "tokens %d deferred %d" % (len(toks), want) in run.stdout, (run.stdout + run.stderr)[-3000:]


def test_model_of_a_slab():
    rng = np.random.default_rng(1)
    toks = tc.gq_tokens(rng, 3, 5)
    lines = [tc.plain_line(0, toks[0]), b"  \t" + tc.plain_line(1, toks[1], eol=b" \r\n"), tc.plain_line(2, toks[2][:4]),
             tc.plain_line(3, toks[0] + [b"7"]), tc.plain_line(4, [b"1", b"nan", b"2", b"1e99", b"3"], eol=b"")]
    text, lb = tc.slab_of(lines, between={1: b"skipped line\n"})
    raw, status = tc.parse_slab(text, lb, 5)
    assert status.tolist() == [[0, 0], [0, 0], [tc.FEW, 4], [tc.MANY, 5], [tc.DEFERRED, 1]]
    assert raw[1].tolist() == [float(t) for t in toks[1]]
    sub, st = tc.parse_slab(text, lb, 5, col_idx=[4, 0, 0])
    assert st[4].tolist() == [0, 0] and sub[4].tolist() == [3.0, 1.0, 1.0]
    line, col = tc.padded_line(rng, 0, [b"5"] * 400, target=4090)
    assert col is not None and line[4089:4090] in b" \t" and line[4090:4091] not in b" \t"
    assert tc.convert(np.array([0.0, 30.0, 1000.0]), tc.GQ).tolist() == [1.0, 0.001, 1e-10]
    assert tc.convert(np.array([0.0, -1.0, -12.0]), tc.GL).tolist() == [1e-16, 0.9, 1 - 1e-10]


# ------------------------------------------------- the conditions of tests/test_gpu_tgls_number.py, checked without a GPU

V, D = "value", "deferred"
GRAMMAR = [
    (b"+5", V), (b".5", V), (b"-.5", V), (b"5.", V), (b"+5.e0", V), (b"1E2", V), (b"1e+2", V), (b"1e-2", V), (b"1e0002", V), (b"1e-0", V),
    (b"-12.5E-1", V),
    (b"0", V), (b"-0", V), (b"-0.0", V), (b"+0.000", V), (b"0e99999999999", V), (b"-0e-99999999999", V), (b"-.0", V), (b"0.", V),
    (b"9007199254740992", V), (b"9007199254740993", D), (b"900719925474099.2e1", V), (b"-9007199254740992", V), (b"9007199254740991", V),
    (b"4503599627370497e-1", V),
    (b"1e22", V), (b"1e23", D), (b"1e-22", V), (b"1e-23", D), (b"1.5e23", V), (b"0.001e26", D), (b"0.001e25", V),
    (b"0.0000000000000000000001", V), (b"0.00000000000000000000001", D), (b"9007199254740992e22", V), (b"9007199254740991e-22", V),
    (b"999999999999999999", D), (b"1000000000000000000", D), (b"10000000000000000000", D), (b"0000000000000000000001", V),
    (b"1.000000000000000", V), (b"1.0000000000000000", D), (b"00.10", V),
    (b"0000000000000000.123456789012345", V), (b"00000000000000000000000000000001", V), (b"000000000000000000000000000000001", D),
    (b"-00000000000000000000000000001e1", V),
    (b"1e", D), (b"1e+", D), (b"e5", D), (b".", D), (b"+", D), (b"-", D), (b"1.2.3", D), (b"--1", D), (b"1_0", D), (b"inf", D), (b"nan", D),
    (b"0x1p3", D), (b"1d5", D)]


def file_mode(unit, path):
    run = subprocess.run([unit, "--file", path], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    return run.stdout


def test_grammar_tokens_are_classified_as_listed(unit, tmp_path):
    """every class has a member, the valued and the deferred tokens are the ones named here, and the header agrees: one line
    of all of them through --file (which fails on a value other than strtod's) defers that many"""
    got = tc.grammar_tokens()
    assert set(c for _, c in got) == {"form", "zero", "mantissa", "exponent", "digits", "length", "outside"}
    assert [t for t, _ in got] == [t for t, _ in GRAMMAR] and len(set(t for t, _ in got)) == len(got)
    assert [(t, D if tc.defers(t) else V) for t, _ in got] == GRAMMAR
    assert sum(tc.defers(t) for t, _ in got) == 23 and len(got) == 60
    assert all(tc.defers(t) for t, c in got if c == "outside") and not any(tc.defers(t) for t, c in got if c in ("form", "zero"))
    assert len(got[43][0]) == 32 and len(got[44][0]) == 32 and len(got[45][0]) == 33 and len(got[46][0]) == 32
    assert tc.mantissa_exponent(b"0.0000000000000000000001") == (1, -22) and tc.mantissa_exponent(b"1.5e23") == (15, 22)
    assert tc.mantissa_exponent(b"900719925474099.2e1") == (2 ** 53, 0) and tc.mantissa_exponent(b"0.001e26") == (1, 23)
    # the sign of a zero is the token's
    for t, c in got:
        if c == "zero":
            assert tc.bits(float(t))[()] == (0x8000000000000000 if t[:1] == b"-" else 0), t
    path = str(tmp_path / "grammar.tgls")
    tc.write_file(path, [[t for t, _ in got]])
    assert "tokens 60 deferred 23" in file_mode(unit, path)


def test_no_spelled_token_defers(unit, tmp_path):
    """10,000 spelled() tokens: at most 32 bytes, in the grammar, the value m * 10^e exactly, every form drawn, and the header
    gives each a value (strtod's, or --file fails)"""
    from fractions import Fraction
    rng = np.random.default_rng(8)
    toks = []
    for _ in range(10000):
        m, e = int(2 ** (53 * rng.random())), int(rng.integers(-22, 23))
        tok = tc.spelled(rng, m, e)
        mm, ee = tc.mantissa_exponent(tok)
        assert len(tok) <= tc.TOKEN_MAX and not tc.defers(tok) and 1 <= mm <= 2 ** 53 and abs(ee) <= 22
        assert Fraction(mm) * Fraction(10) ** ee == Fraction(m) * Fraction(10) ** e, (tok, m, e)
        assert abs(float(tok)) == float(Fraction(m) * Fraction(10) ** e) and (float(tok) < 0) == (tok[:1] == b"-")
        toks.append(tok)
    assert tc.spelled(rng, 2 ** 53, 22) and tc.spelled(rng, 2 ** 53, -22, sign=b"-")[:1] == b"-"
    for what in (lambda t: t[:1] == b"+", lambda t: t[:1] == b"-", lambda t: b"e" in t, lambda t: b"E" in t, lambda t: b"e+" in t,
                 lambda t: b"e-" in t, lambda t: b"." not in t, lambda t: t.lstrip(b"+-")[:1] == b".", lambda t: t.lstrip(b"+-")[:2] == b"0.",
                 lambda t: t.lstrip(b"+-")[:2] == b"00", lambda t: b".e" in t or b".E" in t or t[-1:] == b".",
                 lambda t: tc.mantissa_exponent(t)[1] > 0, lambda t: tc.mantissa_exponent(t)[1] < 0, lambda t: len(t) > 24):
        assert sum(map(what, toks)) >= 200
    path = str(tmp_path / "spelled.tgls")
    tc.write_file(path, [toks[r:r + 50] for r in range(0, 10000, 50)])
    assert "tokens 10000 deferred 0" in file_mode(unit, path)


def test_hard_cases_lie_near_midpoints_and_none_defers(unit, tmp_path):
    """deterministic for the seed; every pair nearer a midpoint than the median of its sample; both operations; the plain and
    a spelled() token of each get strtod's value from the header"""
    from fractions import Fraction
    cases = tc.hard_cases()
    assert len(cases) == len(set(cases)) == 256
    tc.hard_ranking.cache_clear()
    assert tc.hard_cases() == cases
    small = tc.hard_cases(seed=5, sample=2000, keep=16)
    tc.hard_ranking.cache_clear()
    assert tc.hard_cases(seed=5, sample=2000, keep=16) == small and small != tc.hard_cases(seed=6, sample=2000, keep=16)
    ranked = tc.hard_ranking(20240611, 200000)
    median = ranked[len(ranked) // 2][0]
    assert median > Fraction(1, 4)
    for m, k, op in cases:
        assert 1 <= m <= 2 ** 53 and 1 <= k <= 22 and tc.midpoint_distance(m, k, op) < median / 100
    assert sum(op == "*" for _, _, op in cases) == 128 and sum(op == "/" for _, _, op in cases) == 128
    assert sum(tc.midpoint_distance(*c) == 0 for c in cases) == 64
    # m is log-uniform, so 3 in 53 of either operation's 128 are expected past 2^50: operands of full width are among them
    assert all(any(m >= 2 ** 50 and op == o and tc.midpoint_distance(m, k, op) > 0 for m, k, op in cases) for o in "*/")
    # the distance is what it says: 2^53 + 1 lies on a midpoint, a double is half a spacing from the next one
    assert tc.midpoint_distance((2 ** 53 + 1) * 5, 1, "/") == 0 and tc.midpoint_distance(3, 1, "*") == Fraction(1, 2)
    assert tc.midpoint_distance(1, 1, "/") == abs(Fraction(1, 10) * 2 ** 56 % 1 - Fraction(1, 2))
    rng = np.random.default_rng(9)
    plain = [tc.plain_spelling(*c) for c in cases]
    other = [tc.spelled(rng, m, k if op == "*" else -k) for m, k, op in cases]
    for c, a, b in zip(cases, plain, other):
        assert abs(float(b)) == float(a) == float(Fraction(c[0]) * Fraction(10) ** (c[1] if c[2] == "*" else -c[1]))
    path = str(tmp_path / "hard.tgls")
    tc.write_file(path, [plain, other])
    assert "tokens 512 deferred 0" in file_mode(unit, path)


def test_blank_line_and_placed_line():
    toks = [b"1", b"-0", b"2e1"]
    line = tc.blank_line(toks, [b"\v", b"\f", b"\r", b" \t\v\f\r", b"\r"], r=3, eol=b"\r\n")
    assert line.split() == [b"1", b"rs3", b"0.5", b"103"] + toks and line.startswith(b"\v1") and line.endswith(b"2e1\r\r\n")
    assert set(tc.BLANKS + b"\n") == set(c for c in range(256) if bytes([c]).isspace())
    for c in tc.FOREIGN:
        assert (b"1" + bytes([c]) + b"2").split() == [b"1" + bytes([c]) + b"2"]
    for q in range(16):
        for begin in (0, 7, 100):
            line = tc.placed_line(2, begin, q, b"12.5", [b"3"], front=[b"9"])
            assert line.split()[4:] == [b"9", b"12.5", b"3"] and (begin + line.index(b"12.5")) % 16 == q
