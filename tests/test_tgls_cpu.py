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
