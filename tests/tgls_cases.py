"""--tgls text: generators and a pure-Python model of garlic_tgls (csrc/tgls_kernels.hpp, csrc/tgls_number.hpp).

The model is independent of the code under test: float(token) is the correctly rounded value of a decimal, bytes.split() splits
where isspace() does (space, \\t, \\n, \\v, \\f, \\r -- what operator>> and countFields of the reader take for separators), and
the conversion of garlic-data.cpp:1557-1576 is restated with math.pow, which is the host libm's pow."""
import math
import re

import numpy as np

OK, DEFERRED, FEW, MANY = 0, 1, 2, 3
GQ, GL, PL, RAW = 0, 1, 2, -1
TOKEN_MAX = 32
PASS_BYTES = 4096

_NUMBER = re.compile(rb"^[+-]?(?:(\d+)(?:\.(\d*))?|\.(\d+))(?:[eE]([+-]?\d+))?$")


def defers(tok):
    """what tgls_number leaves to the host: outside the grammar, longer than 32 bytes, digits past 2^53, |exponent| > 22"""
    if len(tok) > TOKEN_MAX:
        return True
    m = _NUMBER.match(tok)
    if not m:
        return True
    whole, frac, bare, exp = m.group(1), m.group(2), m.group(3), m.group(4)
    digits = (whole or b"") + (frac or b"") + (bare or b"")
    mant = int(digits)
    if mant == 0:
        return False
    if len(digits.lstrip(b"0")) > 19:
        return True
    e = int(exp or 0) - len((frac or b"") + (bare or b""))
    return mant > 2 ** 53 or abs(e) > 22


def line_of(text, lb, r):
    line = text[lb[r]:min(lb[r + 1], len(text))]
    nl = line.find(b"\n")
    return line if nl < 0 else line[:nl]


def parse_slab(text, lb, ncols, col_idx=None):
    """-> (raw float64 [rows][n_kept] with NaN where the model has no value, status int32 [rows][2])"""
    text = bytes(text)
    idx = np.arange(ncols) if col_idx is None else np.asarray(col_idx)
    kept = set(int(c) for c in idx)
    rows = len(lb) - 1
    raw = np.full((rows, len(idx)), np.nan)
    status = np.zeros((rows, 2), dtype=np.int32)
    for r in range(rows):
        samples = line_of(text, lb, r).split()[4:]
        offence = None
        full = np.full(ncols, np.nan)
        for j, tok in enumerate(samples):
            if j >= ncols:
                offence = offence or (MANY, ncols)
                break
            if j in kept:
                if defers(tok):
                    offence = offence or (DEFERRED, j)
                else:
                    full[j] = float(tok)
        if len(samples) < ncols:
            offence = offence or (FEW, len(samples))
        if offence:
            status[r] = offence
        raw[r] = full[idx]
    return raw, status


def host_values(text, lb, ncols, col_idx=None):
    """the rows as the host's stream parse reads them (every token a plain decimal here): float of every kept token"""
    idx = np.arange(ncols) if col_idx is None else np.asarray(col_idx)
    out = np.empty((len(lb) - 1, len(idx)))
    for r in range(len(lb) - 1):
        toks = line_of(bytes(text), lb, r).split()[4:]
        out[r] = np.array([float(t) for t in toks])[idx]
    return out


def convert(raw, gl_type):
    """garlic-data.cpp:1557-1576 operation for operation, per distinct value"""
    raw = np.asarray(raw, dtype=np.float64)
    if gl_type == RAW:
        return raw.copy()
    uniq, inv = np.unique(raw.view(np.uint64), return_inverse=True)
    table = np.empty(uniq.shape[0])
    for k, v in enumerate(uniq.view(np.float64)):
        gl = float(v)
        if gl_type in (GQ, PL):
            gl = gl / -10.0
        gl = gl if gl > -10 else -10.0
        gl = math.pow(10.0, gl)
        if gl_type != GQ:
            gl = 1 - gl
        if gl <= 0:
            gl = 0.0000000000000001
        if gl > 1:
            gl = 1.0
        table[k] = gl
    return table[inv].reshape(raw.shape)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------ generators

def gq_tokens(rng, rows, ncols, one_byte=False):
    hi = 10 if one_byte else 100
    return [[b"%d" % v for v in rng.integers(0, hi, size=ncols)] for _ in range(rows)]


def pl_tokens(rng, rows, ncols):
    return [[b"%d" % v for v in rng.integers(0, 256, size=ncols)] for _ in range(rows)]


def gl_tokens(rng, rows, ncols, decimals=4):
    out = []
    for _ in range(rows):
        vals = -rng.integers(0, 12 * 10 ** decimals, size=ncols) / 10 ** decimals
        out.append([("%.*f" % (int(rng.integers(1, decimals + 1)), v)).encode() for v in vals])
    return out


def pad_token(tok, width):
    """the same number in `width` bytes: zeros between the sign and the digits"""
    sign = tok[:1] if tok[:1] in b"+-" else b""
    body = tok[len(sign):]
    if body[:1] == b".":
        body = b"0" + body
    return sign + b"0" * max(0, width - len(sign) - len(body)) + body


def sep(rng, lo=1, hi=5):
    return bytes(rng.choice([0x20, 0x09], size=int(rng.integers(lo, hi + 1))).tolist())


def plain_line(r, toks, eol=b"\n"):
    return b"1 rs%d 0.%d %d " % (r, r, 100 + r) + b" ".join(toks) + eol


def padded_line(rng, r, toks, target=None, lead=b"", trail=b"", eol=b"\n", planted=None):
    """tokens padded to 12..24 bytes and separated by runs of 1..5 spaces and tabs.  target: one token (the first that can)
    begins exactly `target` bytes into the line; planted: the bytes that stand there instead of the padded token.
    -> (line, column of the token at target or None)"""
    line = lead + b"1" + sep(rng) + b"rs%d" % r + sep(rng) + b"0.5" + sep(rng) + b"%d" % (100 + r) + sep(rng)
    at_target = None
    for j, tok in enumerate(toks):
        pos = len(line)
        if target is not None and pos == target and at_target is None:
            at_target = j
            if planted is not None:
                tok = planted
        width, s = int(rng.integers(12, 25)), sep(rng)
        if target is not None and at_target is None and pos < target:
            left = target - pos
            if 13 <= left <= 29:
                width = min(24, left - 1)
                s = sep(rng, left - width, left - width)
            elif 30 <= left <= 58:
                stride = min(29, max(13, left - 20))
                width = min(24, stride - 1)
                s = sep(rng, stride - width, stride - width)
        line += (tok if at_target == j and planted is not None else pad_token(tok, width)) + (s if j + 1 < len(toks) else b"")
    return line + trail + eol, at_target


def slab_of(lines, between=None):
    """-> (text, line_begin): the lines back to back; between[r]: bytes the caller leaves out in front of line r"""
    text, lb = b"", []
    for r, line in enumerate(lines):
        if between and between.get(r):
            text += between[r]
        lb.append(len(text))
        text += line
    lb.append(len(text))
    return text, np.array(lb, dtype=np.int64)


def write_file(path, token_rows):
    with open(path, "wb") as f:
        for r, toks in enumerate(token_rows):
            f.write(plain_line(r, toks))
