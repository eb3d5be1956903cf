"""--tgls text: generators and a pure-Python model of garlic_tgls (csrc/tgls_kernels.hpp, csrc/tgls_number.hpp).

The model is independent of the code under test: float(token) is the correctly rounded value of a decimal, bytes.split() splits
where isspace() does (space, \\t, \\n, \\v, \\f, \\r -- what operator>> and countFields of the reader take for separators), and
the conversion of garlic-data.cpp:1557-1576 is restated with math.pow, which is the host libm's pow."""
import functools
import math
import re
from fractions import Fraction

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


def mantissa_exponent(tok):
    """a token of the grammar as tgls_number reads it -> (m, e): every digit in m, the fraction digits folded into e"""
    g = _NUMBER.match(tok)
    whole, frac, bare, exp = g.group(1), g.group(2), g.group(3), g.group(4)
    fraction = (frac or b"") + (bare or b"")
    return int((whole or b"") + fraction), int(exp or 0) - len(fraction)


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


# ------------------------------------------------------------------------ number forms, fast-path borders, separators

BLANKS = b" \t\v\f\r"                 # isspace() without the newline, which ends the line
FOREIGN = [0x08, 0x0E, 0x00, 0x80, 0xFF]      # the neighbours of 9..13, NUL and bytes with the top bit: part of a token


def grammar_tokens():
    """[(token, class)]: the forms of the grammar, the zeros, the borders of the fast path and what lies outside.  Which of
    them have a value is not written here: defers() says it, and tests/test_tgls_cpu.py spells the expectation out"""
    out = [(t, "form") for t in (b"+5", b".5", b"-.5", b"5.", b"+5.e0", b"1E2", b"1e+2", b"1e-2", b"1e0002", b"1e-0", b"-12.5E-1")]
    out += [(t, "zero") for t in (b"0", b"-0", b"-0.0", b"+0.000", b"0e99999999999", b"-0e-99999999999", b"-.0", b"0.")]
    out += [(t, "mantissa") for t in (b"9007199254740992", b"9007199254740993", b"900719925474099.2e1", b"-9007199254740992",
                                      b"9007199254740991", b"4503599627370497e-1")]
    out += [(t, "exponent") for t in (b"1e22", b"1e23", b"1e-22", b"1e-23", b"1.5e23", b"0.001e26", b"0.001e25",
                                      b"0." + b"0" * 21 + b"1", b"0." + b"0" * 22 + b"1", b"9007199254740992e22",
                                      b"9007199254740991e-22")]
    out += [(t, "digits") for t in (b"999999999999999999", b"1000000000000000000", b"10000000000000000000",
                                    b"0000000000000000000001", b"1.000000000000000", b"1.0000000000000000", b"00.10")]
    out += [(t, "length") for t in (b"0" * 16 + b".123456789012345", b"0" * 31 + b"1", b"0" * 32 + b"1", b"-" + b"0" * 28 + b"1e1")]
    out += [(t, "outside") for t in (b"1e", b"1e+", b"e5", b".", b"+", b"-", b"1.2.3", b"--1", b"1_0", b"inf", b"nan", b"0x1p3", b"1d5")]
    return out


def spelled(rng, m, e, sign=None):
    """the value m * 10^e (1 <= m <= 2^53, |e| <= 22) as one token of at most 32 bytes in a form drawn at random: trailing
    zeros behind the digits while m and e stay inside the fast path, the dot inside or in front of the digits (zeros behind
    it included), an e / E exponent for the rest of the power, a sign, leading zeros.  sign: None = drawn, or b"", b"+", b"-" """
    assert 1 <= m <= 2 ** 53 and abs(e) <= 22
    sign = (b"", b"+", b"-")[int(rng.integers(0, 3))] if sign is None else sign
    for attempt in range(50):
        # trailing zeros are digits of the number tgls_number reads: m * 10^t, e - t must stay in range
        t_max = 0
        while m * 10 ** (t_max + 1) <= 2 ** 53 and e - (t_max + 1) >= -22 and t_max < 6:
            t_max += 1
        t = int(rng.integers(0, t_max + 1)) if rng.random() < 0.4 else 0
        digits, power = b"%d" % (m * 10 ** t), e - t
        nd = len(digits)
        form = int(rng.integers(0, 4))
        if form == 0 and power <= 0:                       # a plain decimal: the dot takes the whole power
            frac = -power
        elif form == 1:                                    # no dot
            frac = None
        else:                                              # the dot anywhere, up to three zeros behind it in front of the digits
            frac = int(rng.integers(0, nd + 4))
        if frac is None:
            body, x = digits, power
        elif frac == 0:
            body, x = digits + b".", power
        elif frac < nd:
            body, x = digits[:nd - frac] + b"." + digits[nd - frac:], power + frac
        else:
            body, x = (b"0" if rng.random() < 0.5 else b"") + b"." + b"0" * (frac - nd) + digits, power + frac
        if x != 0 or rng.random() < 0.2:
            style = int(rng.integers(0, 4))
            body += (b"e", b"E")[style & 1] + (b"-" if x < 0 else b"+" if style & 2 else b"") + \
                (b"%03d" if rng.random() < 0.1 else b"%d") % abs(x)
        if body[:1] != b"." and rng.random() < 0.25:
            body = b"0" * int(rng.integers(1, 1 + max(1, TOKEN_MAX - len(sign) - len(body)))) + body
        tok = sign + body
        if len(tok) <= TOKEN_MAX:
            break
    else:
        tok = sign + b"%de%d" % (m, e)
    assert not defers(tok), tok
    return tok


def plain_spelling(m, k, op):
    """m followed by e+k (the product) or e-k (the quotient)"""
    return b"%de%s%d" % (m, b"+" if op == "*" else b"-", k)


def midpoint_distance(m, k, op):
    """how far the exact m * 10^k (op "*") or m / 10^k (op "/") lies from the nearest midpoint between two adjacent doubles,
    as a Fraction of their spacing: 0 = on a midpoint, 1/2 = a double itself.  Integer arithmetic throughout"""
    num, den = (m * 10 ** k, 1) if op == "*" else (m, 10 ** k)
    s = num.bit_length() - den.bit_length() - 53           # num / den / 2^s in [2^52, 2^54)
    if s >= 0:
        den <<= s
    else:
        num <<= -s
    q = num // den
    if q >= 1 << 53:
        den <<= 1
        q = num // den
    elif q < 1 << 52:
        num <<= 1
        q = num // den
    assert 1 << 52 <= q < 1 << 53
    rem = num - q * den                                    # the part of the value below one spacing: rem / den
    return Fraction(abs(2 * rem - den), 2 * den)


@functools.lru_cache(maxsize=4)
def hard_ranking(seed, sample):
    """`sample` pairs (m log-uniform in [1, 2^53), k in 1..22, either operation), each distinct pair once, sorted by
    midpoint_distance, nearest first: [(distance, m, k, op)]"""
    rng = np.random.default_rng(seed)
    nbits = rng.integers(1, 54, size=sample)
    low = rng.integers(0, 2 ** 53, size=sample, dtype=np.int64)
    ks = rng.integers(1, 23, size=sample)
    ops = rng.integers(0, 2, size=sample)
    pairs = set()
    for b, r, k, o in zip(nbits.tolist(), low.tolist(), ks.tolist(), ops.tolist()):
        pairs.add(((1 << (b - 1)) | (r >> (54 - b)), k, "*" if o else "/"))
    return sorted((midpoint_distance(m, k, op), m, k, op) for m, k, op in pairs)


def hard_cases(seed=20240611, sample=200000, keep=256):
    """the pairs of the sample whose exact quotient or product lies nearest a midpoint between two doubles: where a division
    or multiplication that is not correctly rounded shows first.  -> `keep` distinct (m, k, op).
    Half are quotients and half are products, each the nearest of its operation, so that both always occur.  A product m * 10^k
    can lie ON a midpoint (m * 5^k odd and 54 bits long: the tie that goes to even), a quotient cannot; a log-uniform m makes
    thousands of such ties, all of distance 0 and most with a small m.  They fill half of the products' share at most, those
    of the largest m; the other half are the nearest products that are not ties."""
    ranked = hard_ranking(seed, sample)
    quotients = [(m, k, op) for _, m, k, op in ranked if op == "/"][:keep // 2]
    ties = sorted(((m, k, op) for d, m, k, op in ranked if op == "*" and d == 0), reverse=True)[:keep // 4]
    products = [(m, k, op) for d, m, k, op in ranked if op == "*" and d > 0][:keep - len(quotients) - len(ties)]
    return quotients + ties + products


def blank_line(toks, seps, r=0, eol=b"\n"):
    """a line whose separators are the caller's: seps[0] leads the line, seps[1 + j] stands in front of sample token j,
    seps[-1] trails it (len(seps) == len(toks) + 2, every one but the first and last non-empty); the four leading columns
    are separated by the bytes of BLANKS in turn"""
    assert len(seps) == len(toks) + 2 and all(len(s) > 0 for s in seps[1:-1])
    head = b"1" + BLANKS[r % 5:r % 5 + 1] + b"rs%d" % r + BLANKS[(r + 1) % 5:(r + 1) % 5 + 1] + b"0.5" + \
        BLANKS[(r + 2) % 5:(r + 2) % 5 + 1] + b"%d" % (100 + r)
    return seps[0] + head + b"".join(s + t for s, t in zip(seps[1:], toks)) + seps[-1] + eol


def placed_line(r, line_begin, q, tok, behind, front=(), not_before=0):
    """a line that begins at slab offset line_begin whose token `tok` (sample column len(front)) starts at a slab offset that
    is q modulo 16 and at least not_before bytes into the line, behind a run of spaces and tabs sized for that; `behind`: the
    tokens that follow"""
    head = plain_line(r, list(front), eol=b"").rstrip(b" ")
    first = max(len(head) + 1, not_before)
    run = first - len(head) + (q - (line_begin + first)) % 16
    blanks = bytes((0x20, 0x09)[(r + i) & 1] for i in range(run))
    line = head + blanks + tok + b"".join(b" " + t for t in behind) + b"\n"
    assert (line_begin + line.index(blanks + tok) + run) % 16 == q
    return line
