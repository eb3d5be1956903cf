"""BGZF members for the inflate tests: a BGZF writer over Python's zlib, a bit writer for hand-made fixed-Huffman streams,
the named cases, the random members and their corrupted twins.  The expected bytes of every member come from
zlib.decompress(member, 31), never from the code under test."""
import functools
import random
import struct
import zlib

OK, BAD_BLOCK_TYPE, BAD_CODE_LENGTHS, BAD_SYMBOL, BAD_DISTANCE, INPUT_ENDED, OUTPUT_FULL, OUTPUT_SHORT, BAD_CRC = range(9)
ANY_STATUS = -1          # zlib refuses the member: any status but OK
STATUS_OR_BYTES = -2     # zlib accepts it although a header byte differs: a status, or exactly zlib's bytes


def header(member_bytes, extra_before=b"", extra_after=b""):
    bc = b"BC" + struct.pack("<HH", 2, member_bytes - 1)
    extra = extra_before + bc + extra_after
    return b"\x1f\x8b\x08\x04" + b"\x00" * 4 + b"\x00\xff" + struct.pack("<H", len(extra)) + extra


def member_of_raw(raw, data, extra_before=b"", extra_after=b"", crc=None, isize=None):
    """a BGZF member around a raw deflate stream; crc / isize default to those of `data`"""
    n = 12 + len(extra_before) + 6 + len(extra_after) + len(raw) + 8
    assert n <= 65536, n
    foot = struct.pack("<II", zlib.crc32(data) if crc is None else crc, len(data) if isize is None else isize)
    return header(n, extra_before, extra_after) + raw + foot


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return c.compress(data) + c.flush()


def member(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, **kw):
    return member_of_raw(deflate(data, level, strategy), data, **kw)


EOF_BLOCK = member(b"")
assert EOF_BLOCK == bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def split(blob):
    """the members of a BGZF byte string"""
    out, at = [], 0
    while at < len(blob):
        xlen = struct.unpack_from("<H", blob, at + 10)[0]
        extra, k, size = blob[at + 12:at + 12 + xlen], 0, None
        while k < len(extra):
            slen = struct.unpack_from("<H", extra, k + 2)[0]
            if extra[k:k + 2] == b"BC" and slen == 2:
                size = struct.unpack_from("<H", extra, k + 4)[0] + 1
            k += 4 + slen
        out.append(blob[at:at + size])
        at += size
    return out


def isize_of(m):
    return struct.unpack_from("<I", m, len(m) - 4)[0]


def write_bgzf(data, block_bytes=65280, level=6, eof=True):
    """data as a BGZF byte string in blocks of block_bytes (an int, or a function of the offset)"""
    out, at = [], 0
    while at < len(data):
        n = block_bytes(at) if callable(block_bytes) else block_bytes
        out.append(member(data[at:at + n], level))
        at += n
    return b"".join(out) + (EOF_BLOCK if eof else b"")


class Bits:
    """a deflate bit stream: codes most significant bit first, everything else least significant first"""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value, nbits):
        self.acc |= value << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, value, nbits):
        self.put(int(format(value, "0%db" % nbits)[::-1], 2), nbits)

    def done(self):
        if self.n:
            self.put(0, 8 - self.n)
        return bytes(self.out)


LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


def fixed_stream(tokens):
    """one final fixed-Huffman block from tokens: an int is a literal, (length, distance) a match"""
    b = Bits()
    b.put(1, 1)
    b.put(1, 2)

    def litlen(s):
        if s < 144:
            b.code(0x30 + s, 8)
        elif s < 256:
            b.code(0x190 + s - 144, 9)
        elif s < 280:
            b.code(s - 256, 7)
        else:
            b.code(0xC0 + s - 280, 8)

    for t in tokens:
        if isinstance(t, int):
            litlen(t)
            continue
        length, dist = t
        k = max(i for i in range(29) if LEN_BASE[i] <= length) if length < 258 else 28
        litlen(257 + k)
        b.put(length - LEN_BASE[k], LEN_EXTRA[k])
        d = max(i for i in range(30) if DIST_BASE[i] <= dist)
        b.code(d, 5)
        b.put(dist - DIST_BASE[d], DIST_EXTRA[d])
    litlen(256)
    return b.done()


def replay(tokens):
    out = bytearray()
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            for _ in range(t[0]):
                out.append(out[-t[1]])
    return bytes(out)


def hand_made(tokens):
    raw, data = fixed_stream(tokens), replay(tokens)
    assert zlib.decompress(raw, -15) == data
    return member_of_raw(raw, data)


@functools.lru_cache(None)
def text():
    """about 56 KB of VCF-like lines: 200 samples of GT:GQ"""
    rng = random.Random(11)
    lines = []
    for k in range(40):
        cells = ["%d%s%d:%d" % (rng.randrange(2), "|/"[rng.randrange(2)], rng.randrange(2), rng.randrange(100)) for _ in range(200)]
        lines.append("\t".join(["7", str(1000 + 37 * k), "rs%d" % k, "A", "C", ".", "PASS", ".", "GT:GQ"] + cells))
    return ("\n".join(lines) + "\n").encode()


def text_like(rng, n):
    t = text()
    at = rng.randrange(len(t))
    return ((t[at:] + t) * (n // len(t) + 2))[:n]


@functools.lru_cache(None)
def clean_cases():
    """[(name, member)]: every member inflates; its bytes are zlib.decompress(member, 31)"""
    t, short = text(), b"ACGT\n" * 3
    rng = random.Random(5)
    cases = [("stored short", member(short, 0)), ("stored text", member(t, 0)),
             ("fixed short", member(short, 6)), ("fixed text", member(t, 6, zlib.Z_FIXED)),
             ("dynamic 1", member(t, 1)), ("dynamic 6", member(t, 6)), ("dynamic 9", member(t, 9)),
             ("huffman only", member(t, 6, zlib.Z_HUFFMAN_ONLY)), ("rle", member(t, 6, zlib.Z_RLE))]
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 9)
    raw = b""
    for k, at in enumerate(range(0, len(t), 20000)):
        raw += c.compress(t[at:at + 20000]) + c.flush(zlib.Z_SYNC_FLUSH if k & 1 else zlib.Z_FULL_FLUSH)
    cases.append(("flushes", member_of_raw(raw + c.flush(), t)))
    cases.append(("incompressible", member(bytes(rng.randrange(256) for _ in range(65280)), 6)))
    full = (t * 2)[:65536]
    cases += [("full size %d" % lv, member(full, lv)) for lv in range(1, 10)]
    far = [rng.randrange(32, 127) for _ in range(32768)]
    cases += [("distance 1 length 258", hand_made([65, (258, 1)])),
              ("distance 32768 length 258", hand_made(far + [(258, 32768)])),
              ("length 3", hand_made([97, 98, 99, (3, 3)])),
              ("distance = produced", hand_made([97, 98, 99, 100, 101, (4, 5)])),
              ("eof block", EOF_BLOCK),
              ("extra subfield before BC", member(short, 6, extra_before=b"XY" + struct.pack("<H", 3) + b"abc")),
              ("extra subfield behind BC", member(short, 6, extra_after=b"ZZ" + struct.pack("<H", 0)))]
    for name, m in cases:
        assert len(m) <= 65536 and len(zlib.decompress(m, 31)) == isize_of(m), name
    return cases


def _refused(m):
    try:
        zlib.decompress(m, 31)
    except zlib.error:
        return True
    return False


@functools.lru_cache(None)
def corrupt_cases():
    """[(name, member, status)]: zlib refuses every one"""
    t = text()
    good = member(t, 6)
    flip = lambda m, at: m[:at] + bytes([m[at] ^ 0x10]) + m[at + 1:]
    n = len(t)
    raw = deflate(t, 6)
    over = Bits()
    over.put(1, 1), over.put(2, 2), over.put(0, 5), over.put(0, 5), over.put(15, 4)
    for _ in range(19):
        over.put(1, 3)
    tokens = [97, 98, 99, 100, 101, (4, 6)]
    cases = [("crc byte flipped", flip(good, len(good) - 7), BAD_CRC),
             ("isize one more", member_of_raw(raw, t, isize=n + 1), OUTPUT_SHORT),
             ("isize one less", member_of_raw(raw, t, isize=n - 1), OUTPUT_FULL),
             ("block type 3", member_of_raw(b"\x07\x00", b""), BAD_BLOCK_TYPE),
             ("distance one beyond", member_of_raw(fixed_stream(tokens), b"abcdeabcd"), BAD_DISTANCE),
             ("cut short", member_of_raw(raw[:-100], t), INPUT_ENDED),
             ("over-subscribed code lengths", member_of_raw(over.done() + b"\x00" * 4, b""), BAD_CODE_LENGTHS)]
    for name, m, _ in cases:
        assert _refused(m), name
    return cases


STRATEGIES = [zlib.Z_DEFAULT_STRATEGY, zlib.Z_FILTERED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FIXED]


@functools.lru_cache(None)
def random_members(count=2000, seed=2024):
    """[(member, data)]: random level, strategy and length 0 .. 65,280 over text-like and random bytes"""
    rng = random.Random(seed)
    out = []
    for _ in range(count):
        n = rng.randrange(65281)
        data = text_like(rng, n) if rng.randrange(3) else rng.randbytes(n)
        m = member(data, rng.randrange(10), STRATEGIES[rng.randrange(5)])
        out.append((m, data))
    return out


@functools.lru_cache(None)
def corrupted_members(count=2000, seed=2024):
    """[(member, expect, bytes)]: the random members with 1 to 3 random bytes overwritten.  expect: ANY_STATUS where zlib
    refuses; OK with zlib's bytes where it accepts and the 12 + XLEN bytes of header are intact; else STATUS_OR_BYTES"""
    rng = random.Random(seed + 1)
    out = []
    for m, _ in random_members(count, seed):
        b = bytearray(m)
        where = [rng.randrange(len(b)) for _ in range(rng.randrange(1, 4))]
        for at in where:
            b[at] = rng.randrange(256)
        b = bytes(b)
        try:
            data = zlib.decompress(b, 31)
        except zlib.error:
            out.append((b, ANY_STATUS, b""))
            continue
        out.append((b, OK if b[:18] == m[:18] else STATUS_OR_BYTES, data))
    return out


def records(items):
    """the byte string the host unit reads: per member u32 length, the member, i32 expect, u32 length, the expected bytes"""
    out = []
    for m, expect, data in items:
        out.append(struct.pack("<I", len(m)) + m + struct.pack("<iI", expect, len(data)) + data)
    return b"".join(out)
