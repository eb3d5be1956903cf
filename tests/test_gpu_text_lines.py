"""GPU: the line index of a slab of device text (garlic_text_lines) against a Python restatement of text::SlabLines::take
(garlic_amd/host/text_slabs.hpp).

text_lines_* work on tiles of 256 aligned 16-byte pieces (4 KB) and number the line ends by a popcount scan inside the tile
and a scan over the tiles: the cases put line ends at every offset of a piece and at the borders of the slab, lines across
many tiles, more than 256 tiles, and the text at every alignment."""
import numpy as np
import pytest

import bgzf_cases as bc
from garlic_amd import abi

pytestmark = pytest.mark.gpu


def take(slab, last, seen=0):
    """SlabLines::take: (begin, end, number, consumed, seen)"""
    begin, end, number, at, n = [], [], [], 0, len(slab)
    while at < n:
        nl = slab.find(b"\n", at)
        if nl < 0 and not last:
            break
        e = nl if nl >= 0 else n
        blank = e == at or (e == at + 1 and slab[at:at + 1] == b"\r")
        seen += 1
        if not blank:
            begin.append(at), end.append(e), number.append(seen)
        at = e + 1 if nl >= 0 else n
    return begin, end, number, at, seen


def on_device(text, offset=0, poison=0x0A):
    """the text at `offset` bytes past a 16-byte aligned device address, line ends as poison on each side"""
    import torch
    buf = torch.full((len(text) + 160,), poison, dtype=torch.uint8, device="cuda")
    at = (-buf.data_ptr()) % 16 + 64 + offset
    if text:
        buf[at:at + len(text)] = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    return buf, buf.data_ptr() + at


def check(ctx, text, last, offset=0, seen=0, head_bytes=0, tag=None):
    buf, ptr = on_device(text, offset)
    got = abi.text_lines(ctx, ptr, len(text), last, seen=seen, head_bytes=head_bytes)
    begin, end, number, consumed, seen_out = take(text, last, seen)
    tag = (tag, last, offset)
    assert got["begin"].tolist() == begin and got["end"].tolist() == end and got["number"].tolist() == number, tag
    assert got["consumed"] == consumed and got["seen"] == seen_out, (tag, got["consumed"], consumed, got["seen"], seen_out)
    if head_bytes:
        want = np.zeros((len(begin), head_bytes), dtype=np.uint8)
        for k, (b, e) in enumerate(zip(begin, end)):
            head = text[b:min(e, b + head_bytes)]
            want[k, :len(head)] = np.frombuffer(head, dtype=np.uint8)
        assert np.array_equal(got["heads"], want), tag
    return got


@pytest.mark.parametrize("last", [0, 1])
def test_borders_of_the_slab(gpu_ctx, last):
    for text in [b"", b"abc", b"\n", b"\nabc", b"abc\n", b"\n\n", b"\r", b"\r\n", b"a\r\n", b"\r\r\n", b"ab\n\r", b"ab\n\rc", b"ab\ncd",
                 b"\n\r\n\n\r\nab\n\n\n\r\n\r\ncd\r\n\n", b"x" * 5 + b"\n" + b"y" * 70000 + b"\n" + b"tail"]:
        check(gpu_ctx, text, last, seen=17, head_bytes=8, tag=text[:20])


@pytest.mark.parametrize("last", [0, 1])
def test_a_line_end_at_every_offset_of_a_piece(gpu_ctx, last):
    for at in range(34):
        check(gpu_ctx, b"a" * at + b"\n" + b"b" * (40 - at), last, tag=at)
        check(gpu_ctx, b"a" * at + b"\n", last, tag=at)                 # ... and as the last byte


@pytest.mark.parametrize("last", [0, 1])
def test_every_alignment_of_the_text(gpu_ctx, last):
    text = bc.text()[:9000] + b"\n\r\n" + bc.text()[9000:20011]
    for offset in range(16):
        check(gpu_ctx, text, last, offset=offset, head_bytes=32, tag="aligned")


def test_heads_shorter_equal_and_longer_than_the_lines(gpu_ctx):
    text = b"".join(b"%d" % (10 ** k) + b"\n" for k in range(0, 40)) + b"no end"
    for head_bytes in (1, 7, 8, 9, 16, 64):
        check(gpu_ctx, text, 1, head_bytes=head_bytes, tag=head_bytes)
        check(gpu_ctx, text, 0, offset=5, head_bytes=head_bytes, tag=head_bytes)


def test_100000_short_lines_across_the_tiles(gpu_ctx):
    rng = np.random.default_rng(8)
    kinds = [b"a", b"bc", b"def", b"\r", b""]
    text = b"".join(kinds[k] + b"\n" for k in rng.integers(0, 5, 100000))
    assert len(text) > 256 * 4096 // 8
    got = check(gpu_ctx, text, 0, offset=3, head_bytes=4, tag="short lines")
    assert 50000 < len(got["begin"]) < 70000
    check(gpu_ctx, text + b"zz", 1, offset=11, tag="short lines, a last one without end")
    many_tiles = bc.text() * 25                  # more than 256 tiles: a second round of the scan over the tiles
    assert len(many_tiles) > 257 * 4096
    check(gpu_ctx, many_tiles + b"cut", 0, offset=7, head_bytes=16, tag="many tiles")


def test_capacity_is_reported_and_then_enough(gpu_ctx):
    text = b"one\ntwo\n\nthree\n"
    buf, ptr = on_device(text)
    with pytest.raises(abi.GarlicError) as e:
        abi.text_lines(gpu_ctx, ptr, len(text), 1, capacity=2)
    assert e.value.code == abi.ERR_RANGE and "3 lines" in str(e.value)
    got = abi.text_lines(gpu_ctx, ptr, len(text), 1, capacity=3, head_bytes=5)
    assert got["begin"].tolist() == [0, 4, 9] and got["number"].tolist() == [1, 2, 4]
    assert bytes(got["heads"][2]) == b"three"
