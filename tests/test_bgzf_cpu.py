"""The BGZF decoder (garlic_amd/csrc/inflate.hpp) and the block walk (garlic_amd/host/bgzf_blocks.hpp), without a GPU."""
import os
import subprocess
import zlib

import bgzf_cases as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_cases_are_what_they_claim():
    """zlib's own view of the named cases: block types, sizes, and that the hand-made streams decode"""
    cases = dict(bc.clean_cases())
    first_block_type = lambda m: (m[12 + int.from_bytes(m[10:12], "little")] >> 1) & 3
    final = lambda m: m[12 + int.from_bytes(m[10:12], "little")] & 1
    assert first_block_type(cases["stored short"]) == 0 and final(cases["stored short"]) == 1
    assert first_block_type(cases["fixed short"]) == 1 and first_block_type(cases["fixed text"]) == 1
    assert all(first_block_type(cases["dynamic %d" % lv]) == 2 for lv in (1, 6, 9))
    assert first_block_type(cases["huffman only"]) == 2 and first_block_type(cases["rle"]) == 2
    assert first_block_type(cases["incompressible"]) == 0
    assert all(bc.isize_of(cases["full size %d" % lv]) == 65536 for lv in range(1, 10))
    assert bc.isize_of(cases["distance 32768 length 258"]) == 32768 + 258
    assert 50000 < len(bc.text()) < 60000
    assert bc.split(bc.write_bgzf(bc.text(), 1000))[-1] == bc.EOF_BLOCK


def test_inflate_unit_under_sanitizers(tmp_path):
    """tests/host_unit/inflate_unit.cpp, compiled here with ASan + UBSan (a stand-alone program, nothing loaded into python):
    every case, 2,000 random members and the same with 1 to 3 bytes overwritten, each from and into heap buffers of the exact
    sizes; the block walk over whole and broken files"""
    exe = str(tmp_path / "inflate_unit")
    src = os.path.join(ROOT, "tests", "host_unit", "inflate_unit.cpp")
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                         "-fno-omit-frame-pointer", "-o", exe, src], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    clean = bc.clean_cases()
    (tmp_path / "clean.rec").write_bytes(bc.records([(m, bc.OK, zlib.decompress(m, 31)) for _, m in clean]))
    (tmp_path / "corrupt.rec").write_bytes(bc.records([(m, status, b"") for _, m, status in bc.corrupt_cases()]))
    (tmp_path / "random.rec").write_bytes(bc.records([(m, bc.OK, zlib.decompress(m, 31)) for m, _ in bc.random_members()]))
    (tmp_path / "random_corrupt.rec").write_bytes(bc.records(bc.corrupted_members()))
    members = [m for _, m in clean] + [bc.EOF_BLOCK]
    (tmp_path / "walk.bgzf").write_bytes(b"".join(members))
    at, lines = 0, []
    for m in members:
        lines.append("%d %d %d" % (at, len(m), bc.isize_of(m)))
        at += len(m)
    (tmp_path / "walk.txt").write_text("\n".join(lines) + "\n")
    two = members[0] + members[4]
    (tmp_path / "cut_header.bgzf").write_bytes(two + members[5][:9])
    (tmp_path / "past_end.bgzf").write_bytes(two + members[5][:-1])
    gz = zlib.compressobj(6, zlib.DEFLATED, 31)
    (tmp_path / "then_gzip.bgzf").write_bytes(two + gz.compress(b"plain gzip\n") + gz.flush())
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "inflate_unit ok: %d members" % (len(clean) + len(bc.corrupt_cases()) + 4000) in r.stdout, \
        (r.stdout + r.stderr)[-3000:]
