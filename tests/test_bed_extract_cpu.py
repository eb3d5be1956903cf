"""CPU: what garlic_bed_extract / garlic_bed_get_rows and garlic-lod --keep / --pops promise without a device -- the header's
history entry and version, the Python binding, the tool's help text -- and the keep-file reader through a stand-alone program
built with ASan + UBSan."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("garlic_bed_extract", "garlic_bed_get_rows")


def _header():
    with open(os.path.join(ROOT, "include", "garlic_hip.h")) as f:
        return f.read()


def test_header_lists_both_functions_under_version_8():
    text = _header()
    assert re.search(r"#define GARLIC_HIP_ABI_VERSION 8\b", text)
    history = text[text.index(" * 8: "):text.index("#define GARLIC_HIP_ABI_VERSION")]
    for name in NEW:
        assert name in history, name
        assert re.search(r"\bint %s\(" % name, text), name
    # "likewise": the entry says that nothing that existed changed
    assert re.search(r"garlic_bed_extract,\s*\*?\s*garlic_bed_get_rows \(likewise\)", history)


def test_abi_binds_both_functions():
    with open(os.path.join(ROOT, "garlic_amd", "abi.py")) as f:
        text = f.read()
    for name in NEW:
        assert '"%s"' % name in text, name                  # SYMBOLS: build() resolves every one of them
        assert "L.%s.argtypes" % name in text, name
    from garlic_amd import abi
    assert abi.ABI_VERSION == 8
    assert set(NEW) <= set(abi.SYMBOLS)
    assert callable(abi.Bed.extract) and callable(abi.Bed.get_rows)


def test_help_names_keep_and_pops():
    tool = os.path.join(ROOT, "garlic_amd", "host", "garlic-lod")
    if not os.path.exists(tool):
        pytest.fail("garlic_amd/host/garlic-lod is not built (build() makes it)")
    r = subprocess.run([tool, "--help"], capture_output=True, text=True)
    text = r.stdout + r.stderr
    assert "--keep" in text and "--pops" in text, text[-2000:]


def test_keep_file_reader(tmp_path):
    """tests/host_unit/bed_keep_unit.cpp (compiled here, ASan + UBSan; a stand-alone program): the .fam's order kept,
    duplicates, an unknown pair (error text with the pair and the line number), extra columns, CRLF, an empty result, the
    family IDs in first-seen order"""
    exe = str(tmp_path / "bed_keep_unit")
    src = os.path.join(ROOT, "tests", "host_unit", "bed_keep_unit.cpp")
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                         "-fno-omit-frame-pointer", "-o", exe, src], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and "bed_keep_unit ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
    assert "line 3" in r.stderr and "(B a1)" in r.stderr            # the unknown pair's message
