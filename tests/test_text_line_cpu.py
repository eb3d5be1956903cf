"""What the text parsers share (garlic_amd/csrc/text_line.hpp), without a GPU."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "garlic_amd", "csrc")


def test_text_eq_mask_unit_under_sanitizers(tmp_path):
    """tests/host_unit/text_eq_mask_unit.cpp, compiled here with ASan + UBSan (a stand-alone program, nothing loaded into
    python): the byte-parallel compare against the plain byte loop"""
    exe = str(tmp_path / "text_eq_mask_unit")
    src = os.path.join(ROOT, "tests", "host_unit", "text_eq_mask_unit.cpp")
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                         "-fno-omit-frame-pointer", "-o", exe, src], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "text_eq_mask_unit ok" in r.stdout, (r.stdout + r.stderr)[-3000:]


def test_the_line_walk_is_written_once():
    """the piece load, the first line end, the keep mask and the status store stand in text_line.hpp and nowhere else under
    csrc/, and the four parsers call them"""
    once = {"piece load": "0x0Au << (8 * (k & 3))", "first line end": "__ffsll((unsigned long long)has)",
            "keep mask": "(1u << (int)(end - mine)) - 1u", "status store": "0x7FFFFFFFull"}
    for what, mark in once.items():
        holders = sorted(f for f in os.listdir(CSRC) if f.endswith((".hpp", ".hip", ".inc")) and mark in open(os.path.join(CSRC, f)).read())
        assert holders == ["text_line.hpp"], (what, holders)
    for header, kernel in [("vcf_kernels.hpp", "vcf_parse_kernel"), ("tped_kernels.hpp", "tped_parse_kernel"),
                           ("tgls_kernels.hpp", "tgls_parse_kernel"), ("vcf_gl_kernels.hpp", "tgls_vcf_parse_kernel")]:
        text = open(os.path.join(CSRC, header)).read()
        body = text[text.index("\n" + kernel + "("):]
        for call in ["text_line_of(", "text_load_piece(", "text_first_end(", "text_keep_mask(", "text_write_status("]:
            assert call in body, (kernel, call)
    hip = open(os.path.join(CSRC, "garlic_hip.hip")).read()
    assert len(re.findall(r"the offsets must ascend inside the slab", hip)) == 1
    assert '#include "vcf_kernels.hpp"' not in open(os.path.join(CSRC, "tgls_kernels.hpp")).read()


def test_text_slabs_unit_under_sanitizers(tmp_path):
    """tests/host_unit/text_slabs_unit.cpp, compiled here with ASan + UBSan (a stand-alone program, nothing loaded into
    python): the slab walk of garlic_amd/host/text_slabs.hpp, pushed and pulled, over files it writes"""
    exe = str(tmp_path / "text_slabs_unit")
    src = os.path.join(ROOT, "tests", "host_unit", "text_slabs_unit.cpp")
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                         "-o", exe, src, "-lz"], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "text_slabs_unit ok" in r.stdout, (r.stdout + r.stderr)[-3000:]


def test_the_slab_loop_is_written_once():
    """the read / cut / refuse loop stands in text_slabs.hpp; the loaders call it and declare no static function ahead"""
    host = os.path.join(ROOT, "garlic_amd", "host")
    loops = {f: open(os.path.join(host, f)).read().count("} while (!rd.eof ||") for f in os.listdir(host) if f.endswith((".hpp", ".cpp"))}
    assert {f: n for f, n in loops.items() if n} == {"text_slabs.hpp": 1}
    src = open(os.path.join(host, "garlic_host.cpp")).read()
    assert src.count("forEachSlab(") + src.count("slabsOrFail(") >= 6 and "rd.next(" not in src
    loaders = src[src.index("void loadBedData("):src.index("std::vector<FreqData *> *readFreqData(")]
    assert not re.findall(r"^static [^\n{}]*\)\s*;\s*$", loaders, flags=re.M)
