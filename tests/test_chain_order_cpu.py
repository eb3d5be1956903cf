"""The host model that orders lod_chain_kernel's work list (garlic_amd/host/chain_order.hpp), without a GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chain_order_unit_program(tmp_path):
    """tests/host_unit/chain_order_unit.cpp, compiled here with ASan + UBSan (a stand-alone program, nothing loaded into
    python): the order is a permutation, deterministic, and on equal items (and everywhere else) never simulated slower
    than longest first"""
    exe = str(tmp_path / "chain_order_unit")
    src = os.path.join(ROOT, "tests", "host_unit", "chain_order_unit.cpp")
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                         "-fno-omit-frame-pointer", "-o", exe, src], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "chain_order_unit ok" in r.stdout, (r.stdout + r.stderr)[-3000:]


def test_library_orders_its_list_with_the_model():
    """the library compiles the same header and the constants name the measurement they came from"""
    hip = open(os.path.join(ROOT, "garlic_amd", "csrc", "garlic_hip.hip")).read()
    hpp = open(os.path.join(ROOT, "garlic_amd", "host", "chain_order.hpp")).read()
    assert '#include "../host/chain_order.hpp"' in hip and "garlic_host::chainOrder(" in hip
    assert "profiles/chain_onepass_ab.txt" in hpp
    assert os.path.exists(os.path.join(ROOT, "profiles", "chain_onepass_ab.txt"))
